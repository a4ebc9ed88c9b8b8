"""What the CPU and the GPU suite of the sessions' keyed tag share: hash keys and words, a difference the CRC-32 does not see, synthetic batches for
the verify step and what it must give for them, from crc32_words and the Python-integer tag of tests/polyhash_ref.py."""
import numpy as np

import polyhash_ref as R

P = R.P
OK, EDECODE = 0, -9


def hash_keys(rng):
    """(hi, lo): the field value 0, 1, p itself (taken as 0), p - 1, all ones, a random one"""
    return [R.key_words(k) for k in (0, 1, P, P - 1, (1 << 64) - 1, int(rng.integers(0, 1 << 63)) * 2 + 1)]


def words(rng, n):
    return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def masked(w, bits):
    m = np.array(w[:(bits + 31) // 32], np.uint32)
    if bits % 32:
        m[-1] &= np.uint32((0xFFFFFFFF << (32 - bits % 32)) & 0xFFFFFFFF)
    return m


def crc_collision(q, K, bits, rng):
    """a non-zero difference d (words) with crc32_words(K ^ d) == crc32_words(K): the CRC is affine over GF(2), so L(e) = crc(e) ^ crc(0) is linear, and
    33 single-bit differences at the same length have a combination on which the 32-bit L vanishes -- one Gaussian elimination finds it"""
    W = (bits + 31) // 32
    zero = np.zeros(W, np.uint32)
    c0 = q.crc32_words(zero, bits)
    pos = sorted(int(p) for p in rng.choice(bits, 33, replace=False))
    rows = []
    for j, p in enumerate(pos):
        e = zero.copy()
        e[p >> 5] = np.uint32(0x80000000 >> (p & 31))
        rows.append((q.crc32_words(e, bits) ^ c0, 1 << j))
    basis = {}                                              # leading bit -> (value, combination)
    for v, comb in rows:
        while v:
            top = v.bit_length() - 1
            if top not in basis:
                basis[top] = (v, comb)
                break
            v, comb = v ^ basis[top][0], comb ^ basis[top][1]
        if not v:
            d = zero.copy()
            for j, p in enumerate(pos):
                if (comb >> j) & 1:
                    d[p >> 5] ^= np.uint32(0x80000000 >> (p & 31))
            assert d.any()
            return d
    raise AssertionError("33 vectors of 32 bits are dependent")


def batch(q, rng, bits_list, r, shared, collide=()):
    """a synthetic batch for the verify step, one block per entry of bits_list, its kind by position: 0 a good block, 1 ok with another CRC, 2 a failed
    decode; a block named in `collide` is a good block whose decoded row differs from Alice's key by a difference the CRC does not see.  Key rows of
    W + 1 words, decoded rows of 3 more, garbage everywhere past a block's length"""
    n, W = len(bits_list), max((b + 31) // 32 for b in bits_list)
    Wk, Wn = W + 1, W + 4
    out, keys = words(rng, n * Wn).reshape(n, Wn), words(rng, n * Wk).reshape(n, Wk)
    alice = out[:, :Wk].copy()
    want, ok, kinds = np.zeros(n, np.uint32), np.ones(n, np.int32), np.arange(n) % 3
    for b, bits in enumerate(bits_list):
        nw = (bits + 31) // 32
        if b in collide:
            kinds[b] = 0
            out[b, :nw] ^= crc_collision(q, alice[b], bits, rng)
        want[b] = q.crc32_words(alice[b], bits) ^ (0x10 if kinds[b] == 1 else 0)
        ok[b] = kinds[b] != 2
    hk = words(rng, 2 * r) if shared else words(rng, n * 2 * r).reshape(n, 2 * r)
    return dict(out=out, keys=keys, key_bits=np.array(bits_list, np.int32), crc_want=want, ok=ok, iters=rng.integers(1, 60, n).astype(np.int32), hash_keys=hk,
                kinds=kinds, alice=alice, r=r, shared=shared)


def expected(q, B):
    """what the verify step must give for a batch, from crc32_words and the Python-integer tag"""
    n, Wk = B["keys"].shape
    keys, tags = np.zeros((n, Wk), np.uint32), np.zeros((n, 2 * B["r"]), np.uint32)
    status, flips, crc = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    for b in range(n):
        bits = int(B["key_bits"][b])
        nw = (bits + 31) // 32
        crc[b] = q.crc32_words(B["out"][b], bits)
        good = bool(B["ok"][b]) and crc[b] == B["crc_want"][b]
        status[b] = OK if good else EDECODE
        if good:
            keys[b, :nw] = masked(B["out"][b], bits)
            flips[b] = sum(bin(int(x)).count("1") for x in keys[b, :nw] ^ masked(B["keys"][b], bits))
            tags[b] = R.tags(B["out"][b], bits, B["hash_keys"] if B["shared"] else B["hash_keys"][b])
        else:
            keys[b, :nw] = B["keys"][b, :nw]
    return dict(status=status, corrected=flips, iterations=B["iters"], crc=crc, keys=keys, tags=tags)


def check_verdict(got, want):
    for f in ("status", "corrected", "iterations", "crc", "keys", "tags"):
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape and (got[f] == want[f]).all(), f

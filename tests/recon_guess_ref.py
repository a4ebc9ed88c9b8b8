"""The verdict of a guessing round inside a reconciliation session (csrc/qldpc_recon_guess_core.h), restated in numpy / Python for the tests, and the
synthetic sources both suites settle.  The CRC here is zlib's, not the library's.

Two keys that differ in fewer than 33 adjacent bits never share a CRC-32, so two PASSING trials with different keys need a collision: `collision(kb)`
is the pattern inside the last 33 valid bits (it contains the last valid bit) that leaves the CRC of any key of kb >= 33 bits unchanged."""
import zlib

import numpy as np

FIELDS = ("tried", "winner", "n_ok", "n_pass", "ambiguous", "trial_iterations")
OK, EDECODE = 0, -9


def mask_words(kb):
    nw = (kb + 31) // 32
    m = np.full(nw, 0xFFFFFFFF, np.uint32)
    if kb & 31:
        m[-1] = (0xFFFFFFFF << (32 - (kb & 31))) & 0xFFFFFFFF
    return m


def crc(words, kb):
    m = mask_words(kb)
    return zlib.crc32((np.asarray(words, np.uint32)[:m.size] & m).astype(">u4").tobytes())


def settle(g, rows, ok, iters, keys, key_bits, want, first):
    """-> dict of the arrays qldpc_recon_guess_settle_host writes (keys: words past a key's length stay 0)"""
    T, n = 1 << g, keys.shape[0]
    out = dict(status=np.zeros(n, np.int32), corrected=np.zeros(n, np.int32), iterations=np.zeros(n, np.int32), crc=np.zeros(n, np.int32),
               keys=np.zeros_like(keys), guess=np.zeros((n, 6), np.int32), passed=np.zeros(n * T, np.int32), trial_crc=np.zeros(n * T, np.uint32))
    for s in range(n):
        kb = int(key_bits[s])
        m = mask_words(kb)
        r, o, it = rows[s * T:(s + 1) * T], ok[s * T:(s + 1) * T], iters[s * T:(s + 1) * T]
        c = np.array([crc(r[t], kb) for t in range(T)], np.uint32)
        p = (o != 0) & (c == np.uint32(want[s]))
        win = int(np.flatnonzero(p)[0]) if p.any() else -1
        amb = int(any(((r[t, :m.size] ^ r[win, :m.size]) & m).any() for t in np.flatnonzero(p))) if win >= 0 else 0
        out["passed"][s * T:(s + 1) * T], out["trial_crc"][s * T:(s + 1) * T] = p, c
        out["guess"][s] = (1, win, int((o != 0).sum()), int(p.sum()), amb, int(it.sum()))
        out["status"][s] = OK if win >= 0 else EDECODE
        out["iterations"][s] = first[s] + (it[win] if win >= 0 else 0)
        out["crc"][s] = np.uint32(c[max(win, 0)]).view(np.int32)
        if win >= 0:
            new = r[win, :m.size] & m
            out["keys"][s, :m.size] = new
            out["corrected"][s] = sum(bin(int(x)).count("1") for x in (keys[s, :m.size] & m) ^ new)
        else:
            out["keys"][s, :m.size] = keys[s, :m.size]
    return out


def collision(kb):
    """uint32 [ceil(kb/32)]: a non-zero pattern within bits kb - 33 .. kb - 1 with crc(x ^ pattern) == crc(x) for every x of kb bits (kb >= 33)"""
    nw = (kb + 31) // 32
    zero = crc(np.zeros(nw, np.uint32), kb)

    def unit(b):
        e = np.zeros(nw, np.uint32)
        e[b >> 5] = np.uint32(0x80000000 >> (b & 31))
        return e

    basis = {}
    for i, b in enumerate(range(kb - 33, kb)):
        v, c = crc(unit(b), kb) ^ zero, 1 << i
        while v and (v.bit_length() - 1) in basis:
            bv, bc = basis[v.bit_length() - 1]
            v, c = v ^ bv, c ^ bc
        if not v:
            pat = np.zeros(nw, np.uint32)
            for k in range(33):
                if (c >> k) & 1:
                    pat ^= unit(kb - 33 + k)
            return pat
        basis[v.bit_length() - 1] = (v, c)
    raise AssertionError("33 vectors of 32 bits are dependent")


def source(rng, g, kb, Wk, Wn, kinds):
    """one synthetic source: `kinds` [T] says what each trial decoded to -- 'a' Alice's key (passes), 'c' her key ^ collision (passes, another key; kb >= 33),
    'w' a zero-syndrome trial with another key (wrong CRC), 'f' a failed trial that happens to hold Alice's key (right CRC, ok = 0), 'x' a failed trial.
    Every row gets random bits past key_bits (padding of the last key word and the parity part).  -> rows [T, Wn], ok, iters [T], key row [Wk], want, first"""
    T, nw = 1 << g, (kb + 31) // 32
    m = mask_words(kb)
    alice = rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32) & m
    rows = rng.integers(0, 2 ** 32, (T, Wn), dtype=np.uint64).astype(np.uint32)
    ok = np.zeros(T, np.int32)
    for t, kind in enumerate(kinds):
        noise = rows[t, :nw] & ~m
        if kind in "acf":
            rows[t, :nw] = alice | noise
        if kind == "c":
            rows[t, :nw] ^= collision(kb)
        if kind == "w" and not ((rows[t, :nw] ^ alice) & m).any():
            rows[t, 0] ^= np.uint32(0x80000000)
        ok[t] = kind in "acw"
    key = rng.integers(0, 2 ** 32, Wk, dtype=np.uint64).astype(np.uint32)
    key[:nw] = (alice ^ (rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32) & rng.integers(0, 2 ** 32, nw, dtype=np.uint64).astype(np.uint32) & m)) | (key[:nw] & ~m)
    return rows, ok, rng.integers(1, 60, T).astype(np.int32), key, crc(alice, kb), int(rng.integers(1, 60))


def random_kinds(rng, T, kb, p_pass, p_wrong):
    u = rng.random(T)
    kinds = np.where(u < p_pass, "a", np.where(u < p_pass + p_wrong, "w", np.where(u < p_pass + p_wrong + 0.1, "f", "x")))
    if kb >= 33:
        kinds = np.where((kinds == "a") & (rng.random(T) < 0.3), "c", kinds)
    return "".join(kinds)


def batch(rng, g, kb, Wk, Wn, kinds_list):
    """sources stacked as the calls take them -> dict(rows, ok, iters, keys, key_bits, want, first)"""
    parts = [source(rng, g, k, Wk, Wn, kinds) for k, kinds in zip(kb, kinds_list)]
    return dict(rows=np.concatenate([p[0] for p in parts]), ok=np.concatenate([p[1] for p in parts]), iters=np.concatenate([p[2] for p in parts]),
                keys=np.stack([p[3] for p in parts]), key_bits=np.array(kb, np.int32), want=np.array([p[4] for p in parts], np.uint32),
                first=np.array([p[5] for p in parts], np.int32))


def hand_built(T=8):
    """the named cases -> {name: (kinds, key_bits, (winner, n_ok, n_pass, ambiguous))}; T >= 8"""
    x = "x" * (T - 4)
    return {
        "a zero-syndrome trial with a wrong CRC below the winner": ("xwa" + x + "x", 1000, (2, 2, 1, 0)),
        "two passing trials with equal keys": ("xaxa" + x, 1000, (1, 2, 2, 0)),
        "two passing trials whose keys differ in the last valid bits": ("axc" + x + "x", 1000, (0, 2, 2, 1)),
        "the same with the other key first": ("cxa" + x + "x", 33, (0, 2, 2, 1)),
        "two passing trials that differ only in padding bits": ("axxa" + x, 1001, (0, 2, 2, 0)),
        "no passing trial": ("wfxw" + x, 1000, (-1, 2, 0, 0)),
    }


def same(got, want):
    """every array of two settle dicts, exactly"""
    plain = lambda a: np.stack([a[f] for f in FIELDS], axis=1) if np.asarray(a).dtype.names else np.asarray(a)
    for k in want:
        g, w = plain(got[k]), plain(want[k])
        if g.shape != w.shape or not (g.astype(np.int64) == w.astype(np.int64)).all():
            return k
    return None

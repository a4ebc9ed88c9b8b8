"""numpy restatement of the Monte-Carlo frame definition (include/qldpc.h, "Monte-Carlo FER loop"), shared by tests/test_mc.py and
tests/test_mc_gpu.py.  Nothing here calls the library.

    generator  Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, key = (seed lo, seed hi)
    source     info word j of frame i = output word j % 4 at counter (j / 4, 0, i_lo, i_hi), MSB-first, bits past K cleared
    channel    VN v of frame i flips iff u < floor(p[class(v)] 2^32), u = output word v % 4 at counter (v / 4, 1, i_lo, i_hi)
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable arrays of 32-bit values -> the four output words (uint64 arrays holding 32-bit values)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def _stream(seed, first, n, stream, count):
    """output words 0 .. count-1 of the stream (0 source, 1 channel) of frames first .. first + n - 1 -> uint32 [n, count]"""
    idx = [(int(first) + f) & 0xFFFFFFFFFFFFFFFF for f in range(n)]
    lo = np.array([i & 0xFFFFFFFF for i in idx], np.uint64)[:, None]
    hi = np.array([i >> 32 for i in idx], np.uint64)[:, None]
    blocks = np.arange((count + 3) // 4, dtype=np.uint64)[None, :]
    out = philox(blocks, np.uint64(stream), lo, hi, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.stack(np.broadcast_arrays(*out), axis=-1).reshape(n, -1)[:, :count].astype(np.uint32)


def classes(K, N, info_bits_pos=None, vn_class=None):
    """the class map a NULL vn_class stands for: channel (0) at info_bits_pos, pinned (1) elsewhere"""
    if vn_class is not None:
        return np.asarray(vn_class, np.uint8)
    cls = np.ones(N, np.uint8)
    cls[np.arange(K) if info_bits_pos is None else np.asarray(info_bits_pos)] = 0
    return cls


def pack(bits):
    """bits [n, m] of 0/1 -> uint32 [n, ceil(m/32)], MSB-first"""
    b = np.asarray(bits, np.uint8)
    pad = (-b.shape[1]) % 32
    b = np.concatenate([b, np.zeros((b.shape[0], pad), np.uint8)], axis=1)
    return np.packbits(b, axis=1, bitorder="big").view(">u4").astype(np.uint32)


def unpack(words, m):
    w = np.ascontiguousarray(words, dtype=np.uint32).astype(">u4")
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="big")[:, :m]


def frames(K, N, seed, qber, first, n, info_bits_pos=None, vn_class=None, parity_ber=0.0):
    """(info words [n, ceil(K/32)], flip words [n, ceil(N/32)]) of frames first .. first + n - 1"""
    Wk = (K + 31) // 32
    info = _stream(seed, first, n, 0, Wk)
    if K % 32:
        info[:, -1] &= np.uint32((0xFFFFFFFF << (32 - K % 32)) & 0xFFFFFFFF)
    thr = np.array([int(np.floor(float(qber) * 2.0 ** 32)), int(np.floor(float(parity_ber) * 2.0 ** 32)), 0], np.uint64)
    u = _stream(seed, first, n, 1, N).astype(np.uint64)
    return info, pack(u < thr[classes(K, N, info_bits_pos, vn_class)][None, :])


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)).sum())

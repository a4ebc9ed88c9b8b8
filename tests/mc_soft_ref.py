"""numpy restatement of the quantised soft-output channel of the Monte-Carlo loop (include/qldpc.h, "Quantised soft-output channels"),
shared by tests/test_mc_soft.py and tests/test_mc_soft_gpu.py.  Nothing here calls the library but tables(), which takes the 64-level AWGN
table from it (awgn_table() below is its restatement by math.erfc).

    draw       u = output word v % 4 of Philox at counter (v / 4, 3, i_lo, i_hi) for VN v of frame i
    level      #{k : u >= cum[b][k]} = np.searchsorted(cum[b], u, side="right"), b = the codeword bit
    classes    0: LLR = value[level]; 1: LLR = +-PIN by b, the sign inverted iff u < floor(parity_ber 2^32); 2: LLR = 0
    flip       b = 0 and LLR < 0, or b = 1 and LLR > 0
"""
import math

import numpy as np

import mc_ref

PIN = np.float32(23.025850929840455)
TWO32 = 2 ** 32


def llr_frames(K, N, seed, table, first, n, cw_bits=None, info_bits_pos=None, vn_class=None, parity_ber=0.0):
    """(LLRs [n, N] float32, flip words [n, ceil(N/32)]) of frames first .. first + n - 1; cw_bits [n, N] of 0/1 (None = all-zero)"""
    cum0, cum1, value = (np.asarray(a) for a in table)
    u = mc_ref._stream(seed, first, n, 3, N).astype(np.uint64)
    b = np.zeros((n, N), np.uint8) if cw_bits is None else np.asarray(cw_bits, np.uint8)
    cls = mc_ref.classes(K, N, info_bits_pos, vn_class)[None, :]
    level = np.where(b == 1, np.searchsorted(cum1.astype(np.uint64), u, side="right"), np.searchsorted(cum0.astype(np.uint64), u, side="right"))
    llr = value.astype(np.float32)[level]
    inverted = u < np.uint64(int(math.floor(float(parity_ber) * 2.0 ** 32)))
    llr = np.where(cls == 1, np.where((b == 1) != inverted, -PIN, PIN), llr)
    llr = np.where(cls == 2, np.float32(0.0), llr).astype(np.float32)
    return llr, mc_ref.pack(np.where(b == 1, llr > 0, llr < 0))


def awgn_table(sigma, rmax=3.0, maxq=31):
    """floor(r / rmax * maxq) clamped to [-maxq - 1, maxq] for r = (1 - 2 b) + sigma n, by math.erfc -> (cum0, cum1, value)"""
    q = 2 * maxq + 2
    cum = [[int(math.floor(TWO32 * (0.5 * math.erfc(-(((k - maxq) * rmax / maxq - (1 - 2 * b)) / sigma) / math.sqrt(2.0))))) for k in range(q - 1)]
           for b in (0, 1)]
    return np.array(cum[0], np.uint64), np.array(cum[1], np.uint64), np.arange(q, dtype=np.float32) - np.float32(maxq + 1)


def tables(q):
    """the table shapes of the tests: the 64-level AWGN table of the library, Q = 2, and Q = 256 with runs of equal thresholds whose rows
    start with 0 and end with 2^32"""
    rng = np.random.default_rng(11)
    out = {"awgn64": q.mc_awgn_table(0.8414, 3.0, 31)}
    # Q = 2: a binary asymmetric channel, 10 % / 20 % on the wrong side; level 0 says "bit 1"
    out["q2"] = (np.array([int(0.1 * TWO32)], np.uint64), np.array([int(0.8 * TWO32)], np.uint64), np.array([-1.5, 2.5], np.float32))
    rows = []
    for _ in (0, 1):
        r = np.sort(rng.integers(0, TWO32, 255, dtype=np.uint64))
        r[40:60] = r[40]                                                    # runs of equal thresholds: levels of probability zero
        r[100:103] = r[100]
        r[:3] = 0                                                           # levels 0 .. 2 cannot occur
        r[-5:] = TWO32                                                      # nor can the last five
        rows.append(np.sort(r))
    value = rng.permutation(np.linspace(-20.0, 20.0, 256)).astype(np.float32)
    value[7] = 0.0                                                          # a level that says nothing: no flip whatever was sent
    out["q256"] = (rows[0], rows[1], value)
    return out


def mixed_classes(N):
    cls = (np.arange(N) * 7 // 5 % 3).astype(np.uint8)
    assert all((cls == c).sum() > N // 5 for c in (0, 1, 2))
    return cls


def gf2_rank(A):
    """rank over GF(2) of a 0/1 matrix"""
    A = np.array(A, np.uint8) & 1
    rank = 0
    for c in range(A.shape[1]):
        rows = np.nonzero(A[rank:, c])[0]
        if rows.size == 0:
            continue
        p = rank + rows[0]
        A[[rank, p]] = A[[p, rank]]
        others = np.nonzero(A[:, c])[0]
        others = others[others != rank]
        A[others] ^= A[rank]
        rank += 1
        if rank == A.shape[0]:
            break
    return rank

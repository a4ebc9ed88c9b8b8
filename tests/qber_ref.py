"""The rule of the syndrome-weight QBER estimate (csrc/qldpc_qber_core.h) restated in numpy and Python integers: VN states, counts by effective
degree, tables, score and argmax.  Test infrastructure: written from the rule's text, not from the library's code."""
import math
import os

import numpy as np

SCALE = 1 << 24
EXACT, ERASED, NOISY = 0, 1, 2


def unpack_row(words, n):
    w = np.asarray(words, dtype=np.uint32).ravel()
    return np.array([(int(w[i >> 5]) >> (31 - (i & 31))) & 1 for i in range(n)], np.uint8)


def pack_row(bits):
    b = np.asarray(bits, dtype=np.uint8)
    out = np.zeros((b.size + 31) // 32, np.uint32)
    for i in np.flatnonzero(b):
        out[i >> 5] |= np.uint32(1 << (31 - (int(i) & 31)))
    return out


def states(N, bits, vn_class=None, n_channel=None, erase=None, known=None, value=None):
    """-> (state[N], value[N]) from unpacked 0/1 arrays (None = absent)"""
    cls = np.zeros(N, np.int64) if vn_class is None else np.asarray(vn_class).astype(np.int64)
    nch = N if n_channel is None else int(n_channel)
    er = np.zeros(N, np.uint8) if erase is None else np.asarray(erase)
    kn = np.zeros(N, np.uint8) if known is None else np.asarray(known)
    st = np.empty(N, np.int64)
    val = np.asarray(bits).astype(np.uint8).copy()
    for v in range(N):
        if kn[v]:
            st[v] = EXACT
            val[v] = value[v]
        elif cls[v] == 2 or er[v]:
            st[v] = ERASED
        elif cls[v] == 1 or v >= nch:
            st[v] = EXACT
        else:
            st[v] = NOISY
    return st, val


def counts(var, chk, N, M, D, bits, vn_class=None, n_channel=None, synd=None, erase=None, known=None, value=None):
    """counts[D + 1][2] of one frame as Python ints; (var, chk) = the code's edges, everything else unpacked 0/1 arrays"""
    st, val = states(N, bits, vn_class, n_channel, erase, known, value)
    d = [0] * M
    u = [0 if synd is None else int(synd[c]) for c in range(M)]
    dead = [False] * M
    for v, c in zip(var, chk):
        v, c = int(v), int(c)
        if st[v] == ERASED:
            dead[c] = True
        if st[v] == NOISY:
            d[c] += 1
        u[c] ^= int(val[v])
    out = [[0, 0] for _ in range(D + 1)]
    for c in range(M):
        if dead[c]:
            continue
        out[d[c]][0] += 1
        out[d[c]][1] += u[c]
    return out


def grid(n_grid, q_lo, q_hi):
    lo, hi = float(np.float32(q_lo)), float(np.float32(q_hi))
    return [lo * (hi / lo) ** (k / (n_grid - 1)) for k in range(n_grid)]


def p_d(q, d):
    return (1.0 - (1.0 - 2.0 * q) ** d) / 2.0


def tables(D, n_grid, q_lo, q_hi):
    """L1, L0 as lists of Python ints [D + 1][n_grid] (row 0 zero), q as doubles"""
    qs = grid(n_grid, q_lo, q_hi)
    L1 = [[0] * n_grid] + [[int(round(math.log(p_d(q, d)) * SCALE)) for q in qs] for d in range(1, D + 1)]
    L0 = [[0] * n_grid] + [[int(round(math.log1p(-p_d(q, d)) * SCALE)) for q in qs] for d in range(1, D + 1)]
    return L1, L0, qs


def score(cnt, L1, L0, k):
    return sum(int(cnt[d][1]) * int(L1[d][k]) + (int(cnt[d][0]) - int(cnt[d][1])) * int(L0[d][k]) for d in range(1, len(cnt)))


def argmax(cnt, L1, L0):
    """the smallest k of maximal score, -1 without an informative check of degree >= 1; Python integers throughout"""
    if sum(int(cnt[d][0]) for d in range(1, len(cnt))) == 0:
        return -1
    n_grid = len(L1[0])
    S = [score(cnt, L1, L0, k) for k in range(n_grid)]
    return S.index(max(S))


COMBOS = ("null", "class", "syndrome", "erase_known", "all")


def toy_edges():
    """N = 45, M = 7: check c takes VNs c, c + 7, ... (degrees 6 - 7) plus VN 44 on checks 0 and 6: N is no multiple of 32"""
    var, chk = [], []
    for v in range(44):
        var.append(v); chk.append(v % 7)
    var += [44, 44]; chk += [0, 6]
    return 45, 7, np.array(var, np.int32), np.array(chk, np.int32)


def frames(rng, N, M, F, combo):
    """random inputs of F frames as unpacked 0/1 arrays (None = that input is absent): dict(bits [F, N], cls [N], nch [F], synd [F, M],
    erase / known / value [F, N]).  `erase_known` and `all` make VN 1 of every frame both erased and known, and known on a class-2 VN."""
    f = dict(bits=rng.integers(0, 2, (F, N)).astype(np.uint8), cls=None, nch=None, synd=None, erase=None, known=None, value=None)
    if combo in ("class", "all"):
        f["cls"] = rng.choice(np.array([0, 0, 0, 0, 1, 2], np.uint8), N)
        f["nch"] = rng.integers(0, N + 1, F).astype(np.int32)
        f["nch"][0] = N
    if combo in ("syndrome", "all"):
        f["synd"] = rng.integers(0, 2, (F, M)).astype(np.uint8)
    if combo in ("erase_known", "all"):
        f["erase"] = (rng.random((F, N)) < 0.04).astype(np.uint8)
        f["known"] = (rng.random((F, N)) < 0.06).astype(np.uint8)
        f["value"] = rng.integers(0, 2, (F, N)).astype(np.uint8)
        f["erase"][:, 1] = 1
        f["known"][:, 1] = 1
        if f["cls"] is not None:
            f["cls"][2] = 2
            f["known"][:, 2] = 1
    return f


CODES = ("peg504", "ira1280", "toy45")


def make_code(q, name):
    """the three codes of the suites: PEGReg504x1008 (check degrees 5 - 8), a small IRA code, the toy above"""
    if name == "peg504":
        return q.Code.from_alist(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "PEGReg504x1008.alist"))
    if name == "ira1280":
        return q.Code.ira(1280, 1024)
    N, M, var, chk = toy_edges()
    return q.Code.from_edges(N, M, var, chk)


def host_counts(q, code, f, i):
    """the library's host mirror on frame i of a frames() dict"""
    pick = lambda a: None if a is None else q.pack_bits(a[i])
    return q.qber_counts_host(code, q.pack_bits(f["bits"][i]), f["cls"], None if f["nch"] is None else int(f["nch"][i]), pick(f["synd"]), pick(f["erase"]),
                              pick(f["known"]), pick(f["value"]))


def frame_counts(var, chk, N, M, D, f, i):
    """counts of frame i of a frames() dict"""
    pick = lambda a: None if a is None else a[i]
    return counts(var, chk, N, M, D, f["bits"][i], f["cls"], None if f["nch"] is None else f["nch"][i], pick(f["synd"]), pick(f["erase"]), pick(f["known"]),
                  pick(f["value"]))


def sigma(cnt, q):
    """the spread of the estimate at q from the counts: sigma^-2 = SUM_d n_d p_d'^2 / (p_d (1 - p_d)), p_d' = d (1 - 2 q)^(d - 1)"""
    info = 0.0
    for d in range(1, len(cnt)):
        n = int(cnt[d][0])
        if n:
            p = p_d(q, d)
            info += n * (d * (1.0 - 2.0 * q) ** (d - 1)) ** 2 / (p * (1.0 - p))
    return info ** -0.5 if info > 0 else float("inf")

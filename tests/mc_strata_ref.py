"""numpy restatement of the fixed-weight frame definition and of the strata estimate (include/qldpc.h, "Fixed-weight error strata"), shared by
tests/test_mc_strata.py and tests/test_mc_strata_gpu.py.  Nothing here calls the library.

    key        u_v = the stream-1 word of VN v of frame i (mc_ref._stream), coarsened to u'_v = u_v >> (32 - key_bits)
    flip set   the w channel-class VNs smallest in the order (u'_v, v): a lexsort, not a select
    others     a pinned VN flips iff u_v < floor(parity_ber 2^32), a punctured VN never
    estimate   exact binomial weights by math.comb over the exact fraction of q, P^ piecewise linear between strata
"""
import functools
import math
from fractions import Fraction

import numpy as np

import mc_ref


def keys(N, seed, first, n, key_bits=32):
    """(raw words, coarsened keys) of VNs 0 .. N-1 of frames first .. first + n - 1 -> uint64 [n, N] each"""
    u = mc_ref._stream(seed, first, n, 1, N).astype(np.uint64)
    return u, u >> np.uint64(32 - (int(key_bits) or 32))


def frames(K, N, seed, weights, first, n, key_bits=32, info_bits_pos=None, vn_class=None, parity_ber=0.0):
    """(info words [n, ceil(K/32)], flip words [n, ceil(N/32)]) of frames first .. first + n - 1, frame f at weight weights[f]"""
    info = mc_ref.frames(K, N, seed, 0.0, first, n, info_bits_pos, vn_class)[0]
    cls = mc_ref.classes(K, N, info_bits_pos, vn_class)
    u, key = keys(N, seed, first, n, key_bits)
    chan = np.nonzero(cls == 0)[0]
    flips = (cls == 1)[None, :] & (u < np.uint64(int(np.floor(float(parity_ber) * 2.0 ** 32))))
    weights = np.broadcast_to(np.asarray(weights), (n,))
    for f in range(n):
        order = np.lexsort((chan, key[f, chan]))          # by key, equal keys by VN
        flips[f, chan[order[:int(weights[f])]]] = True
    return info, mc_ref.pack(flips)


def boundary_ties(K, N, seed, weight, first, n, key_bits, info_bits_pos=None, vn_class=None):
    """per frame: does the key of the last VN taken equal the key of the first VN left out (bool [n])"""
    cls = mc_ref.classes(K, N, info_bits_pos, vn_class)
    key = np.sort(keys(N, seed, first, n, key_bits)[1][:, cls == 0], axis=1)
    return key[:, weight - 1] == key[:, weight]


@functools.lru_cache(maxsize=None)
def binom_int(n, w, a, d):
    """the numerator of Binom(n, a / d)(w) over the denominator d^n: an exact integer"""
    return math.comb(n, w) * a ** w * (d - a) ** (n - w)


def fer(n_channel, weights, frames_, frame_errors, qber):
    """the four outputs of the estimate.  The binomial weights are exact: qber, a double, is the fraction a / d, and every b(w) is kept as its
    integer numerator over d^n; the hat functions add small integer factors; a sum becomes a double by ONE correctly rounded division of two
    integers, and the sums over the strata (positive terms) by math.fsum of such doubles"""
    q = Fraction(qber)                                      # the double, exactly
    a, d, n = q.numerator, q.denominator, int(n_channel)
    D = d ** n
    w = [int(x) for x in weights]
    b = lambda x: binom_int(n, x, a, d)                     # noqa: E731
    c = []
    for s in range(len(w)):
        Ll = w[s] - w[s - 1] if s > 0 else 1
        Lr = w[s + 1] - w[s] if s + 1 < len(w) else 1
        A = b(w[s]) * Ll * Lr
        if s > 0:
            A += Lr * sum(b(x) * (x - w[s - 1]) for x in range(w[s - 1] + 1, w[s]))
        if s + 1 < len(w):
            A += Ll * sum(b(x) * (w[s + 1] - x) for x in range(w[s] + 1, w[s + 1]))
        c.append((A, D * Ll * Lr))                          # c_s = A / (D Ll Lr)
    fe, fr = [int(e) for e in frame_errors], [int(f) for f in frames_]
    out0 = math.fsum((A * e) / (B * f) for (A, B), e, f in zip(c, fe, fr))
    below = sum(b(x) for x in range(0, w[0])) / D
    above = sum(b(x) for x in range(w[-1] + 1, n + 1)) / D
    var = math.fsum((A * A * e * (f - e)) / (B * B * f ** 3) for (A, B), e, f in zip(c, fe, fr))
    return [out0, below, above, math.sqrt(var)]

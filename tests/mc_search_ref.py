"""numpy restatement of the puncture-pattern definition (include/qldpc.h, "Monte-Carlo FER loop"), shared by tests/test_mc_search.py and
tests/test_mc_search_gpu.py, next to mc_ref.py whose generator it uses.  Nothing here calls the library.

    key        u_c = output word c % 4 of Philox4x32-10 at counter (c / 4, 2, p_lo, p_hi), key = (seed lo, seed hi); u'_c = u_c >> (32 - key_bits)
    selection  the n_punct candidates smallest in the order (u'_c, c): a lexsort, equal keys to the lower candidate index
"""
import numpy as np

import mc_ref


def keys(seed, pattern, n_cand, key_bits=32):
    """u'_c of candidates 0 .. n_cand-1 of pattern `pattern` (uint64 holding key_bits-bit values)"""
    p = int(pattern) & 0xFFFFFFFFFFFFFFFF
    blocks = np.arange((n_cand + 3) // 4, dtype=np.uint64)
    out = mc_ref.philox(blocks, np.uint64(2), np.uint64(p & 0xFFFFFFFF), np.uint64(p >> 32), int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    u = np.stack(np.broadcast_arrays(*out), axis=-1).reshape(-1)[:n_cand]
    return u >> np.uint64(32 - key_bits)


def pattern(seed, pattern, n_cand, n_punct, key_bits=32):
    """the chosen candidate indices, ascending (int32)"""
    u = keys(seed, pattern, n_cand, key_bits)
    order = np.lexsort((np.arange(n_cand), u))                 # the last key is the primary one: by u', then by c
    return np.sort(order[:n_punct]).astype(np.int32)


def rows(seed, first, n, cand, n_punct, N, key_bits=32):
    """erase rows [n, ceil(N/32)] (uint32, MSB-first) of patterns first .. first + n - 1 over the candidate VNs cand"""
    cand = np.asarray(cand, np.int64)
    bits = np.zeros((n, N), np.uint8)
    for i in range(n):
        bits[i, cand[pattern(seed, int(first) + i, cand.size, n_punct, key_bits)]] = 1
    return mc_ref.pack(bits)

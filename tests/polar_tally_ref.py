"""numpy restatement of the genie-aided polar code construction (include/qldpc.h, "genie-aided code construction"; the rule is
qcrypto-ldpc_amd/csrc/qldpc_polar_tally_core.h), shared by tests/test_polar_construct.py and tests/test_polar_construct_gpu.py, on top of the SC
decoder of tests/polar_ref.py.  Calls nothing of the library.

    genie     L = the leaf beliefs of polar_ref.decode with every position frozen to the frame's true row
    tie       L == 0 (-0.0 too);  wrong: L != 0 and (L < 0) != u
    tally     [2, N]: the wrong frames and the ties of every position;  score = 2 wrong + ties
    order     ascending reliability: by (score descending, rank in the prior ascending)
    K         the largest K whose last K positions of an order have a score sum <= the bound
"""
import numpy as np

import polar_ref as R


def tally(llr, u_bits, messages="i8", maxq=31):
    """llr [F, N], u_bits uint8 [F, N] -> uint64 [2, N]"""
    N = llr.shape[1]
    leaf = R.decode(llr, np.ones(N, bool), u_bits, messages, maxq)[2]
    tie = leaf == 0
    wrong = ~tie & ((leaf < 0) != (np.asarray(u_bits) == 1))
    return np.stack([wrong.sum(axis=0), tie.sum(axis=0)]).astype(np.uint64)


def score(t):
    return 2 * t[0].astype(np.int64) + t[1].astype(np.int64)


def order(t, prior=None):
    """-> int32 [N], ascending reliability"""
    N = t.shape[1]
    rank = np.arange(N)
    if prior is not None:
        rank = np.empty(N, np.int64)
        rank[np.asarray(prior)] = np.arange(N)
    return np.lexsort((rank, -score(t))).astype(np.int32)      # the last key is the first criterion


def best_k(t, order_, bound):
    """the largest K with sum(score[order[N - K:]]) <= bound"""
    cum = np.cumsum(score(t)[np.asarray(order_)[::-1]])
    return int(np.searchsorted(cum, bound, side="right"))

"""CPU suite: the chain table behind the posterior form of the flooding run (qldpc_code_chain_table, qldpc_kernels_fpost.h) and the
graph side of its eligibility.  No GPU compute."""
import os

import numpy as np
import pytest

NONE = 255


def codes(q):
    return {"ira": q.Code.ira(4096, 3277, 0.125, 11, 3, 7), "ira_low_rate": q.Code.ira(2048, 1024, 0.125, 11, 3, 7),
            "ira_peg": q.Code.ira_peg(1024, 768, 0.125, 11, 3, 2, 7)}


@pytest.mark.parametrize("name", ["ira", "ira_low_rate", "ira_peg"])
def test_chain_table_agrees_with_the_edge_list(q, name):
    code = codes(q)[name]
    assert code.is_ira and code.max_cn_degree <= 27
    tab = code.chain_table()
    assert tab is not None and tab.shape == (code.M, 4) and tab.dtype == np.uint8
    K, M = code.N - code.M, code.M
    var, chk = code.edges()                                   # CN-major: a check's edges in row order
    first = np.searchsorted(chk, np.arange(M + 1))
    rows = [var[first[c]:first[c + 1]] for c in range(M)]
    # check 0 has no left edge, the last VN has degree 1 (no check M shares it)
    assert tab[0, 0] == NONE and tab[0, 2] == NONE and tab[M - 1, 3] == NONE
    assert (var == K + M - 1).sum() == 1 and chk[var == K + M - 1][0] == M - 1
    for c in range(M):
        l, r, lnb, rnb = (int(t) for t in tab[c])
        assert rows[c][r] == K + c
        chain_here = {r}
        if c > 0:
            assert rows[c][l] == K + c - 1 and rows[c - 1][lnb] == K + c - 1 and lnb == tab[c - 1, 1]
            chain_here.add(l)
        if c + 1 < M:
            assert rows[c + 1][rnb] == K + c and rnb == tab[c + 1, 0]
        # every other edge of the row is an information edge
        assert all((v >= K) == (k in chain_here) for k, v in enumerate(rows[c]))
    # every chain VN has exactly the edges the table names
    deg = np.bincount(var, minlength=code.N)
    assert (deg[K:K + M - 1] == 2).all() and deg[K + M - 1] == 1


def test_graphs_without_the_chain_do_not_qualify(q, gold):
    peg = q.Code.from_alist(os.path.join(gold, "PEGReg504x1008.alist"))
    assert not peg.is_ira and peg.chain_table() is None
    # a chain with one link moved: VN K + 1 on checks {1, 3} instead of {1, 2}
    code = q.Code.ira(512, 384, 0.125, 11, 3, 7)
    var, chk = code.edges()
    K = code.N - code.M
    chk2 = chk.copy()
    hit = np.flatnonzero((var == K + 1) & (chk == 2))
    assert hit.size == 1
    chk2[hit[0]] = 3
    order = np.argsort(chk2, kind="stable")
    broken = q.Code.from_edges(code.N, code.M, var[order], chk2[order])
    assert broken.chain_table() is None


def test_check_degrees_above_27_do_not_qualify(q):
    """the packed state word holds 27 sign bits and a 5-bit index"""
    code = q.Code.ira(4096, 3686, 0.125, 11, 3, 7)            # rate 0.9: 36 information edges per check
    assert code.is_ira and code.max_cn_degree > 27
    assert code.chain_table() is None

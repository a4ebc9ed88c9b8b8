"""The sweep over operating points of a table channel (qldpc_mc_sweep_tables), host suite: qldpc_mc_sweep_tables_check_host -- every argument
check the device call runs first -- over accepted configurations and over every refusal with its status code, through the Python front end
and, where the front end cannot say it, through the C structures; and the sanitizer pass of tests/c/mc_sweep_tables_sanitize.c."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mc_soft_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, BATCH = 1998, 192
ESIZE, EINVAL = -6, -1


@pytest.fixture(scope="module")
def tables(q):
    t = mc_soft_ref.tables(q)
    return [t["q2"], t["awgn64"], q.mc_awgn_table(1.0), t["q256"]]      # 2, 64, 64 and 256 levels


def status(q, *args, **kw):
    try:
        q.mc_sweep_tables_check(*args, **kw)
    except q.QldpcError as e:
        return e.status
    return 0


def test_accepted_configurations(q, tables):
    order = np.random.default_rng(3).permutation(N)[:60].astype(np.int32)      # not ascending
    assert status(q, N, BATCH, tables, max_frames=150, chunk=32) == 0
    assert status(q, N, BATCH, tables, labels=[1.0, 1.5, 2.0, 2.35], n_punct=[0, 20, 40, 60], punct_order=order, max_frames=150, max_frame_errors=7, chunk=1) == 0
    assert status(q, N, BATCH, tables, n_punct=[60, 0, 60, 0], punct_order=order, chunk=BATCH, first_frame=2 ** 64 - 1, max_frames=2 ** 64 - 1) == 0
    assert status(q, N, BATCH, tables, n_punct=[0, 0, 0, 0], punct_order=None) == 0                      # n_order = 0 with every n_punct = 0
    assert status(q, N, BATCH, tables[:1]) == 0                                                             # P = 1
    assert status(q, N, BATCH, [tables[i % 4] for i in range(q.MC_SWEEP_MAX_POINTS)]) == 0              # P = 4 096
    assert status(q, N, 1, tables, chunk=1) == 0 and status(q, 1, 1, tables[:1]) == 0
    assert status(q, 1 << 20, (1 << 13) - 1, tables[:1]) == 0                                               # one frame short of 2^31 lanes of four VNs


def test_refusals_with_their_codes(q, tables):
    order = np.arange(100, 160, dtype=np.int32)
    c0, c1, value = tables[1]
    decreasing = c0.copy()
    decreasing[5] = decreasing[4] - 1
    above = c1.copy()
    above[-1] = 2 ** 32 + 1
    at_the_top = c1.copy()
    at_the_top[-1] = 2 ** 32                                                  # 2^32 itself is a level that nothing reaches, not an error
    assert status(q, N, BATCH, [(c0, at_the_top, value)]) == 0
    # per table, the codes of qldpc_mc_set_channel
    assert status(q, N, BATCH, tables + [(c0[:0], c1[:0], value[:1])]) == ESIZE                          # 1 level
    assert status(q, N, BATCH, [(np.zeros(256, np.uint64), np.zeros(256, np.uint64), np.zeros(257, np.float32))] + tables) == ESIZE      # 257 levels
    assert status(q, N, BATCH, tables[:2] + [(decreasing, c1, value)] + tables[2:]) == EINVAL
    assert status(q, N, BATCH, tables + [(c0, above, value)]) == EINVAL
    # the rest, the codes of qldpc_mc_sweep
    assert status(q, N, BATCH, []) == ESIZE                                                                 # P = 0
    assert status(q, N, BATCH, [tables[0]] * (q.MC_SWEEP_MAX_POINTS + 1)) == ESIZE
    assert status(q, N, BATCH, tables, chunk=BATCH + 1) == ESIZE
    assert status(q, N, BATCH, tables, chunk=-1) == ESIZE
    assert status(q, N, BATCH, tables, max_frames=0) == ESIZE
    assert status(q, N, BATCH, tables, n_punct=[0, 1, 2, 61], punct_order=order) == ESIZE                # n_punct > n_order
    assert status(q, N, BATCH, tables, n_punct=[0, -1, 2, 3], punct_order=order) == ESIZE
    assert status(q, N, BATCH, tables, n_punct=[0, 1, 2, 3], punct_order=None) == ESIZE                  # n_order = 0: every n_punct must be 0
    assert status(q, N, BATCH, tables, n_punct=[0, 1, 2, 3], punct_order=np.concatenate([order, order[:1]])) == EINVAL      # a repeated VN
    assert status(q, N, BATCH, tables, n_punct=[0, 1, 2, 3], punct_order=np.concatenate([order, [N]])) == EINVAL            # a VN outside [0, N)
    assert status(q, N, BATCH, tables, n_punct=[0, 1, 2, 3], punct_order=np.concatenate([order, [-1]])) == EINVAL
    assert status(q, 1 << 20, 1 << 13, tables[:1]) == ESIZE                                                 # 2^13 frames of 2^18 quads: 2^31 lanes
    assert status(q, 0, BATCH, tables) == ESIZE and status(q, N, 0, tables) == ESIZE
    with pytest.raises(q.QldpcError) as e:
        q.mc_sweep_tables_check(N, BATCH, tables, labels=[1.0, 2.0])                                     # the front end's own: one label per table
    assert e.value.status == ESIZE


def test_refusals_through_the_c_structures(q, tables):
    """a missing array and non-zero reserved words, which the Python front end cannot express"""
    check = q._L.qldpc_mc_sweep_tables_check_host
    order = np.arange(10, dtype=np.int32)

    def cfg_of():
        return q._mc_sweep_tables_cfg(tables, None, [0, 1, 2, 3], order, 0, 100, 0, 0, "test")

    cfg, keep = cfg_of()
    assert check(N, BATCH, C.byref(cfg)) == 0
    assert check(N, BATCH, None) == EINVAL
    for where in ("cfg", "point", "table", "value", "cum", "points", "order"):
        cfg, keep = cfg_of()
        pts = keep[0]
        if where == "cfg":
            cfg.reserved[0] = 1
        elif where == "point":
            pts[2].reserved = 1
        elif where == "table":
            pts[3].table.reserved[1] = 1
        elif where == "value":
            pts[1].table.value = None
        elif where == "cum":
            pts[1].table.cum[0] = None
        elif where == "points":
            cfg.points = None
        else:
            cfg.punct_order = None
        assert check(N, BATCH, C.byref(cfg)) == EINVAL, where
    # the order of the checks is qldpc_mc_sweep's: reserved words of the cfg before the sizes, the sizes before the arrays
    cfg, keep = cfg_of()
    cfg.reserved[0], cfg.n_points = 1, 0
    assert check(N, BATCH, C.byref(cfg)) == EINVAL
    cfg, keep = cfg_of()
    cfg.points, cfg.max_frames = None, 0
    assert check(N, BATCH, C.byref(cfg)) == ESIZE
    cfg, keep = cfg_of()
    cfg.n_points = 2                                                         # a prefix of the points is a sweep of its own
    assert check(N, BATCH, C.byref(cfg)) == 0


def test_host_side_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mc_sweep_tables_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "mc_sweep_tables_sanitize.c"),
                           os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr

"""CPU suite: the merged form of the syndrome-weight QBER count (qldpc_qber_counts_merged_host: runs of checks across erased accumulator VNs are one
observation each) against the restatement of the rule in tests/qber_merge_ref.py, and what it buys where half of the parity is punctured.  No GPU compute."""
import os
import subprocess

import numpy as np
import pytest

import qber_merge_ref as mref
import qber_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGE_CODES = ((1280, 1024), (5120, 4096))


@pytest.fixture(scope="module")
def codes(q):
    out = {}
    for N, K in MERGE_CODES:
        code = q.Code.ira(N, K)
        out[(N, K)] = (code, *code.edges())
    return out


@pytest.mark.parametrize("shape", MERGE_CODES)
@pytest.mark.parametrize("combo", qber_ref.COMBOS)
def test_merged_mirror_is_the_rule(q, codes, shape, combo):
    """count for count: parity erased evenly spaced at 25 / 50 / 60 %, at random at 40 %, and the constructed cases, under the five input combinations"""
    code, var, chk = codes[shape]
    N, M = code.N, code.M
    assert mref.is_chain(var, chk, N, M)
    rng = np.random.default_rng(N * 7 + len(combo))
    named = combo != "null" and combo != "class"
    F = len(mref.PATTERNS) + (len(mref.NAMED) if named else 0)
    f, names = mref.overlay(rng, var, chk, N, M, qber_ref.frames(rng, N, M, F, combo), named)
    notes = {}
    for i in range(F):
        detail = {}
        want = np.array(mref.frame_counts(var, chk, N, M, f, i, detail), np.uint32)
        got = mref.host_counts(q, code, f, i)
        assert got.shape == (mref.ROWS, 2) and (got == want).all(), (shape, combo, names[i], np.flatnonzero((got != want).any(axis=1)))
        notes[names[i]] = detail["runs"]
    if combo != "syndrome":
        return
    # the clean inputs (no class map, no random erasures): every case the rule names is really there
    run = lambda name, h: next(r for r in notes[name] if r["head"] == h)
    assert run("head0", 0)["tail"] == 2 and run("head0", 0)["left_out"] is None
    assert run("last", M - 2)["tail"] == M - 1 and run("last", M - 2)["left_out"] == "erased"
    assert run("known_link", 10)["tail"] == 11 and run("known_link", 12)["tail"] == 13
    assert run("erased_info", 20)["tail"] == 21 and run("erased_info", 20)["left_out"] == "erased"
    assert run("long", 30)["tail"] == 46 and run("long", 30)["left_out"] == "long"
    assert run("long", 50)["tail"] == 65 and run("long", 50)["left_out"] is None
    assert run("long", 100)["left_out"] == "long"
    if shape == MERGE_CODES[0]:      # four checks of 16 information edges and more
        assert run("degree", 70)["tail"] == 73 and run("degree", 70)["left_out"] == "degree" and run("degree", 70)["d"] > 63
        counted = [r for rs in notes.values() for r in rs if r["left_out"] is None]
        assert any(3 in r["mults"] for r in counted), "the socket shuffle of Code.ira(1280, 1024) no longer puts a VN on three nearby checks"
        assert any(2 in r["mults"] for r in counted)


@pytest.mark.parametrize("combo", qber_ref.COMBOS)
def test_without_a_link_merged_is_unmerged(q, codes, combo):
    """no erased VN K + c, c < M - 1: the merged counts are the unmerged ones padded to 64 rows (erased information VNs and an erased last parity VN stay)"""
    code, var, chk = codes[MERGE_CODES[0]]
    N, M, K, D = code.N, code.M, code.N - code.M, code.max_cn_degree
    rng = np.random.default_rng(5 + len(combo))
    f = qber_ref.frames(rng, N, M, 3, combo)
    if f["cls"] is not None:
        f["cls"][K:N - 1][f["cls"][K:N - 1] == 2] = 1
    if f["erase"] is not None:
        f["erase"][:, K:N - 1] = 0
        f["erase"][0, N - 1] = 1
    for i in range(3):
        plain, merged = qber_ref.host_counts(q, code, f, i), mref.host_counts(q, code, f, i)
        assert (merged[:D + 1] == plain).all() and not merged[D + 1:].any(), (combo, i)
    assert int(merged[:, 0].sum()) > 0 or combo in ("class", "all")


def test_non_chain_codes_are_refused(q):
    for name in ("toy45", "peg504"):
        code = qber_ref.make_code(q, name)
        with pytest.raises(q.QldpcError) as e:
            q.qber_counts_merged_host(code, np.zeros((code.N + 31) // 32, np.uint32))
        assert e.value.status == -7 and "chain" in str(e.value), name


def test_half_the_parity_punctured(q):
    """Code.ira_peg(16384, 8192), parity erased evenly spaced at exactly M / 2, q = 0.03, 8 frames of the syndrome form (parity VNs pinned to Alice's
    bits): the unmerged rule keeps at most one check and says nothing or the clamp; every merged estimate lies within 5 sigma + one grid step of its
    frame's empirical flip rate, sigma from the merged counts (qber_ref.sigma) -- the bound of test_sessions_estimate_blocks"""
    N, K, F, qtrue = 16384, 8192, 8, 0.03
    M = N - K
    code = q.Code.ira_peg(N, K)
    var, chk = code.edges()
    rng = np.random.default_rng(8192)
    cls = np.zeros(N, np.uint8); cls[K:] = 1
    erase = q.pack_bits(mref.spaced(N, M, M // 2))
    alice = rng.integers(0, 2, (F, N)).astype(np.uint8)
    synd = np.zeros((F, M), np.uint8)
    for v, c in zip(var, chk):
        synd[:, c] ^= alice[:, v]
    flips = (rng.random((F, N)) < qtrue).astype(np.uint8)
    flips[:, K:] = 0
    bob = alice ^ flips
    L1, L0, qs, _ = q.qber_table_host(q.QBER_MAX_DEGREE, 256)
    for i in range(F):
        args = (code, q.pack_bits(bob[i]), cls, K, q.pack_bits(synd[i]), erase)
        plain = np.zeros((q.QBER_MAX_DEGREE + 1, 2), np.uint64)
        plain[:code.max_cn_degree + 1] = q.qber_counts_host(*args)
        assert int(plain[:, 0].sum()) <= 1 and q.qber_argmax_host(plain, L1, L0) in (-1, 0)
        merged = q.qber_counts_merged_host(*args)
        k = q.qber_argmax_host(merged, L1, L0)
        emp = flips[i].sum() / K
        sig = qber_ref.sigma(merged.tolist(), emp)
        step = float(qs[min(k + 1, 255)] - qs[min(k + 1, 255) - 1])
        print("frame %d: merged q = %.5f, empirical %.5f, sigma %.5f, step %.5f, runs counted %d" % (i, qs[k], emp, sig, step, int(merged[:, 0].sum())))
        assert int(merged[:, 0].sum()) >= M // 2 - 1 and k >= 0
        assert abs(float(qs[k]) - emp) <= 5 * sig + step, i


def test_merged_host_code_under_asan_ubsan(tmp_path):
    """the merged mirror and the repeat table as a stand-alone program with exactly sized buffers"""
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    exe = str(tmp_path / "qber_merge_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "c", "qber_merge_sanitize.c"),
                           os.path.join(csrc, "qldpc_qber_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr

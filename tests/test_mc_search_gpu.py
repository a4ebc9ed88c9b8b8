"""Puncture patterns and the pattern search of the Monte-Carlo loop on the device (qldpc_mc_patterns_dev, qldpc_mc_search): the erase rows
against the host mirror word for word, and every counter row, goal and best of MonteCarlo.search against numpy pattern -> mc_frames_host ->
encoder -> LLRs with the pattern's VNs at 0 -> CPU oracle.  Exact equality everywhere."""
import os
import subprocess

import numpy as np
import pytest

import mc_ref
import mc_search_ref
from mc_oracle import KINDS, N_ITE, PATTERN_ROW as ROW, ROOT, SEED, SIM, counters, frames_reference, setups, sim_rows, stage_times, u32  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
F, N_PAT = 8, 24
# (n_punct, QBER) and the first of the 24 patterns per setup, chosen by the scan recorded in the docstring of test_search_equals_the_oracle_row_for_row
POINT = {"peg": (60, 0.17), "ira": (100, 0.013)}
FIRST = {"peg": 47, "ira": 16}
NONE = 2 ** 64 - 1


def search_reference(s, kind, qber, n_punct, first_pattern, n_pat=N_PAT, first_frame=0, cand=None):
    """rows [n_pat] of ROW, goal, best, best_frame_errors, best_bit_errors of patterns [first_pattern, first_pattern + n_pat), by numpy;
    computed once per argument set"""
    key = ("search", kind, qber, n_punct, first_pattern, n_pat, first_frame, None if cand is None else tuple(cand))
    if key in s._ref:
        return s._ref[key]
    cand = np.nonzero(s.cls == 1)[0] if cand is None else np.asarray(cand)
    vns = [cand[mc_search_ref.pattern(SEED, first_pattern + i, cand.size, n_punct)] for i in range(n_pat)]      # LLRs[pattern[i]] = 0 in its F frames
    f = frames_reference(s, kind, ("bsc", qber), first_frame + first_pattern * F, n_pat * F, vns, block=F)
    be, ok, it = (f[k].reshape(n_pat, F) for k in ("be", "ok", "it"))
    rows = np.zeros(n_pat, [(k, np.uint64) for k in ROW])
    rows["pattern"] = first_pattern + np.arange(n_pat)
    rows["frames"] = F
    rows["frame_errors"], rows["bit_errors"] = (be > 0).sum(1), be.sum(1)
    rows["undetected"], rows["not_converged"], rows["iter_sum"] = ((be > 0) & ok).sum(1), (~ok).sum(1), it.sum(1)
    out = dict(stats=rows, **summary(rows))
    s._ref[key] = out
    return out


def summary(rows):
    """goal and best of a set of rows by the definition: lowest index without frame errors; fewest frame errors, then bit errors, then index"""
    clean = rows["pattern"][rows["frame_errors"] == 0]
    b = np.lexsort((rows["pattern"], rows["bit_errors"], rows["frame_errors"]))[0]
    return dict(goal=int(clean.min()) if clean.size else NONE, best=int(rows["pattern"][b]), best_frame_errors=int(rows["frame_errors"][b]),
                best_bit_errors=int(rows["bit_errors"][b]))


def same(res, ref):
    assert res["stats"].dtype.names == ROW and res["stats"].shape == ref["stats"].shape
    for k in ROW:
        assert (res["stats"][k] == ref["stats"][k]).all(), (k, res["stats"][k], ref["stats"][k])
    for k in ("goal", "best", "best_frame_errors", "best_bit_errors"):
        assert int(res[k]) == ref[k], (k, res[k], ref[k])


@pytest.mark.parametrize("name", ["peg", "ira"])
def test_patterns_equal_the_host_mirror(q, setups, name):
    """default candidates (scattered among info VNs on the PEG code; N = 1008 and 2000 end in a full and in a partial word), a custom list of
    257, a single candidate; n_punct at both ends, next to them and inside; 32 and 3 key bits; across the carry of the pattern index; 1 and 70
    patterns per call"""
    s = setups(name)
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    rng = np.random.default_rng(5)
    lists = {"default": None, "257": np.sort(rng.choice(s.N, 257, replace=False)).astype(np.int32), "one": np.array([s.N - 1], np.int32)}
    for label, cand in lists.items():
        mc.set_candidates(cand)
        c = np.nonzero(s.cls == 1)[0] if cand is None else cand
        assert cand is not None or c.size == s.N - s.K
        for n_punct in sorted({0, 1, c.size // 3, c.size - 1, c.size}):
            for key_bits in (32, 3):
                for first, n in ((0, 70), (2 ** 32 - 3, 70), (0, 1), (2 ** 32 - 1, 1)):
                    if n == 70 and label != "default" and key_bits == 3 and first == 0:
                        continue
                    got = u32(mc.patterns(first, n, n_punct, key_bits))
                    ref = mc_search_ref.rows(SEED, first, n, c, n_punct, s.N, key_bits)
                    assert got.shape == ref.shape == (n, (s.N + 31) // 32) and (got == ref).all(), (label, n_punct, key_bits, first, n)
                    host = np.stack([mc_ref.pack(np.isin(np.arange(s.N), mc.pattern_vns(first + i, n_punct, key_bits))[None, :])[0] for i in (0, n - 1)])
                    assert (got[[0, n - 1]] == host).all()
                    assert mc_ref.popcount(got) == n * n_punct
    if name == "peg":      # scattered: the candidates share words with info VNs
        words = np.unique(np.nonzero(s.cls == 1)[0] // 32)
        assert np.isin(np.nonzero(s.cls == 0)[0] // 32, words).any()


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["peg", "ira"])
def test_search_equals_the_oracle_row_for_row(q, setups, name, kind):
    """24 patterns x 8 frames against numpy pattern -> mc_frames_host -> encoder -> LLRs with the pattern's VNs at 0 -> CPU oracle: every row, goal,
    best, best_frame_errors and best_bit_errors exactly equal.  The inputs must make the search mean something in the reference (asserted
    first): the first pattern has a frame error, between 3 and 18 of the 24 patterns have none, at least 3 distinct frame-error counts occur.
    (n_punct, QBER, first pattern) per setup were chosen by a scan with the oracle on the CPU over patterns 0 .. 71 of SEED (NMS 0.75, 20
    iterations, the real flips of mc_frames_host on the all-zero codeword; frame errors per pattern of 8 frames, the window of the test):
      PEGReg504x1008, 60 of the 504 parity VNs punctured, QBER 0.17, patterns 47 .. 70:
          flood  3 2 0 1 1 2 2 1 0 1 1 0 2 0 2 0 2 1 2 1 2 2 4 0    6 without errors
          hlay   2 1 0 0 0 0 1 0 0 0 0 0 2 0 0 0 0 1 0 1 1 0 2 0   16
          i8     3 2 0 1 2 2 3 1 0 1 1 0 2 1 2 0 2 2 2 2 2 2 4 0    5
      IRA(2000, 1590), 100 of the 410 parity VNs punctured, QBER 0.013, patterns 16 .. 39:
          flood  4 2 0 3 1 0 2 0 0 2 2 3 3 3 0 3 4 1 1 1 3 1 0 1    6
          hlay   4 2 0 2 0 0 2 0 0 1 1 2 2 3 0 2 4 0 0 0 2 1 0 0   11
          i8     4 2 0 3 1 1 2 0 0 2 2 3 3 3 0 3 4 1 1 1 3 1 0 1    5
    The three kinds share one point per setup, which is why the window does not start at pattern 0: from 0 the layered decoder has no frame
    error in pattern 0 at any point where the flooding ones leave 3 patterns clean.  The frames of the test carry the source's codewords
    instead of the all-zero one, so single counts may differ from this table; the conditions are asserted on the test's own reference."""
    s = setups(name)
    n_punct, qber = POINT[name]
    p0 = FIRST[name]
    ref = search_reference(s, kind, qber, n_punct, p0)
    fe = ref["stats"]["frame_errors"]
    print(name, kind, fe.tolist(), ref["goal"], ref["best"])
    assert fe[0] >= 1 and 3 <= int((fe == 0).sum()) <= 18 and np.unique(fe).size >= 3
    mc = q.MonteCarlo(s.decoder(kind), s.enc, seed=SEED)
    res = mc.search(qber, n_punct, F, first_pattern=p0, max_patterns=N_PAT, stop_at_goal=False)
    same(res, ref)
    assert res["patterns"] == N_PAT and res["frames"] == N_PAT * F and res["batches"] == 1 and res["next_pattern"] == p0 + N_PAT and res["decode_ms"] > 0
    stage_times(res, ("pattern", "expand", "generate", "load", "decode", "monitor"))
    assert int(res["stats"]["frames"].sum()) == N_PAT * F and ref["goal"] not in (p0, NONE)


@pytest.mark.parametrize("name,kind", [("peg", "flood"), ("ira", "hlay"), ("peg", "i8")])
def test_rows_do_not_depend_on_batch_or_split(q, setups, name, kind):
    s = setups(name)
    n_punct, qber = POINT[name]
    p0 = FIRST[name]
    ref = search_reference(s, kind, qber, n_punct, p0)
    goal = ref["goal"]
    dec = s.decoder(kind)
    for batch, per_round in ((192, 24), (64, 8), (80, 10)):
        mc = q.MonteCarlo(dec, s.enc, seed=SEED, batch=batch)
        res = mc.search(qber, n_punct, F, first_pattern=p0, max_patterns=N_PAT, stop_at_goal=False)
        same(res, ref)
        assert res["batches"] == -(-N_PAT // per_round) and res["patterns"] == N_PAT
        res = mc.search(qber, n_punct, F, first_pattern=p0, max_patterns=N_PAT, stop_at_goal=True)
        stop = min(N_PAT, ((goal - p0) // per_round + 1) * per_round)          # the end of the round that holds the goal
        assert res["patterns"] == stop and res["batches"] == -(-stop // per_round) and res["next_pattern"] == p0 + stop and res["goal"] == goal
        part = dict(stats=ref["stats"][:stop], **summary(ref["stats"][:stop]))
        same(res, part)
    # two calls split at pattern 7: the rows of the parts are the rows of the whole
    mc = q.MonteCarlo(dec, s.enc, seed=SEED, batch=80)
    a = mc.search(qber, n_punct, F, first_pattern=p0, max_patterns=7, stop_at_goal=False)
    b = mc.search(qber, n_punct, F, first_pattern=a["next_pattern"], max_patterns=N_PAT - 7, stop_at_goal=False)
    assert a["next_pattern"] == p0 + 7 and b["next_pattern"] == p0 + N_PAT and int(b["stats"]["pattern"][0]) == p0 + 7
    both = np.concatenate([a["stats"], b["stats"]])
    same(dict(stats=both, **summary(both)), ref)
    same(a, dict(stats=ref["stats"][:7], **summary(ref["stats"][:7])))
    same(b, dict(stats=ref["stats"][7:], **summary(ref["stats"][7:])))


@pytest.mark.parametrize("name,kind", [("peg", "flood"), ("ira", "i8")])
def test_fixed_puncture_set_in_run(q, setups, name, kind):
    s = setups(name)
    n_punct, qber = POINT[name]
    p0 = FIRST[name]
    ref = search_reference(s, kind, qber, n_punct, p0)
    fe = ref["stats"]["frame_errors"]
    mc = q.MonteCarlo(s.decoder(kind), s.enc, seed=SEED)
    res = mc.search(qber, n_punct, F, first_pattern=p0, max_patterns=N_PAT, stop_at_goal=False)
    for p in (p0 + int(np.nonzero(fe > 0)[0][0]), p0 + int(np.nonzero(fe == 0)[0][0])):
        vns = mc.pattern_vns(p, n_punct)
        assert (vns == np.nonzero(s.cls == 1)[0][mc_search_ref.pattern(SEED, p, s.N - s.K, n_punct)]).all()
        mc.set_puncture(vns)
        r = mc.run(qber, p * F, F)
        row = res["stats"][p - p0]
        assert int(row["pattern"]) == p
        for k in ROW[1:]:
            assert int(r[k]) == int(row[k]) == int(ref["stats"][p - p0][k]), (p, k)
    mc.set_puncture([])
    ctr, hist, failed = s.reference(kind, qber, 0, 192)
    assert counters(mc.run(qber, 0, 192)) == ctr and (mc.iter_hist() == hist).all() and (mc.failed_frames() == failed).all()


def test_qldpc_sim_device_search_prints_the_same_best(q, setups, tmp_path):
    s = setups("peg")
    alist = os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist")
    out = str(tmp_path / "pattern.txt")
    eff, qber = 1.3, 0.18
    n_punct = min(max(q.parity_bits_to_punct(s.N, s.K, q.min_code_rate(qber, eff)), 0), s.N - s.K)
    assert 0 < n_punct < s.N - s.K
    args = ["-a", alist, "-r", "NMS", "-p", "0.75", "-i", str(N_ITE), "-b", "192", "-s", "%g:%g:0.01" % (qber, qber), "-S", str(SEED), "-D",
            "-X", str(eff), "-F", str(F), "-f", "40", "-o", out]
    _, text = sim_rows(args)
    res = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED).search(qber, n_punct, F, max_patterns=40, stop_at_goal=True)
    lines = text.splitlines()
    assert "# ber %.4f: best of %d patterns: FE %d, BE %d per %d frames" % (qber, res["patterns"], res["best_frame_errors"], res["best_bit_errors"], F) in lines
    pats = [l for l in lines if l.startswith("#   pattern")]
    assert pats == ["#   pattern %3d: FE %d / %d, BE %d" % (int(r["pattern"]), int(r["frame_errors"]), F, int(r["bit_errors"])) for r in res["stats"]]
    written = [int(l) for l in open(out).read().splitlines() if not l.startswith("#")]
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    assert written == mc.pattern_vns(res["best"], n_punct).tolist()
    refused = subprocess.run([SIM] + args[:-2] + ["-E", "3"], capture_output=True, text=True, timeout=60)      # -E does not apply to the search
    assert refused.returncode != 0 and "-E" in refused.stderr
    refused = subprocess.run([SIM] + [a for a in args if a != "-D"], capture_output=True, text=True, timeout=60)
    assert refused.returncode != 0 and "-D" in refused.stderr


def test_refused_calls_leave_the_object_usable(q, setups):
    s = setups("peg")
    n_punct, qber = POINT["peg"]
    p0 = FIRST["peg"]
    ref = search_reference(s, "flood", qber, n_punct, p0)
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    n_cand = s.N - s.K

    def refused(status, call, *a, **kw):
        with pytest.raises(q.QldpcError) as e:
            call(*a, **kw)
        assert e.value.status == status, (call.__name__, a, kw)
        return str(e.value)

    for bad in (0.0, 0.5, -0.1, float("nan")):
        refused(-6, mc.search, bad, n_punct, F, max_patterns=N_PAT)
    for bad in (-1, n_cand + 1):
        refused(-6, mc.search, qber, bad, F, max_patterns=N_PAT)
        refused(-6, mc.patterns, 0, 4, bad)
        refused(-6, mc.pattern_vns, 0, bad)
    for bad in (0, -1, 193):
        refused(-6, mc.search, qber, n_punct, bad, max_patterns=N_PAT)
    for bad in (-1, 33):
        refused(-6, mc.search, qber, n_punct, F, max_patterns=N_PAT, key_bits=bad)
        assert "key_bits=%d" % bad in refused(-6, mc.patterns, 0, 4, n_punct, bad)      # the message names the offending value
    for bad in ([3, 3], [5, 4], [-1, 2], [0, s.N]):
        refused(-1, mc.set_candidates, bad)
        refused(-1, mc.set_puncture, bad)
    cfg = q.McSearchCfg()
    cfg.n_punct, cfg.frames_per_pattern, cfg.reserved[1] = n_punct, F, 1
    res = q.McSearchResult()
    assert q._L.qldpc_mc_search(mc._h, qber, cfg, 0, N_PAT, res) == -1
    same(mc.search(qber, n_punct, F, first_pattern=p0, max_patterns=N_PAT, stop_at_goal=False), ref)
    bytes_before = mc.device_bytes
    # candidates of one's own, then back to the default: the same rows again, and nothing more allocated
    mc.set_candidates(np.arange(0, s.N, 7))
    assert mc.search(qber, n_punct, F, max_patterns=3, stop_at_goal=False)["patterns"] == 3
    refused(-6, mc.search, qber, len(range(0, s.N, 7)) + 1, F, max_patterns=3)
    mc.set_candidates(None)
    same(mc.search(qber, n_punct, F, first_pattern=p0, max_patterns=N_PAT, stop_at_goal=False), ref)
    mc.patterns(0, 70, n_punct)
    mc.set_puncture([1, 2, 3])
    mc.set_puncture([])
    assert mc.device_bytes == bytes_before

"""The restatement of the variable-node update (tests/vn_rules_ref.py) against the CPU oracle, and the conditions on the inputs that make
tests/test_vn_rules_gpu.py sensitive.  No device.

  * the star formulas equal O.decode bit for bit on set A: flooding with 1 and 2 iterations, one horizontal-layered sweep, MS / OMS / NMS / AMS_MIN
  * flood() equals O.decode on the fan (MS / OMS / NMS, 1, 2, 3 and 5 iterations) and on the stars
  * sensitivity, a condition on the INPUTS: a decoder that sums a VN's slots in reverse, adds Y first, drops the last slot or folds the next
    VN's first slot in differs from the restatement on every star that can show it, and on every degree class of the fan
Run with -s for the share of posteriors each mutant changes (DESIGN.md section 4 records one run).
"""
import os
import re

import numpy as np
import pytest

import vn_rules_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
VN_CAPS = (4, 12)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def set_a(O):
    st = R.stars(list(R.SET_A), list(R.SET_A.values()))
    og = O.Graph.from_edges(st.N, st.M, st.var, st.chk)
    st.bind(og.export())
    return st, og


@pytest.fixture(scope="module")
def the_fan(O):
    N, M, var, chk, deg = R.fan()
    og = O.Graph.from_edges(N, M, var, chk)
    return N, M, var, chk, deg, og, og.export(), R.general_frames(N, seed=77)


def launch_constants():
    """(UN of a register-resident bucket of cap <= 4, UN of the others, QK_WAVES, the same pair for qk_vn_fpost) as the sources state them"""
    launch = open(os.path.join(CSRC, "qldpc_launch.hip")).read()
    m = re.search(r"constexpr int UN = \(CAP > 0 && CAP <= 4\) \? (\d+) : (\d+);", launch)
    w = re.search(r"#define QK_WAVES (\d+)", open(os.path.join(CSRC, "qldpc_kernels.h")).read())
    f = re.search(r"#define QK_FPV_UN\(D\) \(\(D\) <= 4 \? (\d+) : (\d+)\)", open(os.path.join(CSRC, "qldpc_kernels_fpost.h")).read())
    assert "grid_x(b.n, UNX)" in launch and "grid_x(c.n, QK_FPV_UN(c.deg))" in launch
    return int(m.group(1)), int(m.group(2)), int(w.group(1)), int(f.group(1)), int(f.group(2))


def test_the_lists_have_tails(set_a, the_fan):
    """no VN list of set A and no degree class of the fan fills its last wave or its last workgroup, so the tail path (entry i0 repeated) and a
    workgroup with idle waves run in every launch; the check lists (one check per wave) do not fill their last workgroup either"""
    un4, un, waves, fun4, fun = launch_constants()
    st, og = set_a
    dv = np.diff(og.export()["vn_ptr"])
    assert st.N < 3000
    lists = {4: int((dv <= 4).sum()), 12: int(((dv > 4) & (dv <= 12)).sum()), 0: int((dv > 12).sum())}
    print("set A: N = %d, M = %d, VN lists %r" % (st.N, st.M, lists))
    for cap, n in lists.items():
        assert n > 0 and R.tails(n, un4 if cap == 4 else un, waves), (cap, n)
    assert R.tails(st.M, 1, waves)
    assert {d for d in R.SET_A} >= {VN_CAPS[0], VN_CAPS[0] + 1, VN_CAPS[1], VN_CAPS[1] + 1, 64, 65}
    N, M, var, chk, deg, og, ex, y = the_fan
    classes = dict(zip(*[a.tolist() for a in np.unique(deg, return_counts=True)]))
    print("fan: N = %d, M = %d, classes %r, check degrees %r" % (N, M, classes, np.unique(np.diff(ex["cn_ptr"])).tolist()))
    assert set(range(0, 13)) <= set(classes) and {13, 16} <= set(classes)
    for d, n in classes.items():
        if d <= VN_CAPS[1]:
            assert R.tails(n, fun4 if d <= 4 else fun, waves), (d, n)
    assert R.tails(sum(n for d, n in classes.items() if d > VN_CAPS[1]), un, waves)
    assert any(n > fun * waves for d, n in classes.items() if 4 < d <= 12) and any(n > fun4 * waves for d, n in classes.items() if d <= 4)      # more than one workgroup


def test_the_edge_set_ends_at_the_engines_limit():
    """the edge engine stages QE_THREADS x max_dv floats in 64 KiB of LDS: its set reaches exactly that VN degree, and set A holds the first excess"""
    t = re.search(r"#define QE_THREADS (\d+)", open(os.path.join(CSRC, "qldpc_kernels_edge.h")).read())
    assert 64 * 1024 // (int(t.group(1)) * 4) == R.EDGE_MAX_DV == max(R.SET_EDGE)
    assert R.EDGE_MAX_DV + 1 in R.SET_A and list(R.SET_33) == [R.EDGE_MAX_DV + 1]
    assert "VN degree <= %d" % R.EDGE_MAX_DV in open(os.path.join(ROOT, "include", "qldpc.h")).read()


def test_the_fan_is_an_ira_code_for_the_posterior_form(q, the_fan):
    """is_ira, the chain table exists, every check degree <= 27 in more than one CN_CAPS bucket; a degree-0 information VN is accepted by
    from_edges, so the degree-0 body of qk_vn_fpost is reachable and the fan runs it"""
    N, M, var, chk, deg, og, ex, y = the_fan
    code = q.Code.from_edges(N, M, var, chk)
    assert code.is_ira and code.chain_table() is not None
    dc = np.diff(ex["cn_ptr"])
    assert dc.max() <= 27 and (dc <= 12).any() and (dc > 12).any()
    dv = np.diff(ex["vn_ptr"])
    assert (dv[:len(deg)] == deg).all() and (deg == 0).any()
    v2, c2 = code.edges()
    assert (v2 == og.edges()[0]).all() and (c2 == og.edges()[1]).all()      # the product and the oracle hold the same graph in the same edge order


@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_star_restatement_equals_the_oracle(O, set_a, rule, param):
    st, og = set_a
    y, _ = R.frames(st, R.LAYER_FAMILIES, seed=11, rule=rule, param=param)
    for n_ite in (1, 2):
        ref = O.decode(og, y, rule, param, n_ite, "flooding", False, 1)["post"]
        got = R.star_flooding(st, y, rule, param, n_ite)
        assert (bits(got) == bits(ref)).all(), (rule, "flooding", n_ite, int((bits(got) != bits(ref)).sum()))
        assert (bits(R.flood(og.export(), y, rule, param, n_ite)["post"]) == bits(ref)).all()
    ref = O.decode(og, y, rule, param, 1, "hlayered", False, 1)["post"]
    got = R.star_hlayered(st, y, rule, param)
    assert (bits(got) == bits(ref)).all(), (rule, "hlayered", int((bits(got) != bits(ref)).sum()))


@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_the_special_families_reach_their_zeros(set_a, rule, param):
    """*cancel* stars end on exactly +0.0 after one flooding iteration (and after one layered sweep where the partial sums are exact); the
    all -0.0 stars keep -0.0 under the layered sweep, where signbit and !(x >= 0) disagree"""
    st, og = set_a
    y, fam = R.frames(st, R.LAYER_FAMILIES, seed=11, rule=rule, param=param)
    cancel = fam == R.LAYER_FAMILIES.index("cancel")
    post = R.star_flooding(st, y, rule, param, 1)[:, st.centre]
    assert cancel.any(axis=0).all() and (bits(post[cancel]) == 0).all()
    layered = R.star_hlayered(st, y, rule, param)
    if rule != "OMS":
        assert (bits(layered[:, st.centre][cancel]) == 0).all()
    nz = R.all_negzero(fam, R.LAYER_FAMILIES)
    assert nz.any(axis=0).all() and (bits(layered[:, st.centre][nz]) == 0x80000000).all()
    assert (bits(R.star_flooding(st, y, rule, param, 1)[:, st.centre][nz]) == 0).all()      # flooding forms (Y + 0) - 0: +0.0


@pytest.mark.parametrize("rule,param", [r for r in R.MS_RULES if r[0] != "AMS_MIN"])
def test_flood_equals_the_oracle_on_the_fan(O, the_fan, rule, param):
    N, M, var, chk, deg, og, ex, y = the_fan
    for n_ite in (1, 2, 3, 5):
        ref = O.decode(og, y, rule, param, n_ite, "flooding", False, 1)
        got = R.flood(ex, y, rule, param, n_ite)
        assert (bits(got["post"]) == bits(ref["post"])).all(), (rule, n_ite)
        assert (got["hard"] == ref["hard"]).all() and (got["iters"] == ref["iters"]).all() and (got["synd_ok"] == ref["synd_ok"]).all()


def test_inputs_are_sensitive_on_the_stars(set_a):
    """Every mutant differs from the restatement, within the two flooding runs together, on every star that can show it: "rev" from degree 3
    on (two slots commute), "yfirst", "drop_last" and "pad" from degree 2 on"""
    st, og = set_a
    ex = og.export()
    y, _ = R.frames(st, R.FLOOD_FAMILIES, seed=11)
    want = [R.star_flooding(st, y, "MS", 0.0, n) for n in (1, 2)]
    for order in ("rev", "yfirst", "drop_last", "pad"):
        diff = np.zeros(y.shape, bool)
        for n, w in zip((1, 2), want):
            diff |= bits(R.flood(ex, y, "MS", 0.0, n, order)["post"]) != bits(w)
        per_star = np.zeros((len(y), len(st.deg)), bool)
        np.logical_or.at(per_star, (np.arange(len(y))[:, None], st.star_of_vn[None, :]), diff)
        share = {int(d): round(float(diff[:, st.centre[st.deg == d]].mean()), 3) for d in np.unique(st.deg)}
        print("stars %-9s share of centre posteriors changed, by degree: %r" % (order, share))
        need = st.deg >= (3 if order == "rev" else 2)
        assert per_star.any(axis=0)[need].all(), (order, st.deg[need & ~per_star.any(axis=0)])


@pytest.mark.parametrize("rule,param", [("MS", 0.0), ("NMS", 0.75)])
def test_inputs_are_sensitive_on_the_fan(O, the_fan, rule, param):
    """"rev" and "yfirst" differ from the oracle on at least one information VN of every degree >= 2 after two iterations"""
    N, M, var, chk, deg, og, ex, y = the_fan
    ref = bits(O.decode(og, y, rule, param, 2, "flooding", False, 1)["post"])
    for order in ("rev", "yfirst"):
        diff = bits(R.flood(ex, y, rule, param, 2, order)["post"]) != ref
        share = {int(d): round(float(diff[:, :len(deg)][:, deg == d].mean()), 3) for d in np.unique(deg)}
        print("fan %-3s %-6s share of (frame, VN) cells changed, by degree: %r" % (rule, order, share))
        for d in np.unique(deg):
            if d >= 2:
                assert diff[:, :len(deg)][:, deg == d].any(), (rule, order, int(d))

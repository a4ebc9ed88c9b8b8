"""Host suite (no GPU) of the vertical-layered schedule: the code's vlayer order, and the numpy reference the GPU tests compare
against (tests/vlayered_ref.py) pinned to the CPU oracle through its horizontal branch."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import vlayered_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# VN levels of the natural-order level schedule, level(v) = 1 + max level of any earlier VN sharing a check (what the definition gives)
GOLDEN_LEVELS = [("PEGReg504x1008.alist", 1008, 10), ("20.alist", 504, 21), ("1998.5.3.2665.alist", 1998, 233), ("test.qc", 16192, 34),
                 ("NR_1_0_2.qc", 136, 27), ("NR_1_7_30.qc", 2040, 27), ("NR_1_1_24_rm_half.qc", 1104, 27), ("NR_2_3_112.qc", 5824, 15),
                 ("NR_2_6_52_rm_half.qc", 1144, 15)]


def bsc_frames(rng, F, N, p, mag):
    return np.where(rng.random((F, N)) < p, -mag, mag).astype(np.float32)


def load(q, O, gold, name):
    p = os.path.join(gold, name)
    if name.endswith(".qc"):
        return q.Code.from_qc(p), O.Graph.from_qc(p)
    return q.Code.from_alist(p), O.Graph.from_alist(p)


def check_classes(code, order, ptr):
    """a permutation of 0..N-1 cut into classes whose VNs share no check; returns the class of every VN"""
    N = code.N
    assert order.shape == (N,) and (np.sort(order) == np.arange(N)).all()
    assert ptr[0] == 0 and ptr[-1] == N and (np.diff(ptr) > 0).all()
    cls = np.empty(N, np.int64)
    cls[order] = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    var, chk = code.edges()
    key = chk.astype(np.int64) * len(ptr) + cls[var]                      # (check, class) of every edge: no pair twice
    assert len(np.unique(key)) == len(key)
    return cls, var, chk


@pytest.mark.parametrize("name,N,levels", GOLDEN_LEVELS)
def test_vlayer_order_of_the_golden_matrices_is_the_natural_level_schedule(q, O, gold, name, N, levels):
    code, og = load(q, O, gold, name)
    assert code.N == N
    order, ptr, natural = code.vlayer_order()
    assert natural and code.n_vlayers == levels == len(ptr) - 1 == R.vn_levels(og.export())
    cls, var, chk = check_classes(code, order, ptr)
    # the sequential-order property: a VN's class is above that of every earlier VN it shares a check with, and inside a class the
    # VNs are in index order -- so the classes in order are operation for operation the v = 0..N-1 sweep
    idx = np.lexsort((var, chk))
    v, c = var[idx].astype(np.int64), chk[idx]
    same = c[1:] == c[:-1]
    assert (cls[v[1:]][same] > cls[v[:-1]][same]).all()
    for l in range(levels):
        assert (np.diff(order[ptr[l]:ptr[l + 1]]) > 0).all()


@pytest.mark.parametrize("ctor", ["ira", "ira_peg"])
def test_vlayer_order_of_an_ira_code_is_a_colouring(q, ctor):
    code = getattr(q.Code, ctor)(8192, 6554)
    order, ptr, natural = code.vlayer_order()
    assert not natural                                                      # parity VN k shares a check with VN k + 1: no level parallelism
    assert code.max_cn_degree <= code.n_vlayers < code.N // 16                      # the VNs of a check are a clique
    check_classes(code, order, ptr)
    assert code.n_layers == code.layer_order()[1].size - 1                  # the horizontal order is untouched by building the vertical one


def test_schedule_value_agrees_with_the_header(q):
    hdr = open(os.path.join(ROOT, "include", "qldpc.h")).read()
    assert int(re.search(r"QLDPC_SCHED_VLAYERED\s*=\s*(\d+)", hdr).group(1)) == q.SCHEDULES["vlayered"] == 3
    assert int(re.search(r"#define\s+QLDPC_RECON_SCHED_AUTO\s+(\d+)", hdr).group(1)) == 2
    assert q.SCHEDULES["flooding"] == 0 and q.SCHEDULES["hlayered"] == 1


@pytest.mark.parametrize("rule,param", [("MS", 0.0), ("OMS", 0.35), ("NMS", 0.75), ("AMS_MIN", 0.0)])
def test_reference_horizontal_branch_equals_the_oracle_bit_for_bit(O, gold, rule, param):
    og = O.Graph.from_alist(os.path.join(gold, "PEGReg504x1008.alist"))
    llr = bsc_frames(np.random.default_rng(3), 96, 1008, 0.065 if rule in ("NMS", "OMS") else 0.045, 2.6)
    mine = R.decode(og.export(), llr, rule, param, 25, "hlayered")
    ref = O.decode(og, llr, rule, param, 25, "hlayered", True, 1, n_threads=8)
    assert (mine["post"].view(np.uint32) == ref["post"].view(np.uint32)).all()
    assert (mine["iters"] == ref["iters"]).all() and (mine["hard"] == ref["hard"]).all() and (mine["synd_ok"] == ref["synd_ok"]).all()
    if rule in ("NMS", "OMS"):
        assert 0 < (ref["synd_ok"] == 0).sum() < 96                         # both outcomes occur


def test_reference_horizontal_branch_follows_the_oracle_in_depth_fixed_iterations_and_coset_mode(O, gold):
    og = O.Graph.from_alist(os.path.join(gold, "PEGReg504x1008.alist"))
    ex = og.export()
    rng = np.random.default_rng(4)
    llr = bsc_frames(rng, 40, 1008, 0.05, 2.9)
    x = rng.integers(0, 2, (40, 1008))
    tgt = np.stack([og.syndrome(xx)[1] for xx in x])
    coset = np.where(x == 1, -llr, llr).astype(np.float32)
    for kw, okw in [(dict(syndrome_depth=2), (True, 2)), (dict(enable_syndrome=False), (False, 1))]:
        mine = R.decode(ex, llr, "NMS", 0.75, 12, "hlayered", **kw)
        ref = O.decode(og, llr, "NMS", 0.75, 12, "hlayered", *okw, n_threads=8)
        assert (mine["post"].view(np.uint32) == ref["post"].view(np.uint32)).all() and (mine["iters"] == ref["iters"]).all() and (mine["synd_ok"] == ref["synd_ok"]).all()
    mine = R.decode(ex, coset, "NMS", 0.75, 12, "hlayered", target=tgt)
    ref = O.decode(og, coset, "NMS", 0.75, 12, "hlayered", True, 1, n_threads=8, target=tgt)
    assert (mine["post"].view(np.uint32) == ref["post"].view(np.uint32)).all() and (mine["iters"] == ref["iters"]).all() and (mine["synd_ok"] == ref["synd_ok"]).all()
    assert (ref["synd_ok"] == 1).mean() > 0.5


def test_reference_spa_follows_the_oracle_on_converging_frames(O, gold):
    og = O.Graph.from_alist(os.path.join(gold, "PEGReg504x1008.alist"))
    llr = bsc_frames(np.random.default_rng(7), 256, 1008, 0.07, 2.59)
    mine = R.decode(og.export(), llr, "SPA", 0.0, 20, "hlayered")
    ref = O.decode(og, llr, "SPA", 0.0, 20, "hlayered", True, 1, n_threads=8)
    conv = ref["synd_ok"] == 1
    assert conv.sum() > 128                                                 # numpy's tanh is not glibc's: posteriors differ in the last ulp
    assert (mine["hard"][conv] == ref["hard"][conv]).all() and (mine["iters"][conv] == ref["iters"][conv]).all()


def test_reference_vertical_branch_decodes_the_known_answer_frame(q, O, gold):
    kat = json.load(open(os.path.join(gold, "kat_peg504x1008.json")))
    code, og = load(q, O, gold, "PEGReg504x1008.alist")
    ex = og.export()
    llr = np.array(kat["llrs"], np.float32)[None, :]
    for rule, param in (("SPA", 0.0), ("NMS", 0.75)):
        r = R.decode(ex, llr, rule, param, 10, "vlayered")
        assert r["synd_ok"][0] == 1 and r["iters"][0] < 10 and (r["hard"][0][504:] == np.array(kat["decoded"])).all()


def test_reference_vertical_branch_is_invariant_inside_a_class(q, O, gold):
    """the sequential v = 0..N-1 sweep, the code's classes worked through at once, and the classes with their VNs shuffled: same floats"""
    code, og = load(q, O, gold, "PEGReg504x1008.alist")
    ex = og.export()
    order, ptr, _ = code.vlayer_order()
    llr = bsc_frames(np.random.default_rng(12), 48, 1008, 0.06, 2.6)
    seq = R.decode(ex, llr, "NMS", 0.75, 8, "vlayered")
    rng = np.random.default_rng(1)
    shuffled = np.concatenate([rng.permutation(order[ptr[l]:ptr[l + 1]]) for l in range(len(ptr) - 1)])
    for o, p in ((order, ptr), (shuffled, ptr), (shuffled, None)):
        r = R.decode(ex, llr, "NMS", 0.75, 8, "vlayered", order=o, class_ptr=p)
        assert (r["post"].view(np.uint32) == seq["post"].view(np.uint32)).all() and (r["iters"] == seq["iters"]).all()
    assert 0 < (seq["synd_ok"] == 1).sum()
    rev = R.decode(ex, llr, "NMS", 0.75, 8, "vlayered", order=np.arange(1007, -1, -1))
    assert (rev["post"].view(np.uint32) != seq["post"].view(np.uint32)).any()    # the order across classes does matter


def test_vlayer_graph_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "vlayer_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "c", "vlayer_sanitize.c"),
                           os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc", "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr


def test_vertical_schedule_is_validated_before_the_first_device_call(q, gold):
    """the refusals need no device (a valid request on a machine without one ends in "no HIP device"); the GPU suite repeats them"""
    code = q.Code.from_alist(os.path.join(gold, "PEGReg504x1008.alist"))
    for kw in (dict(engine="edges"), dict(msg_dtype="f16"), dict(msg_dtype="i8"), dict(layer_chain="on"), dict(compact="on")):
        with pytest.raises(q.QldpcError) as e:
            q.Decoder(code, 1008, 10, rule="NMS", rule_param=0.75, n_frames=8, schedule="vlayered", **kw)
        assert e.value.status == -7 and "vertical-layered" in str(e.value)
    with pytest.raises(q.QldpcError) as e:
        q.Recon(max_blocks=16, schedule="vlayered")
    assert e.value.status == -1
    if q.device_count() == 0:
        with pytest.raises(q.QldpcError) as e:
            q.Decoder(code, 1008, 10, rule="NMS", rule_param=0.75, n_frames=8, schedule="vlayered")
        assert e.value.status == -5

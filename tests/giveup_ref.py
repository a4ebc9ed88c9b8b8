"""Reference of the give-up rule of the early-exit run (qldpc_decoder_cfg.giveup_patience, csrc/qldpc_giveup_core.h), shared by
tests/test_giveup_host.py and tests/test_giveup_gpu.py.  Not a test module.

The trajectory of a batch: for k = 1 .. n_ite the CPU oracle decodes it with n_ite = k and no syndrome test; the weight of a frame at test k
is the weight of H . signbit(post_k) + s (8-bit messages: post_k < 0).  A plain Python restatement of the rule walks the weights of a frame
and says where it stops and why; `expected` turns that into what the decoder must return.  Trajectories are computed once per argument set
and left unchanged.
"""
import os

import numpy as np

CONVERGED, GAVE_UP, RAN_OUT = 0, 1, 2
N_ITE, QBER_, FRAMES = 30, 0.07, 576
SMALL, LARGE = 130, 576            # 3 groups, the last with 2 frames (round-robin placement) / 9 groups (one XCD per group)
MAG = np.float32(np.log((1 - QBER_) / QBER_))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIST = os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist")

_CACHE = {}


def flips():
    """the frames of these tests: 576 rows of BSC flips at q = 0.07"""
    if "flips" not in _CACHE:
        rng = np.random.default_rng(11)
        f = (rng.random((FRAMES, 1008)) < QBER_).astype(np.uint8)
        f.setflags(write=False)
        _CACHE["flips"] = f
    return _CACHE["flips"]


def llr_of(y):
    return np.where(np.asarray(y) == 1, -MAG, MAG).astype(np.float32)


def code(q):
    if "code" not in _CACHE:
        _CACHE["code"] = q.Code.from_alist(ALIST)
    return _CACHE["code"]


def graphs(q, O):
    """the code, the oracle's graph, the oracle's graph with the checks in the code's layer order (what the layered GPU sweep visits), that order"""
    if "graphs" not in _CACHE:
        og = O.Graph.from_alist(ALIST)
        order, _, _ = code(q).layer_order()
        var, chk = og.edges()
        inv = np.empty(og.M, np.int32)
        inv[order] = np.arange(og.M, dtype=np.int32)
        newc = inv[chk]
        idx = np.argsort(newc, kind="stable")
        _CACHE["graphs"] = (code(q), og, O.Graph.from_edges(og.N, og.M, var[idx], newc[idx]), order)
    return _CACHE["graphs"]


def weights_of(graph, x, target=None):
    """per frame the weight of H x + s"""
    out = np.empty(x.shape[0], np.int32)
    for f in range(x.shape[0]):
        w, s = graph.syndrome(x[f])
        out[f] = w if target is None else int((s != target[f]).sum())
    return out


def trajectory(q, O, kind, llr=None, target=None, graphs_of=None):
    """kind: "flood" / "flood_f16" / "flood_i8" / "hlay" / "hlay_i8" -> dict(post [n_ite][F][N], hard, weight [F][n_ite], ok [F][n_ite]) of the
    LLR rows llr (None: flips() on the all-zero codeword) with the target syndromes `target` (None: zero), NMS 0.75, 30 iterations.
    graphs_of: (oracle graph, the same in layer order, the layer order) of another set-up of the same code"""
    key = ("traj", kind, None if llr is None else llr.tobytes(), None if target is None else target.tobytes())
    if key in _CACHE:
        return _CACHE[key]
    og, ogl, order = graphs(q, O)[1:] if graphs_of is None else graphs_of
    layered = kind.startswith("hlay")
    graph = ogl if layered else og
    tgt = None if target is None else (np.ascontiguousarray(target[:, order]) if layered else target)
    llr = llr_of(flips()) if llr is None else llr
    extra = dict(msg_fp16=kind.endswith("f16"), msg_i8=kind.endswith("i8"))
    post, hard, weight, ok = [], [], [], []
    for k in range(1, N_ITE + 1):
        r = O.decode(graph, llr, "NMS", 0.75, k, "hlayered" if layered else "flooding", False, 1, n_threads=8, target=tgt, **extra)
        sign = (r["post"] < 0) if extra["msg_i8"] else np.signbit(r["post"])
        post.append(r["post"]); hard.append(r["hard"])
        weight.append(weights_of(graph, sign.astype(np.int32), tgt))
        ok.append((weights_of(graph, r["hard"], tgt) == 0).astype(np.int32))
    out = dict(post=np.stack(post), hard=np.stack(hard), weight=np.stack(weight, 1), ok=np.stack(ok, 1), layered=layered)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _CACHE[key] = out
    return out


def n_tests(layered, n_ite=N_ITE):
    """the tests a run makes: flooding after iterations 1 .. n_ite - 1, layered after every sweep"""
    return n_ite if layered else n_ite - 1


def walk(weights, patience, syndrome_depth=1):
    """the rule, restated: (stop test (1-based, 0: ran out), outcome, last weight, best weight) of one frame's weights at its tests"""
    best, since, depth = None, 0, 0
    for t, w in enumerate(weights, 1):
        w = int(w)
        if w == 0:
            depth = (depth + 1) % syndrome_depth
            converged = depth == 0
        else:
            depth, converged = 0, False
        if best is None or w < best:
            best, since = w, 0
        else:
            since += 1
        if converged:
            return t, CONVERGED, w, best
        if patience > 0 and w > 0 and since >= patience:
            return t, GAVE_UP, w, best
    return 0, RAN_OUT, int(weights[-1]), best


def expected(traj, patience, syndrome_depth=1, frames=None):
    """what a decoder with giveup = patience returns for the frames (None: all) of a trajectory: hard, iters, ok, gave, last, best, and the
    outcome per frame and the false give-ups (frames given up that converge with the rule off)"""
    sel = np.arange(traj["weight"].shape[0]) if frames is None else np.asarray(frames)
    T = n_tests(traj["layered"])
    out = dict(hard=[], iters=[], ok=[], gave=[], last=[], best=[], outcome=[], false=[])
    for f in sel:
        w = traj["weight"][f, :T]
        stop, what, last, best = walk(w, patience, syndrome_depth)
        k = stop if stop else N_ITE
        out["hard"].append(traj["hard"][k - 1, f]); out["iters"].append(k); out["ok"].append(traj["ok"][f, k - 1])
        out["gave"].append(int(what == GAVE_UP)); out["last"].append(last); out["best"].append(best); out["outcome"].append(what)
        out["false"].append(int(what == GAVE_UP and walk(w, 0, syndrome_depth)[1] == CONVERGED))
    return {k: np.asarray(v, np.int32) for k, v in out.items()}


def assert_mix(exp):
    """the input shows every outcome and a false give-up -- on the reference, before anybody looks at the device"""
    counts = np.bincount(exp["outcome"], minlength=3)
    assert (counts >= 1).all() and exp["false"].sum() >= 1, (counts, int(exp["false"].sum()))
    assert (exp["ok"][exp["gave"] == 1] == 0).all()
    return counts

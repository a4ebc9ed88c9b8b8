"""Decoder gangs (qldpc.h "decoder gangs", csrc/qldpc_kernels_gang.h) -- GPU parity (-m gpu).

A gang steps several horizontal-layered decoders in lockstep, one launch per colour step and kernel class for all of them.  The reference
is the existing path: every member run alone with qldpc_run on a second, identically configured decoder.  Hard decisions, iteration counts,
success flags and posteriors (as bit patterns) must be equal for every frame of every member; the min-sum members must also equal the CPU
oracle's horizontal-layered result bit for bit.

The four members are the smallest shapes that cross every seam: a ragged last group (70 frames), a decoder sized for more groups than
loaded (130 of 192), several buckets per layer (NR_1_7_30: caps 8 / 12 / 20), unequal layer counts, explicit messages (degree 36, cap 40;
SPA) and the compressed check state in one gang, and members that finish at different sweeps.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ITE = 20
#           name                    rule   param  frames loaded / sized  QBER
MEMBERS = [("PEGReg504x1008.alist", "NMS", 0.75, 70, 130, 0.08),
           ("NR_1_7_30.qc", "NMS", 0.75, 64, 64, 0.03),
           ("1998.5.3.2665.alist", "NMS", 0.75, 130, 192, 0.01),
           ("20.alist", "SPA", 0.0, 1, 1, 0.05)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def layer_graph(O, code, og):
    """the oracle's graph with the checks in the code's layer order (the order the GPU sweeps them in), and that order"""
    order, _, _ = code.layer_order()
    var, chk = og.edges()
    inv = np.empty(code.M, np.int32)
    inv[order] = np.arange(code.M, dtype=np.int32)
    newc = inv[chk]
    idx = np.argsort(newc, kind="stable")
    return O.Graph.from_edges(code.N, code.M, var[idx], newc[idx]), order


@pytest.fixture(scope="module")
def data(q, O, gold):
    """per member: code, the oracle's graph in layer order, the frames, and the oracle's results (min-sum members), computed once"""
    rng = np.random.default_rng(2024)
    out = []
    for name, rule, param, F, cap, p in MEMBERS:
        path = os.path.join(gold, name)
        code = q.Code.from_qc(path) if name.endswith(".qc") else q.Code.from_alist(path)
        og = O.Graph.from_qc(path) if name.endswith(".qc") else O.Graph.from_alist(path)
        ogl, order = layer_graph(O, code, og)
        y = (rng.random((F, code.N)) < p).astype(np.uint8)
        mag = np.float32(q.bsc_llr(p))
        llr = np.where(y == 1, -mag, mag).astype(np.float32)
        m = dict(name=name, rule=rule, param=param, F=F, cap=cap, p=p, code=code, og=og, ogl=ogl, order=order, y=y, mag=mag, llr=llr, ref={})
        if rule != "SPA":      # device exp / log differ from glibc's in the last ulp: SPA is compared with the solo run only
            m["ref"][True] = O.decode(ogl, llr, rule, param, N_ITE, "hlayered", True, 1, n_threads=4)
            m["ref"][False] = O.decode(ogl, llr, rule, param, 4, "hlayered", False, 1, n_threads=4)
        out.append(m)
    return out


def make(q, m, n_ite=N_ITE, synd=True, **kw):
    return q.Decoder(m["code"], m["code"].N, n_ite, rule=m["rule"], rule_param=m["param"], n_frames=m["cap"], schedule="hlayered", enable_syndrome=synd, **kw)


def load_llr(torch, dec, m):
    dec.load_llr(torch.from_numpy(m["llr"]).cuda())


def fetch(q, dec):
    hard = q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), dec.N)
    it, ok = dec.fetch_status()
    post = dec.fetch_post().cpu().numpy().view(np.uint32)
    return hard, it.cpu().numpy(), ok.cpu().numpy(), post


def same(a, b):
    return all(x.shape == y.shape and bool((x == y).all()) for x, y in zip(a, b))


def solo_and_gang(q, torch, data, n_ite=N_ITE, synd=True):
    """every member alone on one decoder (the reference), and all of them as a gang on a second set; returns both result lists and the gang"""
    solo = []
    for m in data:
        d = make(q, m, n_ite, synd)
        load_llr(torch, d, m)
        d.run()
        solo.append(fetch(q, d))
    decs = [make(q, m, n_ite, synd) for m in data]
    for d, m in zip(decs, data):
        load_llr(torch, d, m)
    gang = q.DecoderGang(decs)
    gang.run()
    return solo, [fetch(q, d) for d in decs], gang, decs


def check_all(data, solo, got, synd=True):
    for m, s, g in zip(data, solo, got):
        assert same(s, g), m["name"]
        if m["ref"]:
            ref = m["ref"][synd]
            assert (g[0] == ref["hard"]).all() and (g[1] == ref["iters"]).all() and (g[2] == ref["synd_ok"]).all(), m["name"]


def check_seams(solo):
    """the conditions the shapes were chosen for, on the solo results"""
    a, b, c, _ = solo
    assert 0 < (a[2] == 1).sum() < len(a[2]), a[2]      # A: converged and unconverged frames
    assert b[1].max() <= 3, b[1]                         # B: done early
    assert c[1].max() == N_ITE, c[1]                     # C: runs to the end


# ---- 1 - 3. bit-exact against the solo path ---------------------------------------------------------------------------------------------

def test_gang_equals_solo_runs_and_oracle(q, O, torch, data):
    solo, got, gang, _ = solo_and_gang(q, torch, data)
    st = gang.last_run_stats()
    print("gang stats", st, "iterations", [s[1].max() for s in solo])
    check_seams(solo)
    check_all(data, solo, got)
    assert st["launches"] < st["solo_launches"], st


def test_host_drops_members_with_poll_every_1(q, O, torch, data, monkeypatch):
    monkeypatch.setenv("QLDPC_POLL_EVERY", "1")
    solo, got, gang, _ = solo_and_gang(q, torch, data)
    st = gang.last_run_stats()
    print("gang stats", st)
    check_seams(solo)
    check_all(data, solo, got)
    assert st["dropped"] >= 1 and st["sweeps"] == N_ITE, st
    assert st["launches"] < st["solo_launches"], st


def test_fixed_sweeps(q, O, torch, data):
    solo, got, gang, _ = solo_and_gang(q, torch, data, n_ite=4, synd=False)
    check_all(data, solo, got, synd=False)
    assert gang.last_run_stats()["sweeps"] == 4


# ---- 4. launch count --------------------------------------------------------------------------------------------------------------------

def test_three_decoders_on_one_code_share_every_launch(q, torch, data):
    m = data[1]
    decs = []
    for F in (1, 64, 70):
        d = q.Decoder(m["code"], m["code"].N, 4, rule="NMS", rule_param=0.75, n_frames=F, schedule="hlayered", enable_syndrome=False)
        d.load_llr(torch.from_numpy(np.resize(m["llr"], (F, m["code"].N))).cuda())
        decs.append(d)
    gang = q.DecoderGang(decs)
    gang.run()
    st = gang.last_run_stats()
    assert st["sweeps"] == 4 and st["launches"] * 3 == st["solo_launches"], st
    plan = q.gang_plan([m["code"]] * 3, ["NMS"] * 3, [1] * 3)
    assert st["launches"] == 4 * plan["launches_per_sweep"], (st, plan)
    ref = make(q, dict(m, cap=70), 4, False)
    ref.load_llr(torch.from_numpy(np.resize(m["llr"], (70, m["code"].N))).cuda())
    ref.run()
    assert same(fetch(q, ref), fetch(q, decs[2]))


# ---- 5. forms of loading ----------------------------------------------------------------------------------------------------------------

def test_syndrome_form_class_pinning_erasures_and_take(q, O, torch, data):
    rng = np.random.default_rng(5)
    a, b = data[0], data[1]
    # A in syndrome form: Alice's word x, Bob's y = x ^ e, the target syndrome H x
    x = rng.integers(0, 2, (a["F"], a["code"].N)).astype(np.uint8)
    ya = x ^ a["y"]
    sa = np.stack([a["og"].syndrome(xx)[1] for xx in x]).astype(np.uint8)
    maga = np.full(a["F"], a["mag"], np.float32)
    # B through load_bits with a class vector that pins and punctures, plus per-frame erasures
    Nb = b["code"].N
    cls = np.zeros(Nb, np.uint8)
    cls[rng.choice(Nb, 200, replace=False)] = q.VN_PINNED
    cls[rng.choice(np.nonzero(cls == 0)[0], 40, replace=False)] = q.VN_PUNCTURED
    yb = b["y"].copy()
    yb[:, cls == q.VN_PINNED] = 0      # the all-zero codeword's disclosed bits
    erase = (rng.random((b["F"], Nb)) < 0.01).astype(np.uint8)
    magb = np.full(b["F"], b["mag"], np.float32)

    def load_a(d, y):
        d.load_bits(torch.from_numpy(i32(q.pack_bits(y))).cuda(), torch.from_numpy(maga).cuda())
        d.load_syndrome(torch.from_numpy(i32(q.pack_bits(sa))).cuda())

    def load_b(d):
        d.load_bits(torch.from_numpy(i32(q.pack_bits(yb))).cuda(), torch.from_numpy(magb).cuda(), torch.from_numpy(cls).cuda())
        d.load_erasures(torch.from_numpy(i32(q.pack_bits(erase))).cuda())

    def load(decs, y):
        load_a(decs[0], y)
        load_b(decs[1])
        load_llr(torch, decs[2], data[2])
        load_llr(torch, decs[3], data[3])

    solo = [make(q, m) for m in data]
    load(solo, ya)
    for d in solo:
        d.run()
    want = [fetch(q, d) for d in solo]
    ref = O.decode(a["ogl"], np.where(ya == 1, -a["mag"], a["mag"]).astype(np.float32), "NMS", 0.75, N_ITE, "hlayered", True, 1, n_threads=4, target=sa[:, a["order"]])
    assert (want[0][0] == ref["hard"]).all() and (want[0][1] == ref["iters"]).all() and (ref["hard"][ref["synd_ok"] == 1] == x[ref["synd_ok"] == 1]).all()
    assert (want[0][2] == 1).any()
    decs = [make(q, m) for m in data]
    load(decs, ya)
    gang = q.DecoderGang(decs)
    gang.run()
    got = [fetch(q, d) for d in decs]
    for m, s, g in zip(data, want, got):
        assert same(s, g), m["name"]
    # only A again, with other noise: the others keep their results
    ya2 = x ^ np.roll(a["y"], 1, axis=0)
    load_a(solo[0], ya2)
    solo[0].run()
    load_a(decs[0], ya2)
    gang.run(take=[1, 0, 0, 0])
    assert same(fetch(q, solo[0]), fetch(q, decs[0]))
    assert not same(fetch(q, decs[0]), got[0])
    for k in (1, 2, 3):
        assert same(fetch(q, decs[k]), got[k]), data[k]["name"]


# ---- 6. re-use --------------------------------------------------------------------------------------------------------------------------

def test_gang_solo_gang_and_a_decoder_in_two_gangs(q, O, torch, data):
    decs = [make(q, m) for m in data]
    for d, m in zip(decs, data):
        load_llr(torch, d, m)
    gang = q.DecoderGang(decs)
    gang.run()
    first = [fetch(q, d) for d in decs]
    decs[2].run()      # member C alone, in between
    alone = fetch(q, decs[2])
    gang.run()
    again = [fetch(q, d) for d in decs]
    assert same(first[2], alone) and all(same(x, y) for x, y in zip(first, again))
    ref = data[2]["ref"][True]
    assert (alone[0] == ref["hard"]).all() and (alone[1] == ref["iters"]).all()
    other = q.DecoderGang([decs[2], decs[0]])      # C and A are members of both gangs
    other.run()
    assert same(fetch(q, decs[2]), first[2]) and same(fetch(q, decs[0]), first[0])
    gang.run(take=[0, 1, 1, 0])
    assert all(same(x, fetch(q, d)) for x, d in zip(first, decs))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(q, torch, data):
    m = data[0]
    code, N = m["code"], m["code"].N
    good = make(q, m)

    def dec(**kw):
        kw.setdefault("schedule", "hlayered")
        kw.setdefault("rule", "NMS")
        kw.setdefault("rule_param", 0.75)
        return q.Decoder(code, N, N_ITE, n_frames=kw.pop("n_frames", 130), **kw)

    unsupported = [dec(schedule="flooding"), dec(schedule="vlayered"), dec(msg_dtype="i8"), dec(frames_per_lane=2), dec(compact="on"),
                   dec(layer_chain="on"), dec(schedule="flooding", engine="edges", n_frames=1)]
    for k, bad in enumerate(unsupported):
        with pytest.raises(q.QldpcError) as e:
            q.DecoderGang([good, bad])
        assert e.value.status == -7, k
        assert "member 1" in str(e.value), str(e.value)
    invalid = [[good, q.Decoder(code, N, N_ITE + 1, rule="NMS", rule_param=0.75, n_frames=130, schedule="hlayered")], [good, good],
               [good] + [make(q, dict(m, cap=1)) for _ in range(32)], []]
    for k, members in enumerate(invalid):
        with pytest.raises(q.QldpcError) as e:
            q.DecoderGang(members)
        assert e.value.status == -1, k
    # a taken member with nothing loaded: refused before anything runs -- the loaded member's state is what it was
    other = make(q, m)
    gang = q.DecoderGang([good, other])
    load_llr(torch, good, m)
    with pytest.raises(q.QldpcError) as e:
        gang.run()
    assert e.value.status == -8 and "member 1" in str(e.value)
    with pytest.raises(q.QldpcError) as e:
        good.fetch_packed()      # nothing has run on it
    assert e.value.status == -8
    gang.run(take=[1, 0])
    ref = m["ref"][True]
    got = fetch(q, good)
    assert (got[0] == ref["hard"]).all() and (got[1] == ref["iters"]).all() and (got[2] == ref["synd_ok"]).all()


# ---- 8. sessions ------------------------------------------------------------------------------------------------------------------------

def test_sessions_with_gangs_report_the_same(q, monkeypatch):
    """QLDPC_RECON_GANG=1: a Bob-side call whose blocks fall into several rate groups decodes them in rounds, one gang run per round.  Nothing
    a session reports may change, block for block.  192 blocks over the rate table with max_blocks = 48: several groups have several rounds."""
    rng = np.random.default_rng(3)      # by the sessions' plan: about 19 / 115 / 58 blocks at rates 0.5 / 0.7 / 0.8
    n, key_bits, max_blocks = 192, 20011, 48
    qb = rng.uniform(0.006, 0.058, n).astype(np.float32)
    alice = rng.integers(0, 2, (n, key_bits)).astype(np.uint8)
    bob = alice ^ (rng.random((n, key_bits)) < qb[:, None])
    aw, bw = q.pack_bits(alice), q.pack_bits(bob)
    results, prof = {}, {}
    for mode in ("unset", "1"):
        if mode == "unset":
            monkeypatch.delenv("QLDPC_RECON_GANG", raising=False)
        else:
            monkeypatch.setenv("QLDPC_RECON_GANG", mode)
        ra, rb = q.Recon(max_blocks=max_blocks), q.Recon(max_blocks=max_blocks)      # fresh sessions: the variable is read when the session is made
        rb.profile(True)
        msgs, pars = ra.encode_blocks([aw[i] for i in range(n)], [key_bits] * n, qb)
        st, fixed, co, it = rb.decode_blocks([bw[i] for i in range(n)], [key_bits] * n, qb, msgs, pars)
        prof[mode] = {s["name"]: s["launches"] for s in rb.profile_read()}
        print("QLDPC_RECON_GANG %s: %d of %d blocks ok, %d sweeps in all, profile %s" % (mode, int((np.asarray(st) == 0).sum()), n, int(np.asarray(it).sum()), prof[mode]))
        results[mode] = ([(m.rate_index, m.n_punct) for m in msgs], np.asarray(st).tolist(), [f.tobytes() for f in fixed], np.asarray(co).tolist(), np.asarray(it).tolist())
    groups = {}
    for r, _ in results["unset"][0]:
        groups[r] = groups.get(r, 0) + 1
    assert len(groups) >= 3 and max(groups.values()) > 2 * max_blocks, groups      # at least three rate groups, one of three or more rounds
    assert results["1"] == results["unset"]
    st = np.array(results["1"][1])
    assert (st == 0).mean() > 0.95 and all(results["1"][2][i] == aw[i].tobytes() for i in np.nonzero(st == 0)[0])      # every OK block's key is Alice's
    assert prof["unset"].get("layer_update_gang", 0) == 0 and prof["unset"]["layer_update"] > 0, prof
    assert prof["1"].get("layer_update_gang", 0) > 0, prof
    assert prof["1"].get("layer_update", 0) + prof["1"]["layer_update_gang"] < prof["unset"]["layer_update"], prof

"""GPU suite of the simplified SC decoder (Polar(rule="ssc"), qldpc_kernels_polar_ssc.h): the device against the SSC host mirror
(qldpc_polar_decode_ssc_host, which the CPU suite holds to the numpy restatement) bit for bit in u, info and x, each asked for alone and
together, in both message types; the refusals; the device bytes; the tally and the Monte-Carlo loop around an SSC context."""
import ctypes as C

import numpy as np
import pytest

import polar_mc_ref as M
import polar_ref as R
import polar_ssc_ref as S

pytestmark = pytest.mark.gpu

FMAX = 130
SEED = 20261


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _dev(torch, a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _same(out, host, what):
    for k, v in out.items():
        got = v.cpu().numpy().view(np.uint32)
        assert got.shape == host[k].shape and np.array_equal(got, host[k]), what + ": " + k


def _code(kind, n):
    rng = np.random.default_rng([SEED, n, len(kind)])
    N = 1 << n
    if kind == "random":
        return R.random_code(rng, N)[0]
    if kind == "clustered":
        return S.clustered_code(rng, n)[0]
    if kind == "5g":
        return R.nr_order(N)[N // 2:]
    return R.random_code(rng, N, 0 if kind == "none" else N)[0]


CASES = [("random", n) for n in range(1, 8)] + [("clustered", n) for n in (9, 11, 12)] + [("5g", 10), ("none", 7), ("all", 7)]


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("kind,n", CASES)
def test_device_is_the_ssc_mirror(q, torch, kind, n, messages):
    """70 and 130 frames on a context of 130 (a ragged group; a context larger than the call), the frozen row given and NULL, the three outputs
    together and each alone; the mirror decodes the 130 frames once per frozen row and is sliced"""
    rng = np.random.default_rng([n, messages == "i8", 31])
    N = 1 << n
    pos = _code(kind, n)
    llr = R.i8_inputs(rng, FMAX, N, 31) if messages == "i8" else R.f32_inputs(rng, FMAX, N)
    fz = R.pack(rng.integers(0, 2, (FMAX, N), dtype=np.uint8))
    dec = q.Polar(n, pos, messages, 31, max_frames=FMAX, rule="ssc")
    d_llr = _dev(torch, llr)
    for frozen in (fz, None):
        host = q.polar_decode_ssc_host(n, pos, llr, frozen, messages, 31)
        d_fz = _dev(torch, frozen)
        for F in (70, FMAX):
            fr = None if d_fz is None else d_fz[:F]
            out = dec.decode(d_llr[:F], fr)
            assert set(out) == {"u", "info", "x"}
            _same(out, {k: v[:F] for k, v in host.items()}, "%s n=%d F=%d %s" % (kind, n, F, messages))
            for name in ("u", "info", "x"):
                out = dec.decode(d_llr[:F], fr, want=(name,))
                assert set(out) == {name}
                _same(out, {name: host[name][:F]}, "%s n=%d F=%d %s alone" % (kind, n, F, messages))


def test_pw_half_rate_code_at_2_to_16(q, torch):
    """levels 6 .. 16 in the scratch, rate-0 and rate-1 nodes of up to 2^11 leaves: 70 frames, int8"""
    n, N, F = 16, 1 << 16, 70
    rng = np.random.default_rng(16)
    pos = np.sort(q.polar_pw_order(n)[N // 2:]).astype(np.int32)
    llr = rng.integers(-40, 40, (F, N)).astype(np.int8)
    fz = rng.integers(0, 1 << 32, (F, N // 32), dtype=np.uint64).astype(np.uint32)
    host = q.polar_decode_ssc_host(n, pos, llr, fz, "i8", 31)
    dec = q.Polar(n, pos, "i8", 31, max_frames=F, rule="ssc")
    _same(dec.decode(_dev(torch, llr), _dev(torch, fz)), host, "n=16")
    _same(dec.decode(_dev(torch, llr), _dev(torch, fz), want=("x",)), {"x": host["x"]}, "n=16 x alone")


def test_refusals(q, torch):
    EUNSUPPORTED = -7
    dec = q.Polar(7, [3, 5, 100], "i8", 31, max_frames=8, rule="ssc")
    llr = torch.zeros((4, 128), dtype=torch.int8, device="cuda")
    with pytest.raises(q.QldpcError) as e:
        dec.decode(llr, leaf=True)
    assert e.value.status == EUNSUPPORTED and "QLDPC_POLAR_SC" in str(e.value)
    assert set(dec.decode(llr)) == {"u", "info", "x"}              # the refusal left the context as it was
    with pytest.raises(q.QldpcError) as e:
        q.Polar(14, [3], "i8", 31, max_frames=2, form="wide", rule="ssc")
    assert e.value.status == EUNSUPPORTED and "LANES" in str(e.value)
    # at n = 5 a wide context decodes the lanes' way, and so does its SSC rule
    rng = np.random.default_rng(5)
    pos = R.random_code(rng, 32, 20)[0]
    rq = R.i8_inputs(rng, 70, 32, 31)
    out = q.Polar(5, pos, "i8", 31, max_frames=70, form="wide", rule="ssc").decode(_dev(torch, rq))
    _same(out, q.polar_decode_ssc_host(5, pos, rq, None, "i8", 31), "wide n=5")


@pytest.mark.parametrize("n", [4, 10])
def test_device_bytes(q, torch, n):
    """an SC context built through qldpc_polar_create_rule is qldpc_polar_create_form's to the byte; an SSC context also owns its plan"""
    N = 1 << n
    pos = np.ascontiguousarray(R.nr_order(N)[N // 2:], np.int32)
    make = lambda fn, *tail: _make(q, fn, n, pos, *tail)
    form = make(q._L.qldpc_polar_create_form, 0, 0)
    sc = make(q._L.qldpc_polar_create_rule, 0, 0, 0)
    ssc = make(q._L.qldpc_polar_create_rule, 0, 1, 0)
    assert sc == form and ssc == form + 12 * len(q.polar_ssc_plan(n, pos))
    assert q.Polar(n, pos, max_frames=130).device_bytes() == form
    assert q.Polar(n, pos, max_frames=130, rule="ssc").device_bytes() == ssc > form


def _make(q, fn, n, pos, *tail):
    h = C.c_void_p()
    assert fn(n, pos.size, pos.ctypes.data_as(C.POINTER(C.c_int)), 0, 31, 130, *tail, C.byref(h)) == 0
    size = int(q._L.qldpc_polar_device_bytes(h))
    q._L.qldpc_polar_free(h)
    return size


@pytest.mark.parametrize("n", [4, 8])
def test_tally_on_an_ssc_context_is_the_tally(q, torch, n):
    """every position is frozen in the tally, so the rule has no say"""
    rng = np.random.default_rng([n, 3])
    N, F = 1 << n, 70
    rq = rng.integers(-40, 40, (F, N)).astype(np.int8)
    tr = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    dec = q.Polar(n, R.random_code(rng, N, N // 2)[0], "i8", 31, max_frames=F, rule="ssc")
    got = dec.tally(_dev(torch, rq), _dev(torch, tr)).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, q.polar_tally_host(n, rq, tr, "i8", 31))


def _ssc_counters(q, n, pos, seed, first, F, table):
    """polar_mc_ref.counters with the SSC mirror in the decoder's place"""
    K = len(pos)
    fr = q.polar_mc_frames_host(n, pos, first, F, seed, table, "i8")
    info = q.polar_decode_ssc_host(n, pos, fr["llr"], None, "i8", 31)["info"]
    be = (R.unpack(info, K) != R.unpack(fr["info"], K)).sum(axis=1)
    return dict(frames=F, bit_errors=int(be.sum()), frame_errors=int((be > 0).sum()), undetected=int((be > 0).sum()), crc_fails=0,
                channel_flips=int(fr["flips"].astype(np.int64).sum()), channel_bits=F * (1 << n))


@pytest.mark.parametrize("batch", [2000, 700])
def test_monte_carlo_loop_around_an_ssc_context(q, torch, batch):
    """2 000 frames of the 2 dB table of the published curve: the loop's counters are mirror -> SSC mirror -> numpy verdict, counter for counter"""
    row, pos, tab, _ = M.sc_point(q, 2)
    F = 2000
    dec = q.Polar(10, pos, "i8", 31, max_frames=batch, rule="ssc")
    mc = q.PolarMonteCarlo(dec, seed=M.MC_SEED, batch=batch)
    mc.set_channel(*tab)
    got = mc.run(0, F)
    want = _ssc_counters(q, 10, pos, M.MC_SEED, 0, F, tab)
    print("Eb/N0 %.1f dB: %d frame errors of %d" % (row[0], got["frame_errors"], F))
    assert {k: got[k] for k in M.COUNTERS} == want and want["frame_errors"] > 0
    assert got["batches"] == -(-F // batch)

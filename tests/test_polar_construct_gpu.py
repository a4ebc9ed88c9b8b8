"""GPU suite of the genie-aided polar code construction (qldpc_polar_tally_dev, qcrypto-ldpc_amd/csrc/qldpc_kernels_polar_tally.h, and
qldpc_polar_mc_construct): Polar.tally against the host mirror count for count over the sizes, frame counts and message types, a second call
adding into the same rows, the context's own information set and device_bytes untouched; PolarMonteCarlo.construct against the mirror of its
frames through the mirror of the tally, over batch sizes, split ranges and two channels, with run() unchanged beside it; the refusals.  The
mirror itself is held to the numpy restatement by tests/test_polar_construct.py."""
import numpy as np
import pytest

import polar_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 5, 6, 7, 8, 11]
FRAME_COUNTS = (1, 5, 63, 64, 65, 130)
KINDS = [("i8", 1), ("i8", 31), ("f32", 0)]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _dev_words(torch, words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


@pytest.mark.parametrize("messages, maxq", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_tally_is_the_mirrors(q, torch, n, messages, maxq):
    """every frame count around a wave, on a context whose own code has K = N / 2; then every count again into ONE row, which adds them up"""
    rng = np.random.default_rng([n, maxq, 31])
    N, Fmax = 1 << n, max(FRAME_COUNTS)
    llr = R.i8_inputs(rng, Fmax, N, maxq) if messages == "i8" else R.f32_inputs(rng, Fmax, N)
    words = R.pack(rng.integers(0, 2, (Fmax, N), dtype=np.uint8))
    dec = q.Polar(n, q.polar_pw_order(n)[N // 2:], messages, maxq or 31, max_frames=Fmax)
    bytes_before = dec.device_bytes()
    d_llr, d_u = torch.from_numpy(llr).cuda(), _dev_words(torch, words)
    acc, total = torch.zeros((2, N), dtype=torch.int64, device="cuda"), np.zeros((2, N), np.uint64)
    for F in FRAME_COUNTS:
        want = q.polar_tally_host(n, llr[:F], words[:F], messages, maxq or 31)
        got = dec.tally(d_llr[:F], d_u[:F])
        assert got.dtype == torch.int64 and tuple(got.shape) == (2, N)
        assert np.array_equal(got.cpu().numpy().view(np.uint64), want), "n=%d %s maxq=%d F=%d" % (n, messages, maxq, F)
        assert dec.tally(d_llr[:F], d_u[:F], out=acc) is acc
        total += want
    assert np.array_equal(acc.cpu().numpy().view(np.uint64), total) and total[0].sum() > 0 and total[1].sum() > 0
    assert np.array_equal(dec.tally(d_llr[:0], d_u[:0], out=acc).cpu().numpy().view(np.uint64), total)          # no frames: a no-op
    assert dec.device_bytes() == bytes_before
    # the decoder beside it is what it was: its scratch is shared, its code is its own
    host = q.polar_decode_host(n, dec.info_pos, llr[:65], None, messages, maxq or 31)
    got = dec.decode(d_llr[:65])
    assert all(np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k]) for k in ("u", "info", "x"))


def _bsc(qber):
    t = int(np.floor(qber * 4294967296.0))
    mag = np.float32(np.log((1.0 - qber) / qber))
    return ([(1 << 32) - t], [t], [mag, -mag])


@pytest.mark.parametrize("channel", ["bsc", "awgn"])
def test_construct_is_the_mirrors_frames_through_the_mirrors_tally(q, torch, channel):
    """10 000 frames of N = 1 024 from above 2^32: in batches of 4 096 and of 100, as one call and as two ranges, on a BSC with float messages and
    on a 6-bit AWGN table with int8 messages; run() on the same object gives the counters it gave before"""
    n, N, F, seed, first = 10, 1024, 10000, 9, (1 << 32) - 3000
    messages, table = ("f32", _bsc(0.05)) if channel == "bsc" else ("i8", q.polar_mc_awgn_table(0.85, 4.0, 31, "floor"))
    pos = R.nr_order(N)[N // 2:]
    fr = q.polar_mc_frames_host(n, pos, first, F, seed, table, messages, frozen="random", want=("u", "llr"))
    split = 3333
    want_a = q.polar_tally_host(n, fr["llr"][:split], fr["u"][:split], messages, 31)
    want = q.polar_tally_host(n, fr["llr"][split:], fr["u"][split:], messages, 31, out=want_a.copy())
    assert want[0].max() > 0 and (channel == "awgn" or want[1].max() > 0)
    dec = q.Polar(n, pos, messages, 31, max_frames=4096)
    bytes_before = dec.device_bytes()
    for batch in (0, 100):
        mc = q.PolarMonteCarlo(dec, seed, batch, 64, "random")
        mc.set_channel(*table)
        before = mc.run(first, 600)
        got = mc.construct(first, F)
        assert got["frames"] == F and got["wrong"].dtype == np.uint64
        assert np.array_equal(got["wrong"], want[0]) and np.array_equal(got["ties"], want[1]), batch
        assert all(got[k] >= 0.0 for k in q.POLAR_MC_MS) and got["decode_ms"] > 0.0 and got["monitor_ms"] == 0.0 and got["total_ms"] > 0.0
        a, b = mc.construct(first, split), mc.construct(first + split, F - split)
        assert np.array_equal(a["wrong"], want_a[0]) and np.array_equal(a["ties"], want_a[1])
        assert np.array_equal(a["wrong"] + b["wrong"], want[0]) and np.array_equal(a["ties"] + b["ties"], want[1])
        assert not mc.construct(first, 0)["wrong"].any()
        after = mc.run(first, 600)
        assert {k: before[k] for k in q.POLAR_MC_COUNTERS} == {k: after[k] for k in q.POLAR_MC_COUNTERS} and before["frame_errors"] > 0
    assert dec.device_bytes() == bytes_before


def test_refusals_on_the_device(q, torch):
    ESIZE, EINVAL, EUNSUPPORTED, ESTATE = -6, -1, -7, -8
    n, N = 6, 64
    pos = R.nr_order(N)[32:]
    llr = torch.zeros((8, N), dtype=torch.int8, device="cuda")
    u = torch.zeros((8, 2), dtype=torch.int32, device="cuda")

    def status(call, *needles):
        with pytest.raises(q.QldpcError) as e:
            call()
        assert all(s in str(e.value) for s in needles), str(e.value)
        return e.value.status

    lanes, wide = q.Polar(n, pos, "i8", 31, max_frames=8), q.Polar(n, pos, "i8", 31, max_frames=8, form="wide")
    assert status(lambda: wide.tally(llr, u), "QLDPC_POLAR_LANES") == EUNSUPPORTED
    assert status(lambda: lanes.tally(llr, None)) == EINVAL
    big = torch.zeros((9, N), dtype=torch.int8, device="cuda")
    assert status(lambda: lanes.tally(big, torch.zeros((9, 2), dtype=torch.int32, device="cuda"))) == ESIZE
    assert q._L.qldpc_polar_tally_dev(lanes._h, 8, q._vp(llr.data_ptr()), q._vp(u.data_ptr()), None) == EINVAL
    assert q._L.qldpc_polar_tally_dev(lanes._h, -1, q._vp(llr.data_ptr()), q._vp(u.data_ptr()), None) == EINVAL
    table = q.polar_mc_awgn_table(0.9, 4.0, 31, "floor")

    def loop(dec, frozen="random", source="random", channel=True):
        mc = q.PolarMonteCarlo(dec, 1, 0, 16, frozen, source)
        if channel:
            mc.set_channel(*table)
        return mc

    assert status(lambda: loop(wide).construct(0, 8), "QLDPC_POLAR_LANES") == EUNSUPPORTED
    assert status(lambda: loop(q.PolarList(n, pos, "i8", 31, 2, max_frames=8)).construct(0, 8), "qldpc_polar context") == EUNSUPPORTED
    assert status(lambda: loop(lanes, frozen="zero").construct(0, 8), "QLDPC_POLAR_MC_FROZEN_RANDOM") == EUNSUPPORTED
    assert status(lambda: loop(lanes, source="zero").construct(0, 8), "qldpc_polar_mc_set_source") == ESTATE
    assert status(lambda: loop(lanes, channel=False).construct(0, 8), "qldpc_polar_mc_set_channel") == ESTATE
    mc = loop(lanes, source="zero")
    mc.set_source("random")
    got = mc.construct(0, 8)
    fr = q.polar_mc_frames_host(n, pos, 0, 8, 1, table, "i8", frozen="random", want=("u", "llr"))
    assert np.array_equal(np.stack([got["wrong"], got["ties"]]), q.polar_tally_host(n, fr["llr"], fr["u"], "i8", 31))
    assert q._L.qldpc_polar_mc_construct(mc._h, 0, 8, None, None) == EINVAL

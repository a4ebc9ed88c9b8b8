"""GPU suite of the Monte-Carlo loop around the polar decoders (qldpc_polar_mc_*, qcrypto-ldpc_amd/csrc/qldpc_polar_mc.hip): the device's frames
against the host mirror bit for bit in all five outputs; the counters and the failed list of run() against the restated counters of
tests/polar_mc_ref.py (the mirror's frames through the host decoders) around every decoder form, over batch sizes, split runs, the stop rule and a
short failed list; the reconciliation form; the published curves through run(); determinism.  The mirror itself is held to the numpy restatement
by tests/test_polar_mc.py."""
import numpy as np
import pytest

import polar_list_ref as LR
import polar_mc_ref as M
import polar_ref as R

pytestmark = pytest.mark.gpu

FRAME_COUNTS = (1, 63, 64, 65, 130)
ABOVE = (1 << 32) + 77


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_frames(dev, host, what):
    assert set(dev) == set(host)
    for k in host:
        d, h = dev[k], host[k]
        assert d.shape == h.shape, "%s: %s %s %s" % (what, k, d.shape, h.shape)
        assert np.array_equal(d.view(np.uint32), h.view(np.uint32)) if h.dtype.itemsize == 4 else np.array_equal(d, h), what + ": " + k


def _table(q, messages, sigma, rounding="round"):
    """the 6-bit AWGN table; the float messages get values that are no integers"""
    c0, c1, v = q.polar_mc_awgn_table(sigma, 4.0, 31, rounding)
    return (c0, c1, v if messages == "i8" else (v * np.float32(0.37)).astype(np.float32))


def _decoder(q, kind, n, pos, messages, max_frames):
    """kind -> (the context, its list size or None, its CRC)"""
    if kind in ("lanes", "wide"):
        return q.Polar(n, pos, messages, 31, max_frames=max_frames, form=kind), None, (0, 0)
    L = int(kind[4:])
    crc = LR.CRC11 if len(pos) >= 11 else (0, 0)
    return q.PolarList(n, pos, messages, 31, L, crc[0], crc[1], max_frames=max_frames), L, crc


# ---- frames ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 5, 6, 10])
def test_frames_are_the_mirrors(q, torch, n, messages):
    """info, u, x, llr and flips around an SC context (no CRC) and a list context (CRC 11 where the code holds one), both frozen modes, every frame
    count around a wave of the decoder, from frame 0 and from above 2^32, in one batch and in batches of 64; each output alone too"""
    rng = np.random.default_rng([n, messages == "i8", 8])
    N = 1 << n
    for kind in ("lanes", "list2"):
        pos, _ = R.random_code(rng, N, None if N > 32 else (N // 2 if kind == "lanes" else N))
        dec, _, crc = _decoder(q, kind, n, pos, messages, 130)
        tab = _table(q, messages, 0.9, "floor" if kind == "lanes" else "round")
        for frozen in ("zero", "random"):
            seed = int(rng.integers(0, 1 << 63))
            whole, small = q.PolarMonteCarlo(dec, seed, 0, 16, frozen), q.PolarMonteCarlo(dec, seed, 64, 16, frozen)
            whole.set_channel(*tab)
            small.set_channel(*tab)
            for first in (0, ABOVE):
                host = q.polar_mc_frames_host(n, pos, first, 130, seed, tab, messages, crc[0], crc[1], frozen)
                for F in FRAME_COUNTS:
                    what = "n=%d %s %s K=%d crc=%d %s first=%d F=%d" % (n, messages, kind, len(pos), crc[0], frozen, first, F)
                    _same_frames(_host(whole.frames(first, F)), {k: v[:F] for k, v in host.items()}, what)
                _same_frames(_host(small.frames(first, 130)), host, "n=%d %s %s %s first=%d in batches" % (n, messages, kind, frozen, first))
            for k in q.POLAR_MC_OUTPUTS:
                _same_frames(_host(small.frames(ABOVE, 70, want=(k,))), {k: host[k][:70]}, "n=%d %s %s alone" % (n, kind, k))
    zero = q.PolarMonteCarlo(dec, 1, 0, 16, "random", source="zero")
    zero.set_channel(*tab)
    _same_frames(_host(zero.frames(5, 65)), q.polar_mc_frames_host(n, pos, 5, 65, 1, tab, messages, crc[0], crc[1], "random", "zero"), "zero source")


def test_object_refusals_on_the_device(q, torch):
    ESIZE, EINVAL, ESTATE = -6, -1, -8
    dec = q.Polar(6, R.nr_order(64)[32:], "i8", 31, max_frames=100)
    with pytest.raises(q.QldpcError) as e:
        q.PolarMonteCarlo(dec, batch=101)
    assert e.value.status == ESIZE
    for kw in (dict(batch=-1), dict(fail_cap=-1), dict(frozen=2)):
        with pytest.raises(q.QldpcError) as e:
            q.PolarMonteCarlo(dec, **kw)
        assert e.value.status == EINVAL, kw
    mc = q.PolarMonteCarlo(dec)
    assert mc.batch == 100 and mc.device_bytes() > 100 * 64
    for call in (lambda: mc.run(0, 10), lambda: mc.frames(0, 10)):                       # no table yet
        with pytest.raises(q.QldpcError) as e:
            call()
        assert e.value.status == ESTATE
    good = q.polar_mc_awgn_table(0.9, 4.0, 31, "floor")
    mc.set_channel(*good)
    before = _host(mc.frames(0, 10))
    for bad, status in ((([1], [1], [0.5, 1.0]), EINVAL), (([2, 1], [1, 2], [1.0, 2.0, 3.0]), EINVAL), (([], [], [1.0]), ESIZE)):
        with pytest.raises(q.QldpcError) as e:
            mc.set_channel(*bad)
        assert e.value.status == status
    _same_frames(_host(mc.frames(0, 10)), before, "a refused table leaves the one in force")
    with pytest.raises(q.QldpcError) as e:
        mc.frames(0, -1)
    assert e.value.status == EINVAL
    assert mc.frames(0, 0)["llr"].shape == (0, 64) and mc.run(0, 0)["frames"] == 0 and mc.failed_frames().size == 0
    with pytest.raises(q.QldpcError) as e:
        mc.set_source(3)
    assert e.value.status == EINVAL


# ---- run -----------------------------------------------------------------------------------------------------------------------------------

SIGMA = {(6, "lanes"): 0.9, (6, "wide"): 0.9, (6, "list1"): 0.9, (6, "list4"): 1.0, (10, "lanes"): 0.85, (10, "wide"): 0.85, (10, "list1"): 0.85, (10, "list4"): 0.9}
RUN_FRAMES, RUN_FIRST, RUN_SEED = 300, (1 << 32) - 100, 77


def _counters(res):
    return {k: res[k] for k in M.COUNTERS}


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("kind", ["lanes", "wide", "list1", "list4"])
@pytest.mark.parametrize("n", [6, 10])
def test_run_counts_what_the_restatement_counts(q, torch, n, kind, messages):
    """300 frames across 2^32 at a noise level where 10 - 60 % fail (found with the mirror): every counter and the failed list, in batches of 64, of
    100 and in one; a run split at frame 130; the stop rule; a failed list shorter than the failures"""
    N, F, first = 1 << n, RUN_FRAMES, RUN_FIRST
    pos = R.nr_order(N)[N // 2:]
    dec, L, crc = _decoder(q, kind, n, pos, messages, F)
    tab = _table(q, messages, SIGMA[n, kind])
    ref = lambda a, count: M.counters(q, n, pos, RUN_SEED, a, count, tab, messages, 31, L, crc)
    want, failed = ref(first, F)
    print("n=%d %s %s: %s" % (n, kind, messages, want))
    assert 0.1 * F <= want["frame_errors"] <= 0.6 * F
    runs = {}
    for batch in (64, 100, 0):
        mc = q.PolarMonteCarlo(dec, RUN_SEED, batch, 1024)
        mc.set_channel(*tab)
        res = runs[batch] = mc.run(first, F)
        assert _counters(res) == want, batch
        assert res["batches"] == -(-F // mc.batch) and res["next_frame"] == first + F
        assert np.array_equal(mc.failed_frames(), failed), batch
        assert all(res[k] >= 0.0 for k in q.POLAR_MC_MS) and res["total_ms"] > 0.0
    # split at a frame that is no batch boundary: the counters add up, and each part's failed list is its own
    mc = q.PolarMonteCarlo(dec, RUN_SEED, 64, 1024)
    mc.set_channel(*tab)
    a, fa = mc.run(first, 130), mc.failed_frames()
    b, fb = mc.run(a["next_frame"], F - 130), mc.failed_frames()
    assert a["next_frame"] == first + 130 and M.add(_counters(a), _counters(b)) == want
    assert _counters(a) == ref(first, 130)[0] and np.array_equal(np.concatenate([fa, fb]), failed)
    # the stop rule: at the first batch boundary with 5 frame errors or more
    stop = next(64 * (k + 1) for k in range(5) if (failed < np.uint64(first + 64 * (k + 1))).sum() >= 5)
    res = mc.run(first, F, max_frame_errors=5)
    assert stop < F and res["frames"] == stop and res["batches"] == stop // 64 and _counters(res) == ref(first, stop)[0]
    assert np.array_equal(mc.failed_frames(), failed[failed < np.uint64(first + stop)])
    # a failed list of 7 entries: the first 7, and the counters do not care
    short = q.PolarMonteCarlo(dec, RUN_SEED, 100, 7)
    short.set_channel(*tab)
    assert _counters(short.run(first, F)) == want and np.array_equal(short.failed_frames(), failed[:7])
    none = q.PolarMonteCarlo(dec, RUN_SEED, 100, 0)
    none.set_channel(*tab)
    assert _counters(none.run(first, F)) == want and none.failed_frames().size == 0


@pytest.mark.parametrize("kind", ["lanes", "list4"])
@pytest.mark.parametrize("qber", [0.02, 0.06])
def test_reconciliation_form(q, torch, kind, qber):
    """random frozen values that the decoder is told, a BSC as the 2-level table: N = 1024, K = 512, 2 000 frames in batches of 700"""
    n, N, F = 10, 1024, 2000
    pos = R.nr_order(N)[N - 512:]
    dec, L, crc = _decoder(q, kind, n, pos, "f32", 700)
    mc = q.PolarMonteCarlo(dec, 11, 0, 4096, "random")
    mc.set_bsc(qber, np.log((1.0 - qber) / qber))
    want, failed = M.counters(q, n, pos, 11, 0, F, mc.table, "f32", 31, L, crc, "random")
    res = mc.run(0, F)
    print("%s at QBER %.2f: %s" % (kind, qber, want))
    assert _counters(res) == want and res["batches"] == 3 and np.array_equal(mc.failed_frames(), failed)
    assert abs(want["channel_flips"] / want["channel_bits"] - qber) < 4 * np.sqrt(qber * (1 - qber) / want["channel_bits"])
    if L:
        assert res["undetected"] == 0 and res["crc_fails"] == res["frame_errors"]


# ---- the published curves through run() ------------------------------------------------------------------------------------------------------

def _in_band(row, F, res):
    fer = res["frame_errors"] / F
    print("Eb/N0 %.2f dB: %d / %d = %.5f, published %.4f (%d / %d), band +-%.5f; %.2f ms: source %.2f, encode %.2f, channel %.2f, decode %.2f, monitor %.2f" % (
        row[0], res["frame_errors"], F, fer, row[1], row[3], row[5], R.fer_band(row, F), res["total_ms"], res["source_ms"], res["encode_ms"], res["channel_ms"],
        res["decode_ms"], res["monitor_ms"]))
    assert res["frames"] == F and abs(fer - row[1]) <= R.fer_band(row, F)


@pytest.mark.parametrize("k", range(5))
def test_published_sc_curve_through_run(q, torch, k):
    row, pos, tab, F = M.sc_point(q, k)
    mc = q.PolarMonteCarlo(q.Polar(10, pos, "i8", 31, max_frames=F), M.MC_SEED)
    mc.set_channel(*tab)
    res = mc.run(0, F)
    _in_band(row, F, res)
    assert res["crc_fails"] == 0 and res["undetected"] == res["frame_errors"]


@pytest.mark.parametrize("k", range(4))
def test_published_list_curve_through_run(q, torch, k):
    row, pos, tab, F = M.list_point(q, k)
    mc = q.PolarMonteCarlo(q.PolarList(10, pos, "i8", 31, 4, *LR.CRC11, max_frames=F), M.MC_SEED)
    mc.set_channel(*tab)
    res = mc.run(0, F)
    _in_band(row, F, res)
    assert res["undetected"] == 0 and res["crc_fails"] == res["frame_errors"]


def test_set_awgn_is_the_table_of_the_point(q, torch):
    """set_awgn(Eb/N0, rate) builds the table polar_mc_ref.list_point builds"""
    row, pos, tab, _ = M.list_point(q, 1)
    mc = q.PolarMonteCarlo(q.PolarList(10, pos, "i8", 31, 4, *LR.CRC11, max_frames=64), 3)
    sigma = mc.set_awgn(row[0], 500 / 1024, 4.0, 31, "round")
    assert abs(sigma - np.sqrt(1.0 / (2.0 * (500 / 1024) * 10.0 ** (row[0] / 10.0)))) < 1e-12
    assert all(np.array_equal(a, b) for a, b in zip(mc.table, tab))


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["lanes", "list4"])
def test_the_same_run_twice(q, torch, kind):
    n, N, F = 10, 1024, 1500
    pos = R.nr_order(N)[N // 2:]
    dec, _, _ = _decoder(q, kind, n, pos, "i8", 512)
    mc = q.PolarMonteCarlo(dec, 5, 0, 64)
    mc.set_channel(*_table(q, "i8", SIGMA[n, kind]))
    a, fa = mc.run(9, F), mc.failed_frames()
    b, fb = mc.run(9, F), mc.failed_frames()
    other = q.PolarMonteCarlo(dec, 5, 200, 64)
    other.set_channel(*_table(q, "i8", SIGMA[n, kind]))
    c, fc = other.run(9, F), other.failed_frames()
    assert _counters(a) == _counters(b) == _counters(c) and a["frame_errors"] > 64
    assert len(fa) == 64 and np.array_equal(fa, fb) and np.array_equal(fa, fc) and (np.diff(fa.astype(np.int64)) > 0).all()

"""GPU suite of the polar subsystem (qldpc_polar_*, qcrypto-ldpc_amd/csrc/qldpc_polar.hip): the device against the numpy restatement of
tests/polar_ref.py in all four outputs, bit for bit in both message types; closed forms at N = 2^20; the encoder against the host mirror; the
published SC curve with the host mirror's error counts; context reuse."""
import numpy as np
import pytest

import polar_ref as R

pytestmark = pytest.mark.gpu

FRAME_COUNTS = (1, 63, 64, 65, 130)
MAXQ = (1, 31, 126)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _dev(torch, a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _inputs(rng, messages, F, N, maxq):
    return R.i8_inputs(rng, F, N, maxq) if messages == "i8" else R.f32_inputs(rng, F, N)


def _ref_rows(ref, F):
    return tuple(a[:F] for a in ref)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", range(1, 13))
def test_device_is_the_restatement(q, torch, n, messages):
    """every frame count around a group of 64, with and without frozen values, all outputs together and each alone; the restatement of the 130
    frames is computed once per case and sliced"""
    rng = np.random.default_rng([n, messages == "i8", 4])
    N, Fmax, maxq = 1 << n, max(FRAME_COUNTS), MAXQ[n % 3]
    pos, mask = R.random_code(rng, N)
    llr = _inputs(rng, messages, Fmax, N, maxq)
    fv = rng.integers(0, 2, (Fmax, N), dtype=np.uint8)
    dec = q.Polar(n, pos, messages, maxq, max_frames=Fmax)
    d_llr = _dev(torch, llr)
    for values in (None, fv):
        ref = R.decode(llr, mask, values, messages, maxq)
        d_fv = _dev(torch, None if values is None else R.pack(values))
        for F in FRAME_COUNTS:
            out = _host(dec.decode(d_llr[:F], None if d_fv is None else d_fv[:F], leaf=True))
            assert set(out) == {"u", "info", "x", "leaf"}
            R.check_outputs(out, _ref_rows(ref, F), pos, N, mask, "n=%d F=%d %s" % (n, F, messages))
        F = 65
        for name in ("u", "info", "x"):
            out = _host(dec.decode(d_llr[:F], None if d_fv is None else d_fv[:F], want=(name,)))
            assert set(out) == {name}
            R.check_outputs(out, _ref_rows(ref, F), pos, N, mask, "n=%d alone %s" % (n, name))
        out = _host(dec.decode(d_llr[:F], None if d_fv is None else d_fv[:F], leaf=True, want=()))
        assert set(out) == {"leaf"}
        R.check_outputs(out, _ref_rows(ref, F), pos, N, mask, "n=%d alone leaf" % n)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("K", ["none", "all"])
def test_all_frozen_and_rate_one(q, torch, messages, K):
    rng = np.random.default_rng(11)
    n, N, F = 7, 128, 70
    pos, mask = R.random_code(rng, N, 0 if K == "none" else N)
    llr = _inputs(rng, messages, F, N, 31)
    fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
    out = _host(q.Polar(n, pos, messages, 31, max_frames=F).decode(_dev(torch, llr), _dev(torch, R.pack(fv)), leaf=True))
    R.check_outputs(out, R.decode(llr, mask, fv, messages, 31), pos, N, mask, K)


def _same(a, b, what):
    """two decodes' dicts bit for bit: words as uint32, floats by their bit patterns"""
    assert set(a) == set(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        bits = lambda v: v.view(np.uint32) if v.dtype.itemsize == 4 else v
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), what + ": " + k


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("K", [0, 33])
@pytest.mark.parametrize("n", [5, 7])
def test_small_shape_edges_are_the_mirror(q, torch, n, K, messages):
    """the edges of what the three decoders share (the info row, the level step, the context): 65 frames (two groups, one live lane in the
    second), no information bit, and 33 of them (an info row whose second word holds one bit; N = 32 has no 33 positions, so n = 5 takes all
    32: one full word).  Each output alone, then all together, against the host mirror.  n = 5: the frame is a leaf block read from the
    caller's row"""
    rng = np.random.default_rng([n, K, messages == "i8", 15])
    N, F = 1 << n, 65
    pos, _ = R.random_code(rng, N, min(K, N))
    llr = _inputs(rng, messages, F, N, 31)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    host = q.polar_decode_host(n, pos, llr, fz, messages, 31, leaf=True)
    dec = q.Polar(n, pos, messages, 31, max_frames=F)
    d_llr, d_fz = _dev(torch, llr), _dev(torch, fz)
    for name in ("u", "info", "x", "leaf"):
        out = _host(dec.decode(d_llr, d_fz, leaf=name == "leaf", want=() if name == "leaf" else (name,)))
        _same(out, {name: host[name]}, "n=%d K=%d %s alone" % (n, len(pos), messages))
    _same(_host(dec.decode(d_llr, d_fz, leaf=True)), host, "n=%d K=%d %s all" % (n, len(pos), messages))


@pytest.mark.parametrize("n,messages", [(14, "i8"), (14, "f32"), (16, "i8"), (16, "f32")])
def test_sizes_above_what_stays_on_chip(q, torch, n, messages):
    """levels 6 .. n live in the scratch; 65 frames: a full group and a group of one"""
    rng = np.random.default_rng([n, messages == "i8"])
    N, F, maxq = 1 << n, 65, 31
    pos, mask = R.random_code(rng, N)
    llr = _inputs(rng, messages, F, N, maxq)
    fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
    out = _host(q.Polar(n, pos, messages, maxq, max_frames=F).decode(_dev(torch, llr), _dev(torch, R.pack(fv)), leaf=True))
    R.check_outputs(out, R.decode(llr, mask, fv, messages, maxq), pos, N, mask, "n=%d" % n)


def test_closed_form_all_frozen_at_2_to_20(q, torch):
    """no information bit: u is the frozen row whatever was received, and x its encoding"""
    rng = np.random.default_rng(20)
    n, N, F = 20, 1 << 20, 2
    fv = rng.integers(0, 1 << 32, (F, N // 32), dtype=np.uint64).astype(np.uint32)
    llr = rng.integers(-128, 128, (F, N)).astype(np.int8)
    dec = q.Polar(n, [], "i8", 31, max_frames=F)
    out = _host(dec.decode(_dev(torch, llr), _dev(torch, fv)))
    assert np.array_equal(out["u"].view(np.uint32), fv)
    assert np.array_equal(out["x"].view(np.uint32), q.polar_encode_host(n, fv))
    assert out["info"].shape == (F, 0)


def test_closed_form_noiseless_at_2_to_20(q, torch):
    """no frozen bit and the noiseless LLRs of a random codeword: u re-encodes to that codeword, and the info row is u"""
    rng = np.random.default_rng(21)
    n, N, F = 20, 1 << 20, 2
    x = rng.integers(0, 1 << 32, (F, N // 32), dtype=np.uint64).astype(np.uint32)
    llr = ((1.0 - 2.0 * R.unpack(x, N)) * 7.5).astype(np.float32)
    dec = q.Polar(n, np.arange(N, dtype=np.int32), "f32", max_frames=F)
    out = _host(dec.decode(_dev(torch, llr)))
    assert np.array_equal(out["x"].view(np.uint32), x)
    assert np.array_equal(q.polar_encode_host(n, out["u"].view(np.uint32)), x)
    assert np.array_equal(out["info"], out["u"])


@pytest.mark.parametrize("n,F", [(1, 70), (4, 70), (5, 70), (6, 70), (10, 130), (16, 5), (18, 3)])
def test_encode_dev_is_the_mirror(q, torch, n, F):
    rng = np.random.default_rng(n)
    W = max(1, (1 << n) // 32)
    u = rng.integers(0, 1 << 32, (F, W), dtype=np.uint64).astype(np.uint32)      # below 2^5 with bits past N, which the encoder ignores
    want = q.polar_encode_host(n, u)
    enc = q.Polar(n, [0], "i8", 31, max_frames=F)
    d_u = _dev(torch, u)
    x = enc.encode(d_u)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), want) and np.array_equal(d_u.cpu().numpy().view(np.uint32), u)
    assert enc.encode(d_u, out=d_u) is d_u
    assert np.array_equal(d_u.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize("k", range(5))
def test_published_sc_curve_on_the_device(q, torch, k):
    """the frames of the CPU suite: the device counts the host mirror's block errors exactly, so every point lies in the band around the published
    FER (at 3 dB: 52 / 20 000)"""
    row, pos, msg, rq = R.fer_point(k)
    F = len(msg)
    dec = q.Polar(10, pos, "i8", 31, max_frames=F)
    dev = dec.decode(_dev(torch, rq), want=("info",))["info"].cpu().numpy().view(np.uint32)
    host = q.polar_decode_host(10, pos, rq, None, "i8", 31)["info"]
    e_dev, e_host = int((R.info_bits(dev, len(pos)) != msg).any(axis=1).sum()), int((R.info_bits(host, len(pos)) != msg).any(axis=1).sum())
    print("Eb/N0 %.1f dB: device %d, mirror %d of %d; published %d / %d" % (row[0], e_dev, e_host, F, row[3], row[5]))
    assert np.array_equal(dev, host) and e_dev == e_host
    assert abs(e_dev / F - row[1]) <= R.fer_band(row, F)


def test_reconciliation_form_on_the_device(q, torch):
    pos, x, frozen, llr = R.recon_frames(2)
    out = _host(q.Polar(10, pos, "f32", max_frames=len(x)).decode(_dev(torch, llr), _dev(torch, frozen)))
    host = q.polar_decode_host(10, pos, llr, frozen, "f32")
    assert all(np.array_equal(out[k].view(np.uint32), host[k]) for k in ("u", "info", "x"))
    assert int((out["x"].view(np.uint32) == R.pack(x)).all(axis=1).sum()) >= 1995


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_context_reuse(q, torch, messages):
    """a second call with fewer frames leaves no trace of the first, and the context does not grow"""
    rng = np.random.default_rng(9)
    n, N = 8, 256
    pos, mask = R.random_code(rng, N, 100)
    dec = q.Polar(n, pos, messages, 31, max_frames=130)
    size = dec.device_bytes()
    assert size > 0
    a, b = _inputs(rng, messages, 130, N, 31), _inputs(rng, messages, 5, N, 31)
    fv = rng.integers(0, 2, (130, N), dtype=np.uint8)
    first = _host(dec.decode(_dev(torch, a), _dev(torch, R.pack(fv)), leaf=True))
    second = _host(dec.decode(_dev(torch, b), leaf=True))
    R.check_outputs(first, R.decode(a, mask, fv, messages, 31), pos, N, mask, "first")
    R.check_outputs(second, R.decode(b, mask, None, messages, 31), pos, N, mask, "second")
    assert dec.device_bytes() == size


def test_frame_count_above_the_context(q, torch):
    dec = q.Polar(6, [5], "i8", 31, max_frames=64)
    with pytest.raises(q.QldpcError) as e:
        dec.decode(torch.zeros((65, 64), dtype=torch.int8, device="cuda"))
    assert e.value.status == -6
    assert dec.decode(torch.zeros((0, 64), dtype=torch.int8, device="cuda"))["u"].shape == (0, 2)

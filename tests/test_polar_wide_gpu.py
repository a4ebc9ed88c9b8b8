"""GPU suite of the wide form of the polar SC decoder (Polar(form="wide"), qcrypto-ldpc_amd/csrc/qldpc_kernels_polar_wide.h): the device against
the numpy restatement of tests/polar_ref.py in all four outputs, bit for bit in both message types, at every size around the chip level C; the
edge codes; the lanes form and the host mirror at 2^16 and 2^18; closed forms at N = 2^20; context reuse; the reconciliation form; the memory a
context owns."""
import os
import re

import numpy as np
import pytest

import polar_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHIP = int(re.search(r"#define\s+PLW_CHIP_LOG\s+(\d+)", open(os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc", "qldpc_polar_wide_core.h")).read()).group(1))
FRAME_COUNTS = (1, 2, 3, 5)
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


def _same(a, b, what):
    """two decodes' dicts bit for bit: device tensors as numpy, words as uint32, floats by their bit patterns"""
    assert set(a) == set(b), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, what + ": " + k
        bits = lambda v: v.view(np.uint32) if v.dtype.itemsize == 4 else v
        assert np.array_equal(bits(x), bits(y)), what + ": " + k


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", range(1, max(14, CHIP + 2) + 1))
def test_device_is_the_restatement(q, torch, n, messages):
    """one 5-frame input (the five kinds of float frames; an all-minimum and an all-zero int8 frame), frame counts 1, 2, 3 and 5, with and
    without frozen values (from n = 13 with them only), all outputs together and at 3 frames each alone"""
    rng = np.random.default_rng([n, messages == "i8", 6])
    N, Fmax, maxq = 1 << n, max(FRAME_COUNTS), MAXQ[n % 3]
    pos, mask = R.random_code(rng, N)
    llr = _inputs(rng, messages, Fmax, N, maxq)
    fv = rng.integers(0, 2, (Fmax, N), dtype=np.uint8)
    dec = q.Polar(n, pos, messages, maxq, max_frames=Fmax, form="wide")
    d_llr = _dev(torch, llr)
    for values in ((None, fv) if n < 13 else (fv,)):
        ref = R.decode(llr, mask, values, messages, maxq)
        d_fv = _dev(torch, None if values is None else R.pack(values))
        for F in FRAME_COUNTS:
            out = _host(dec.decode(d_llr[:F], None if d_fv is None else d_fv[:F], leaf=True))
            assert set(out) == {"u", "info", "x", "leaf"}
            R.check_outputs(out, _ref_rows(ref, F), pos, N, mask, "n=%d F=%d %s" % (n, F, messages))
        F = 3
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
    rng = np.random.default_rng(12)
    n, F = CHIP + 1, 3
    N = 1 << n
    pos, mask = R.random_code(rng, N, 0 if K == "none" else N)
    llr = _inputs(rng, messages, F, N, 31)
    fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
    out = _host(q.Polar(n, pos, messages, 31, max_frames=F, form="wide").decode(_dev(torch, llr), _dev(torch, R.pack(fv)), leaf=True))
    R.check_outputs(out, R.decode(llr, mask, fv, messages, 31), pos, N, mask, K)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("K", [0, 33])
@pytest.mark.parametrize("n", [6, 11, 12])
def test_small_shape_edges_are_the_mirror(q, torch, n, K, messages):
    """the edges of what the three decoders share (the info row, level 5 of a leaf block, the context): 65 frames, no information bit, and 33
    of them (an info row whose second word holds one bit).  Each output alone, then all together, against the host mirror.  n = 6: level 6 is
    the caller's row; n = 11: exactly one window; n = 12: two windows and the first combine on the row"""
    rng = np.random.default_rng([n, K, messages == "i8", 16])
    N, F = 1 << n, 65
    pos, _ = R.random_code(rng, N, K)
    llr = _inputs(rng, messages, F, N, 31)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    host = q.polar_decode_host(n, pos, llr, fz, messages, 31, leaf=True)
    dec = q.Polar(n, pos, messages, 31, max_frames=F, form="wide")
    d_llr, d_fz = _dev(torch, llr), _dev(torch, fz)
    for name in ("u", "info", "x", "leaf"):
        out = _host(dec.decode(d_llr, d_fz, leaf=name == "leaf", want=() if name == "leaf" else (name,)))
        _same(out, {name: host[name]}, "n=%d K=%d %s alone" % (n, K, messages))
    _same(_host(dec.decode(d_llr, d_fz, leaf=True)), host, "n=%d K=%d %s all" % (n, K, messages))


@pytest.mark.parametrize("n,messages", [(16, "i8"), (16, "f32"), (18, "i8"), (18, "f32")])
def test_wide_is_the_lanes_form_and_the_mirror(q, torch, n, messages):
    rng = np.random.default_rng([n, messages == "i8", 8])
    N, F, maxq = 1 << n, 2, 31
    pos, _ = R.random_code(rng, N)
    llr = _inputs(rng, messages, F, N, maxq)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    d_llr, d_fz = _dev(torch, llr), _dev(torch, fz)
    wide = _host(q.Polar(n, pos, messages, maxq, max_frames=F, form="wide").decode(d_llr, d_fz, leaf=True))
    lanes = _host(q.Polar(n, pos, messages, maxq, max_frames=F, form="lanes").decode(d_llr, d_fz, leaf=True))
    assert set(wide) == {"u", "info", "x", "leaf"}
    _same(wide, lanes, "n=%d %s: wide, lanes" % (n, messages))
    _same(wide, q.polar_decode_host(n, pos, llr, fz, messages, maxq, leaf=True), "n=%d %s: wide, mirror" % (n, messages))


def test_closed_form_all_frozen_at_2_to_20(q, torch):
    """no information bit: u is the frozen row whatever was received, and x its encoding"""
    rng = np.random.default_rng(22)
    n, N = 20, 1 << 20
    fv = rng.integers(0, 1 << 32, (1, N // 32), dtype=np.uint64).astype(np.uint32)
    llr = rng.integers(-128, 128, (1, N)).astype(np.int8)
    out = _host(q.Polar(n, [], "i8", 31, max_frames=1, form="wide").decode(_dev(torch, llr), _dev(torch, fv)))
    assert np.array_equal(out["u"].view(np.uint32), fv)
    assert np.array_equal(out["x"].view(np.uint32), q.polar_encode_host(n, fv))
    assert out["info"].shape == (1, 0)


def test_closed_form_noiseless_at_2_to_20(q, torch):
    """no frozen bit and the noiseless LLRs of a random codeword: x is the sent word"""
    rng = np.random.default_rng(23)
    n, N = 20, 1 << 20
    x = rng.integers(0, 1 << 32, (1, N // 32), dtype=np.uint64).astype(np.uint32)
    llr = ((1.0 - 2.0 * R.unpack(x, N)) * 7.5).astype(np.float32)
    out = _host(q.Polar(n, np.arange(N, dtype=np.int32), "f32", max_frames=1, form="wide").decode(_dev(torch, llr)))
    assert np.array_equal(out["x"].view(np.uint32), x)
    assert np.array_equal(q.polar_encode_host(n, out["u"].view(np.uint32)), x)
    assert np.array_equal(out["info"], out["u"])


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_context_reuse(q, torch, messages):
    """5 frames, 1 other frame, the 5 again on one context: the first and the third result are identical, the second is its own frame's, and the
    context does not grow; a frame too many is refused and no frame is no work"""
    rng = np.random.default_rng(10)
    n = CHIP + 1
    N = 1 << n
    pos, mask = R.random_code(rng, N, N // 3)
    dec = q.Polar(n, pos, messages, 31, max_frames=5, form="wide")
    size = dec.device_bytes()
    assert size > 0
    a, b = _inputs(rng, messages, 5, N, 31), _inputs(rng, messages, 3, N, 31)[2:]
    fz = R.pack(rng.integers(0, 2, (5, N), dtype=np.uint8))
    d_a, d_b, d_fz = _dev(torch, a), _dev(torch, b), _dev(torch, fz)
    first = _host(dec.decode(d_a, d_fz, leaf=True))
    second = _host(dec.decode(d_b, leaf=True))
    third = _host(dec.decode(d_a, d_fz, leaf=True))
    _same(first, third, "first, third")
    _same(first, q.polar_decode_host(n, pos, a, fz, messages, 31, leaf=True), "first, mirror")
    _same(second, q.polar_decode_host(n, pos, b, None, messages, 31, leaf=True), "second, mirror")
    assert dec.device_bytes() == size
    with pytest.raises(q.QldpcError) as e:
        dec.decode(torch.zeros((6, N), dtype=d_a.dtype, device="cuda"))
    assert e.value.status == -6
    none = dec.decode(torch.zeros((0, N), dtype=d_a.dtype, device="cuda"), leaf=True)
    assert none["u"].shape == (0, N // 32) and none["leaf"].shape == (0, N)
    _same(_host(dec.decode(d_a, d_fz, leaf=True)), first, "after the refusals")


def test_reconciliation_form(q, torch):
    """2 000 frames of N = 1 024: every output of every frame is the lanes form's, and so is the count of reconciled keys"""
    pos, x, frozen, llr = R.recon_frames(2)
    F = len(x)
    assert F == 2000
    d_llr, d_fz = _dev(torch, llr), _dev(torch, frozen)
    wide = _host(q.Polar(10, pos, "f32", max_frames=F, form="wide").decode(d_llr, d_fz))
    lanes = _host(q.Polar(10, pos, "f32", max_frames=F, form="lanes").decode(d_llr, d_fz))
    _same(wide, lanes, "wide, lanes")
    assert int((wide["x"].view(np.uint32) == lanes["x"].view(np.uint32)).all(axis=1).sum()) == 2000
    assert int((wide["x"].view(np.uint32) == R.pack(x)).all(axis=1).sum()) >= 1995


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_a_wide_context_is_small(q, torch, messages):
    """one frame of 2^16: below 1/16 of the lanes context, which holds 64 frames' worth whatever it is asked for (the layouts give about 1/100)"""
    pos = np.arange(1 << 15, dtype=np.int32)
    wide, lanes = (q.Polar(16, pos, messages, 31, max_frames=1, form=form).device_bytes() for form in ("wide", "lanes"))
    print("device bytes at n = 16, one frame, %s: wide %d, lanes %d, 1/%.0f" % (messages, wide, lanes, lanes / wide))
    assert 0 < wide < lanes / 16


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("chip,lanes,leaf", [(12, 256, 1), (6, 64, 32), (8, 512, 1), (13, 1024, 32)])
def test_the_measured_alternatives_are_the_same_decoder(q, torch, monkeypatch, chip, lanes, leaf, messages):
    """what tools/polar_wide_cost.py times beside the defaults -- another chip level, another workgroup, the leaf block on one lane -- at n = 15,
    which has a scratch level above every chip level: all four outputs of 2 frames against the host mirror.  Float messages at chip level 13
    hold more LDS than a launch gets unasked"""
    monkeypatch.setenv("QLDPC_POLAR_WIDE_CHIP", str(chip))
    monkeypatch.setenv("QLDPC_POLAR_WIDE_LANES", str(lanes))
    monkeypatch.setenv("QLDPC_POLAR_WIDE_LEAF", str(leaf))
    rng = np.random.default_rng([chip, lanes, leaf, messages == "i8"])
    n, F = 15, 2
    N = 1 << n
    pos, _ = R.random_code(rng, N)
    llr = _inputs(rng, messages, F, N, 31)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    dec = q.Polar(n, pos, messages, 31, max_frames=F, form="wide")      # reads the environment here
    out = _host(dec.decode(_dev(torch, llr), _dev(torch, fz), leaf=True))
    _same(out, q.polar_decode_host(n, pos, llr, fz, messages, 31, leaf=True), "chip=%d lanes=%d leaf=%d %s" % (chip, lanes, leaf, messages))
    esz = 1 if messages == "i8" else 4
    assert dec.device_bytes() == esz * F * (N - (2 << chip)) + 2 * 4 * F * (N // 32) + 4 * (N // 32) + 4 * max(len(pos), 1)


def test_small_frames_and_the_encoder_on_a_wide_context(q, torch):
    """n <= 5 is one leaf block in either form, and encode() serves a wide context as it serves a lanes one"""
    rng = np.random.default_rng(14)
    for n, F in ((3, 70), (11, 4)):
        W = max(1, (1 << n) // 32)
        u = rng.integers(0, 1 << 32, (F, W), dtype=np.uint64).astype(np.uint32)
        x = q.Polar(n, [0], "i8", 31, max_frames=F, form="wide").encode(_dev(torch, u))
        assert np.array_equal(x.cpu().numpy().view(np.uint32), q.polar_encode_host(n, u))

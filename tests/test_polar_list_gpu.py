"""GPU suite of the polar list decoder (qldpc_polar_list_*, qcrypto-ldpc_amd/csrc/qldpc_polar_list.hip): the device against the host mirror in every
output, bit for bit, in both message types and every list size; its identity with the SC decoder at list size 1; partial outputs; context reuse;
the published list-4 curve and the reconciliation form with the mirror's counts.  The mirror itself is held to the numpy restatement by
tests/test_polar_list_host.py."""
import numpy as np
import pytest

import polar_list_ref as LR
import polar_ref as R

pytestmark = pytest.mark.gpu

LISTS = (1, 2, 4, 8)


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


def _same(dev, host, what=""):
    assert set(dev) == set(host), what
    for k in host:
        assert np.array_equal(dev[k].view(np.uint32), host[k].view(np.uint32)), "%s: %s" % (what, k)


def _case(rng, n, messages, F, maxq=31, K=None):
    """a random code, inputs with ties, frozen values, a CRC 11 where the information word holds one, and expected remainders"""
    N = 1 << n
    pos, _ = R.random_code(rng, N, K)
    llr = R.i8_inputs(rng, F, N, maxq) if messages == "i8" else R.f32_inputs(rng, F, N)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    crc_len, crc_poly = LR.CRC11 if len(pos) >= 11 else (0, 0)
    crc = rng.integers(0, 1 << 11, F).astype(np.uint32) if crc_len else None
    return pos, llr, fz, crc, crc_len, crc_poly


def _both(q, torch, n, pos, llr, fz, crc, messages, maxq, L, crc_len, crc_poly, max_frames=None):
    dec = q.PolarList(n, pos, messages, maxq, L, crc_len, crc_poly, max_frames=max_frames or len(llr))
    dev = _host(dec.decode(_dev(torch, llr), _dev(torch, fz), _dev(torch, crc)))
    return dev, q.polar_list_decode_host(n, pos, llr, fz, crc, messages, maxq, L, crc_len, crc_poly)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("L", LISTS)
@pytest.mark.parametrize("n", [1, 4, 5, 6, 7, 10, 12])
def test_device_is_the_mirror(q, torch, n, L, messages):
    """70 frames: a full wave and a partial one.  n <= 5: the frame is one leaf block; n = 6, 7: the first levels in the scratch; n = 12: 128 words
    a row"""
    rng = np.random.default_rng([n, L, messages == "i8", 5])
    maxq = (1, 31, 126)[(n + L) % 3]
    pos, llr, fz, crc, crc_len, crc_poly = _case(rng, n, messages, 70, maxq)
    dev, host = _both(q, torch, n, pos, llr, fz, crc, messages, maxq, L, crc_len, crc_poly)
    _same(dev, host, "n=%d L=%d %s K=%d" % (n, L, messages, len(pos)))


@pytest.mark.parametrize("n,L,F", [(14, 8, 5), (16, 2, 3)])
@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_larger_sizes(q, torch, n, L, F, messages):
    rng = np.random.default_rng([n, L, messages == "i8"])
    pos, llr, fz, crc, crc_len, crc_poly = _case(rng, n, messages, F)
    dev, host = _both(q, torch, n, pos, llr, fz, crc, messages, 31, L, crc_len, crc_poly)
    _same(dev, host, "n=%d L=%d %s" % (n, L, messages))


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("K", [0, 1, 2, 1024])
def test_all_frozen_few_information_bits_and_rate_one(q, torch, messages, K):
    """fewer live paths than the list has slots (K < 3 at L = 8), and no frozen leaf at all"""
    rng = np.random.default_rng([K, messages == "i8"])
    pos, llr, fz, crc, crc_len, crc_poly = _case(rng, 10, messages, 70, 31, K)
    dev, host = _both(q, torch, 10, pos, llr, fz, crc, messages, 31, 8, crc_len, crc_poly)
    _same(dev, host, "K=%d %s" % (K, messages))


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_list_of_one_is_the_sc_decoder(q, torch, messages):
    rng = np.random.default_rng([10, messages == "i8", 1])
    n, F = 10, 130
    pos, llr, fz, _, _, _ = _case(rng, n, messages, F)
    d_llr, d_fz = _dev(torch, llr), _dev(torch, fz)
    sc = _host(q.Polar(n, pos, messages, 31, max_frames=F).decode(d_llr, d_fz))
    out = _host(q.PolarList(n, pos, messages, 31, 1, max_frames=F).decode(d_llr, d_fz))
    assert all(np.array_equal(out[k], sc[k]) for k in ("u", "info", "x"))
    assert not out["pick"].any() and np.array_equal(out["list_x"][:, 0], sc["x"])


def test_each_output_alone(q, torch):
    rng = np.random.default_rng(8)
    n, F, L = 8, 70, 4
    pos, llr, fz, crc, crc_len, crc_poly = _case(rng, n, "i8", F, 31, 100)
    dec = q.PolarList(n, pos, "i8", 31, L, crc_len, crc_poly, max_frames=F)
    host = q.polar_list_decode_host(n, pos, llr, fz, crc, "i8", 31, L, crc_len, crc_poly)
    d = [_dev(torch, a) for a in (llr, fz, crc)]
    for name in q.LIST_OUTPUTS:
        _same(_host(dec.decode(*d, want=(name,))), {name: host[name]}, name)
    assert dec.decode(*d, want=()) == {}
    _same(_host(dec.decode(*d)), host, "all")


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("K", [0, 33])
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("n", [5, 7])
def test_small_shape_edges_are_the_mirror(q, torch, n, L, K, messages):
    """the edges of what the three decoders share (the info row, the level step, the context): 65 frames (two groups, one live lane in the
    second), no information bit, and 33 of them (an info row whose second word holds one bit; N = 32 has no 33 positions, so n = 5 takes all
    32: one full word), with CRC 11 wherever the information word holds one.  Each output alone, then all together, against the host mirror"""
    rng = np.random.default_rng([n, L, K, messages == "i8", 17])
    pos, llr, fz, crc, crc_len, crc_poly = _case(rng, n, messages, 65, 31, min(K, 1 << n))
    dec = q.PolarList(n, pos, messages, 31, L, crc_len, crc_poly, max_frames=65)
    host = q.polar_list_decode_host(n, pos, llr, fz, crc, messages, 31, L, crc_len, crc_poly)
    d = [_dev(torch, a) for a in (llr, fz, crc)]
    for name in q.LIST_OUTPUTS:
        _same(_host(dec.decode(*d, want=(name,))), {name: host[name]}, "n=%d L=%d K=%d %s %s alone" % (n, L, len(pos), messages, name))
    _same(_host(dec.decode(*d)), host, "n=%d L=%d K=%d %s all" % (n, L, len(pos), messages))


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_context_reuse(q, torch, messages):
    """calls of 130, 3 and 64 frames on one context: a later call leaves no trace of an earlier one, and the context does not grow"""
    rng = np.random.default_rng(9)
    n, L = 8, 4
    pos, llr, fz, crc, crc_len, crc_poly = _case(rng, n, messages, 130, 31, 100)
    dec = q.PolarList(n, pos, messages, 31, L, crc_len, crc_poly, max_frames=130)
    size = dec.device_bytes()
    assert size > 0
    for lo, hi in ((0, 130), (40, 43), (60, 124)):
        host = q.polar_list_decode_host(n, pos, llr[lo:hi], fz[lo:hi], crc[lo:hi], messages, 31, L, crc_len, crc_poly)
        _same(_host(dec.decode(_dev(torch, llr[lo:hi]), _dev(torch, fz[lo:hi]), _dev(torch, crc[lo:hi]))), host, "frames %d .. %d" % (lo, hi))
    assert dec.device_bytes() == size


def test_refusals_of_a_call(q, torch):
    dec = q.PolarList(6, [5, 9], "i8", 31, 4, max_frames=64)
    with pytest.raises(q.QldpcError) as e:
        dec.decode(torch.zeros((65, 64), dtype=torch.int8, device="cuda"))
    assert e.value.status == -6
    with pytest.raises(q.QldpcError) as e:
        dec.decode(torch.zeros((4, 64), dtype=torch.int8, device="cuda"), crc=torch.zeros(4, dtype=torch.int32, device="cuda"))
    assert e.value.status == -1                                   # an expected remainder without a CRC
    out = dec.decode(torch.zeros((0, 64), dtype=torch.int8, device="cuda"))
    assert out["u"].shape == (0, 2) and out["list_x"].shape == (0, 4, 2)


@pytest.mark.parametrize("k", [2, 3])
def test_published_list_curve_on_the_device(q, torch, k):
    """the frames of the CPU suite: the device counts the host mirror's block errors exactly, so the point lies in the band around the published FER"""
    row, pos, msg, rq = LR.list_point(k)
    F = len(msg)
    dec = q.PolarList(10, pos, "i8", 31, 4, *LR.CRC11, max_frames=F)
    dev = _host(dec.decode(_dev(torch, rq), want=("info", "pick")))
    host = q.polar_list_decode_host(10, pos, rq, None, None, "i8", 31, 4, *LR.CRC11, want=("info", "pick"))
    errs = lambda o: int((R.info_bits(o["info"].view(np.uint32), len(pos))[:, :msg.shape[1]] != msg).any(axis=1).sum())
    e_dev, e_host = errs(dev), errs(host)
    print("Eb/N0 %.2f dB: device %d, mirror %d of %d; published %d / %d" % (row[0], e_dev, e_host, F, row[3], row[5]))
    _same(dev, host, "point %d" % k)
    assert e_dev == e_host
    assert abs(e_dev / F - row[1]) <= R.fer_band(row, F)


def test_reconciliation_form_on_the_device(q, torch):
    """QBER 0.06, float messages, Alice's frozen values and CRC: the same keys fail on the device as on the mirror"""
    pos, x, frozen, llr = LR.recon_frames()
    crc = q.polar_crc_host(*LR.CRC11, R.pack(R.encode(x)[:, pos]), len(pos))
    dec = q.PolarList(10, pos, "f32", 31, 4, *LR.CRC11, max_frames=len(x))
    dev = _host(dec.decode(_dev(torch, llr), _dev(torch, frozen), _dev(torch, crc), want=("x", "pick")))
    host = q.polar_list_decode_host(10, pos, llr, frozen, crc, "f32", 31, 4, *LR.CRC11, want=("x", "pick"))
    _same(dev, host, "reconciliation")
    failed = lambda o: (o["x"].view(np.uint32) != R.pack(x)).any(axis=1) | (o["pick"] < 0)
    assert np.array_equal(failed(dev), failed(host)) and failed(dev).any()

"""Monte-Carlo FER loop (qldpc_mc_*), host suite: qldpc_mc_philox_host / qldpc_mc_frames_host run the functions of
csrc/qldpc_mc_core.h that the kernels run per lane, so the frame definition is checked here without a device, against the numpy
restatement in tests/mc_ref.py.  Every comparison is exact equality of words."""
import os
import subprocess

import numpy as np
import pytest

import mc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
FAR = 2 ** 32 - 100                        # 192 frames from here carry the index into the counter's high word
# (K, N, info_bits_pos): PEGReg504x1008 with the IDENTITY encoder's positions, and an IRA code whose K and N both leave a partial last word
CODES = {"peg": (504, 1008, np.arange(504, 1008, dtype=np.int32)), "ira": (1590, 2000, None)}

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_philox_known_answers(q, ctr, key, out):
    assert [int(v) for v in q.mc_philox_host(ctr, key)] == list(out)
    assert [int(v) for v in mc_ref.philox(*ctr, *key)] == list(out)      # and the restatement the other tests compare against


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("first", [0, FAR])
def test_frames_host_equals_the_restatement(q, name, first):
    K, N, pos = CODES[name]
    assert K % 32 and N % 32 or name == "peg"
    info, flips = q.mc_frames_host(K, N, SEED, 0.07, first, 192, info_bits_pos=pos)
    ref_info, ref_flips = mc_ref.frames(K, N, SEED, 0.07, first, 192, info_bits_pos=pos)
    assert info.dtype == np.uint32 and info.shape == ref_info.shape == (192, (K + 31) // 32) and (info == ref_info).all()
    assert flips.shape == ref_flips.shape == (192, (N + 31) // 32) and (flips == ref_flips).all()
    if K % 32:
        assert not (info[:, -1] & np.uint32((1 << (32 - K % 32)) - 1)).any() and (info[:, -1] != 0).any()
    if N % 32:
        assert not (flips[:, -1] & np.uint32((1 << (32 - N % 32)) - 1)).any()
    f = mc_ref.unpack(flips, N)
    cls = mc_ref.classes(K, N, pos)
    assert not f[:, cls == 1].any()                                       # disclosed parity is exact at parity_ber = 0
    assert abs(f[:, cls == 0].mean() - 0.07) < 5 * np.sqrt(0.07 * 0.93 / (192 * K))
    assert abs(mc_ref.unpack(info, K).mean() - 0.5) < 5 * 0.5 / np.sqrt(192 * K)
    if first == FAR:                                                      # the frames past 2^32 are not the frames from 0 again
        assert (info[100:] != q.mc_frames_host(K, N, SEED, 0.07, 0, 92, info_bits_pos=pos)[0]).any()


@pytest.mark.parametrize("name", sorted(CODES))
def test_frames_host_classes_and_thresholds(q, name):
    K, N, pos = CODES[name]
    cls = mc_ref.classes(K, N, pos).copy()
    par = np.nonzero(cls == 1)[0]
    cls[par[::7]] = q.VN_PUNCTURED
    info, flips = q.mc_frames_host(K, N, SEED, 0.04, 5, 64, vn_class=cls, parity_ber=0.25)
    ref_info, ref_flips = mc_ref.frames(K, N, SEED, 0.04, 5, 64, vn_class=cls, parity_ber=0.25)
    assert (info == ref_info).all() and (flips == ref_flips).all()
    f = mc_ref.unpack(flips, N)
    assert not f[:, cls == 2].any()
    pin = f[:, cls == 1]
    assert abs(pin.mean() - 0.25) < 5 * np.sqrt(0.25 * 0.75 / pin.size)   # dirty disclosed parity flips at parity_ber
    # the channel VNs do not see parity_ber, the info words see neither probability
    info0, flips0 = q.mc_frames_host(K, N, SEED, 0.04, 5, 64, vn_class=cls)
    assert (info0 == info).all() and (mc_ref.unpack(flips0, N)[:, cls == 0] == f[:, cls == 0]).all() and not mc_ref.unpack(flips0, N)[:, cls != 0].any()
    none = q.mc_frames_host(K, N, SEED, 0.0, 5, 64, info_bits_pos=pos)[1]
    assert not none.any()
    # a threshold is floor(p 2^32): the largest p below 1 flips all but a 2^-32 share, the smallest positive one nothing here
    full = mc_ref.unpack(q.mc_frames_host(K, N, SEED, np.nextafter(1.0, 0.0), 5, 8, info_bits_pos=pos)[1], N)
    assert full[:, cls != 0].sum() == 0 and full[:, mc_ref.classes(K, N, pos) == 0].all()
    assert not q.mc_frames_host(K, N, SEED, 2.0 ** -33, 5, 8, info_bits_pos=pos)[1].any()
    other = q.mc_frames_host(K, N, SEED + 1, 0.04, 5, 64, vn_class=cls, parity_ber=0.25)
    assert (other[0] != info).any() and (other[1] != flips).any()


@pytest.mark.parametrize("name", sorted(CODES))
def test_a_range_equals_its_parts(q, name):
    K, N, pos = CODES[name]
    whole = q.mc_frames_host(K, N, SEED, 0.05, 0, 192, info_bits_pos=pos)
    a = q.mc_frames_host(K, N, SEED, 0.05, 0, 70, info_bits_pos=pos)
    b = q.mc_frames_host(K, N, SEED, 0.05, 70, 122, info_bits_pos=pos)
    for k in (0, 1):
        assert (np.concatenate([a[k], b[k]]) == whole[k]).all()


def test_frames_host_argument_checks(q):
    K, N, pos = CODES["peg"]
    for bad in (dict(qber=-0.1), dict(qber=1.0), dict(qber=float("nan")), dict(parity_ber=1.0), dict(parity_ber=-1e-9)):
        kw = dict(dict(qber=0.05), **bad)
        qber = kw.pop("qber")
        with pytest.raises(q.QldpcError) as e:
            q.mc_frames_host(K, N, SEED, qber, 0, 4, info_bits_pos=pos, **kw)
        assert e.value.status == -6, bad
    for k, n in ((0, 8), (9, 8), (4, 0)):
        with pytest.raises(q.QldpcError) as e:
            q.mc_frames_host(k, n, SEED, 0.05, 0, 4)
        assert e.value.status == -6
    with pytest.raises(q.QldpcError):
        q.mc_frames_host(K, N, SEED, 0.05, 0, 4, info_bits_pos=pos[:-1])
    with pytest.raises(q.QldpcError) as e:
        q.mc_frames_host(K, N, SEED, 0.05, 0, 4, info_bits_pos=np.concatenate([pos[:-1], pos[:1]]))
    assert e.value.status == -1
    with pytest.raises(q.QldpcError) as e:
        q.mc_frames_host(K, N, SEED, 0.05, 0, 4, vn_class=np.full(N, 3, np.uint8))
    assert e.value.status == -1
    with pytest.raises(q.QldpcError):
        q.mc_frames_host(K, N, SEED, 0.05, 0, 4, vn_class=np.zeros(N - 1, np.uint8))
    with pytest.raises(q.QldpcError):
        q.mc_frames_host(K, N, SEED, 0.05, 0, -1, info_bits_pos=pos)
    info, flips = q.mc_frames_host(K, N, SEED, 0.05, 0, 0, info_bits_pos=pos)
    assert info.shape == (0, 16) and flips.shape == (0, 32)
    with pytest.raises(q.QldpcError):
        q.mc_philox_host((0, 0, 0), (0, 0))


def test_host_mirror_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mc_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "c", "mc_sanitize.c"),
                           os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr

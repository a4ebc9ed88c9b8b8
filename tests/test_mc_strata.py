"""Fixed-weight error strata (qldpc_mc_weight_frames_host, qldpc_mc_strata_fer_host), host suite: the C mirror runs the functions of
csrc/qldpc_mc_core.h that the kernel mc_channel_weight runs per lane, so the fixed-weight frame definition is checked here without a device,
against the numpy restatement of tests/mc_strata_ref.py (a lexsort, where the library selects), and against the BSC frames of
qldpc_mc_frames_host, whose frame with c flips is the fixed-weight frame of weight c.  Words are compared for exact equality; the estimate
against exact rational arithmetic to 1e-9 relative."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mc_ref
import mc_strata_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
FAR = 2 ** 32 - 100                        # 192 frames from here carry the index into the counter's high word


def _mixed(N, seed):
    """a class map that interleaves channel, pinned and punctured VNs"""
    return np.random.default_rng(seed).choice(np.array([0, 0, 1, 2], np.uint8), N)


# name -> (K, N, info_bits_pos, vn_class): the two codes of the GPU suite, the three classes interleaved on N % 32 != 0 and on N % 4 != 0
SHAPES = {"peg": (504, 1008, np.arange(504, 1008, dtype=np.int32), None), "ira": (1590, 2000, None, None),
          "mixed": (300, 1000, None, _mixed(1000, 3)), "odd": (40, 131, None, _mixed(131, 4))}


def _channel_mask(K, N, pos, cls):
    return mc_ref.pack((mc_ref.classes(K, N, pos, cls) == 0)[None, :])[0]


def _popcount_rows(words):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), axis=1).sum(1)


@pytest.mark.parametrize("parity_ber", [0.0, 0.1])
@pytest.mark.parametrize("key_bits", [32, 8, 4, 1])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mirror_equals_the_restatement(q, name, key_bits, parity_ber):
    K, N, pos, cls = SHAPES[name]
    channel_vns = int((mc_ref.classes(K, N, pos, cls) == 0).sum())
    mask = _channel_mask(K, N, pos, cls)
    n = 6
    for first in (0, FAR + 97):                                                           # the second crosses 2^32 inside the six frames
        for weight in (0, 1, channel_vns // 3, channel_vns - 1, channel_vns):
            info, flips = q.mc_weight_frames_host(K, N, SEED, weight, first, n, key_bits, info_bits_pos=pos, vn_class=cls, parity_ber=parity_ber)
            ref_info, ref_flips = mc_strata_ref.frames(K, N, SEED, weight, first, n, key_bits, pos, cls, parity_ber)
            assert info.shape == ref_info.shape and (info == ref_info).all()
            assert flips.shape == ref_flips.shape and (flips == ref_flips).all(), (name, key_bits, first, weight)
            assert (_popcount_rows(flips & mask) == weight).all()
            if parity_ber == 0.0:
                assert (_popcount_rows(flips) == weight).all()                            # nothing outside the channel VNs, the padding included
    # one weight per frame, and key_bits = 0 standing for 32
    w = np.array([0, 1, 2, channel_vns // 2, channel_vns - 1, channel_vns], np.int32)
    got = q.mc_weight_frames_host(K, N, SEED + 1, w, FAR + 97, n, key_bits % 32, info_bits_pos=pos, vn_class=cls, parity_ber=parity_ber)[1]
    assert (got == mc_strata_ref.frames(K, N, SEED + 1, w, FAR + 97, n, key_bits, pos, cls, parity_ber)[1]).all()
    if key_bits <= 4:      # the middle weight cut through a group of equal keys, so the rows above went through the tie rule
        assert mc_strata_ref.boundary_ties(K, N, SEED, channel_vns // 3, 0, n, key_bits, pos, cls).any()


def test_ties_occur_at_the_selection_boundary(q):
    """at key_bits <= 4 a weight in the middle of the channel VNs cuts through a group of equal keys in every frame, so the rows of
    test_mirror_equals_the_restatement reach the rule `equal keys go to the lower VN`; and the rule is visible: among the VNs that hold the
    boundary key, the taken ones are exactly the lowest"""
    for name in sorted(SHAPES):
        K, N, pos, cls = SHAPES[name]
        classes = mc_ref.classes(K, N, pos, cls)
        chan = np.nonzero(classes == 0)[0]
        for key_bits in (4, 1):
            weight = chan.size // 3
            tied = mc_strata_ref.boundary_ties(K, N, SEED, weight, 0, 6, key_bits, pos, cls)
            assert tied.any(), (name, key_bits)
            flips = mc_ref.unpack(q.mc_weight_frames_host(K, N, SEED, weight, 0, 6, key_bits, info_bits_pos=pos, vn_class=cls)[1], N)
            key = mc_strata_ref.keys(N, SEED, 0, 6, key_bits)[1]
            for f in np.nonzero(tied)[0]:
                T = np.sort(key[f, chan])[weight - 1]
                at = chan[key[f, chan] == T]
                took = flips[f, at].astype(bool)
                assert took.any() and not took.all() and (np.diff(took.astype(int)) <= 0).all()      # a prefix of the group, in VN order
                assert flips[f, chan[key[f, chan] < T]].all() and not flips[f, chan[key[f, chan] > T]].any()


@pytest.mark.parametrize("qber", [0.03, 0.26])
@pytest.mark.parametrize("name", ["peg", "ira", "mixed"])
def test_a_bsc_frame_is_the_fixed_weight_frame_of_its_own_flip_count(q, name, qber):
    K, N, pos, cls = SHAPES[name]
    mask = _channel_mask(K, N, pos, cls)
    n = 48
    for first in (0, FAR + 60):
        info, bsc = q.mc_frames_host(K, N, SEED, qber, first, n, info_bits_pos=pos, vn_class=cls, parity_ber=0.1)
        counts = _popcount_rows(bsc & mask).astype(np.int32)
        assert len(set(counts.tolist())) > 5                                              # the binomial spread: many different weights
        winfo, fixed = q.mc_weight_frames_host(K, N, SEED, counts, first, n, info_bits_pos=pos, vn_class=cls, parity_ber=0.1)
        assert (winfo == info).all() and (fixed == bsc).all()
        up = q.mc_weight_frames_host(K, N, SEED, counts + 1, first, n, info_bits_pos=pos, vn_class=cls, parity_ber=0.1)[1]
        assert (_popcount_rows(up ^ fixed) == 1).all() and ((up & fixed) == fixed).all()   # nested: one more bit, none lost


def _cases():
    rng = np.random.default_rng(5)
    out = []
    for n, qber in ((1590, 0.03), (1590, 0.01), (504, 0.26), (2000, 0.11), (37, 0.5)):
        mean = int(n * qber)
        lo, hi = max(0, mean - 30), min(n, mean + 40)
        for weights in (np.arange(lo, hi + 1), np.arange(lo, hi + 1, 7), np.array([lo, lo + 1, lo + 9, hi]), np.array([mean])):
            frames = rng.integers(1, 5000, weights.size)
            fe = (frames * np.clip((weights - lo) / max(hi - lo, 1) + rng.normal(0, 0.05, weights.size), 0, 1)).astype(np.int64)
            out.append((n, weights.astype(np.int32), frames, fe, qber))
    return out


def test_estimate_equals_exact_arithmetic(q):
    """tolerance: the library forms b(w) by lgamma in double, whose error against exact arithmetic grows with n * eps (measured 2.6e-12 at
    n = 1590); 1e-9 relative on each output leaves three decades, and no case here has a tail so small that it leaves the normal doubles"""
    for n, weights, frames, fe, qber in _cases():
        got = q.mc_strata_fer(n, weights, frames, fe, qber)
        ref = mc_strata_ref.fer(n, weights, frames, fe, qber)
        print(n, qber, weights.size, got, ref)
        assert all(r == 0.0 or r > 1e-290 for r in ref)
        for g, r in zip(got, ref):
            assert g == pytest.approx(r, rel=1e-9, abs=0.0), (n, qber, weights, got, ref)


def test_estimate_with_every_weight_simulated(q):
    for n, qber in ((1590, 0.03), (300, 0.2), (1, 0.7)):
        w = np.arange(n + 1)
        out = q.mc_strata_fer(n, w, np.full(n + 1, 10), np.full(n + 1, 10), qber)
        assert abs(out[0] - 1.0) < 1e-12 and out[1] == 0.0 and out[2] == 0.0 and out[3] == 0.0
        half = q.mc_strata_fer(n, w, np.full(n + 1, 10), np.full(n + 1, 5), qber)
        assert abs(half[0] - 0.5) < 1e-12 and half[3] > 0.0


def test_refusals(q):
    z = np.zeros(1, np.uint32)
    good = dict(K=40, N=131, seed=1, weights=3, first_frame=0, n_frames=2)

    def refused(status, **kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(q.QldpcError) as e:
            q.mc_weight_frames_host(**args)
        assert e.value.status == status, (kw, e.value)

    refused(-6, weights=41)                                                               # above the channel VNs
    refused(-6, weights=-1)
    refused(-6, weights=np.array([0, 41]))
    refused(-6, key_bits=33)
    refused(-6, key_bits=-1)
    refused(-6, parity_ber=1.0)
    refused(-6, K=0)
    refused(-6, K=132)
    refused(-1, vn_class=np.full(131, 3, np.uint8))
    refused(-1, info_bits_pos=np.zeros(40, np.int32))                                     # repeated positions
    assert q._L.qldpc_mc_weight_frames_host(40, 131, None, None, 1, 0.0, 0, 2, None, 0, None, z.ctypes.data_as(q._up)) == -1      # no weights
    assert q._L.qldpc_mc_weight_frames_host(40, 131, None, None, 1, 0.0, 0, 2, None, 0, None, None) == -1                         # nothing to write
    assert q.mc_weight_frames_host(40, 131, 1, 40, 0, 0)[1].shape == (0, 5)               # no frames: nothing to do

    fine = dict(n_channel=100, weights=[3, 5, 9], frames=[10, 10, 10], frame_errors=[0, 5, 10], qber=0.05)

    def fer_refused(status, **kw):
        args = dict(fine)
        args.update(kw)
        with pytest.raises(q.QldpcError) as e:
            q.mc_strata_fer(**args)
        assert e.value.status == status, (kw, e.value)

    assert q.mc_strata_fer(**fine)[0] > 0
    fer_refused(-6, weights=[3, 5, 101])
    fer_refused(-6, weights=[-1, 5, 9])
    fer_refused(-6, weights=[], frames=[], frame_errors=[])                               # n_strata = 0
    fer_refused(-6, frames=[10, 0, 10], frame_errors=[0, 0, 10])
    fer_refused(-6, qber=0.0)
    fer_refused(-6, qber=1.0)
    fer_refused(-6, n_channel=0)
    fer_refused(-1, weights=[3, 3, 9])
    fer_refused(-1, weights=[5, 3, 9])
    w = np.array([3, 5], np.int32)
    f = np.array([4, 4], np.uint64)
    out = np.zeros(4)
    dp = C.POINTER(C.c_double)
    assert q._L.qldpc_mc_strata_fer_host(100, 2, None, f.ctypes.data_as(q._u64p), f.ctypes.data_as(q._u64p), 0.1, out.ctypes.data_as(dp)) == -1
    assert q._L.qldpc_mc_strata_fer_host(100, 2, w.ctypes.data_as(q._ip), None, f.ctypes.data_as(q._u64p), 0.1, out.ctypes.data_as(dp)) == -1
    assert q._L.qldpc_mc_strata_fer_host(100, 2, w.ctypes.data_as(q._ip), f.ctypes.data_as(q._u64p), f.ctypes.data_as(q._u64p), 0.1, None) == -1


def test_host_mirrors_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mc_strata_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "mc_strata_sanitize.c"),
                           os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr

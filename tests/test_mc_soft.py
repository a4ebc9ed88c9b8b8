"""Quantised soft-output channels of the Monte-Carlo loop, host suite: qldpc_mc_llr_host runs the functions of csrc/qldpc_mc_core.h that
mc_soft_channel runs per lane, so the channel definition is checked here without a device against the numpy restatement in
tests/mc_soft_ref.py; qldpc_mc_awgn_table against math.erfc.  Exact equality everywhere but the +-2 counts of the two erfc paths."""
import os
import subprocess

import numpy as np
import pytest

import mc_ref
import mc_soft_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
FAR = 2 ** 32 - 100
TWO32 = 2 ** 32
# (K, N, info_bits_pos): PEGReg504x1008 with the IDENTITY encoder's positions; N = 1998 (1998.5.3.2665.alist): N % 4 = 2, N % 32 = 14
CODES = {"peg": (504, 1008, np.arange(504, 1008, dtype=np.int32)), "a1998": (1776, 1998, None)}


def f32_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and (a.view(np.uint32) == b.view(np.uint32)).all()


@pytest.fixture(scope="module")
def tables(q):
    return mc_soft_ref.tables(q)


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("first", [0, FAR])
@pytest.mark.parametrize("shape", ["awgn64", "q2", "q256"])
def test_llr_host_equals_the_restatement(q, tables, name, first, shape):
    K, N, pos = CODES[name]
    assert N % 4 == 2 and N % 32 or name == "peg"
    table = tables[shape]
    cw = np.random.default_rng(3).integers(0, 2, (150, N)).astype(np.uint8)      # any words: the channel does not ask for codewords
    llr, flips = q.mc_llr_host(K, N, SEED, table, first, 150, cw_words=mc_ref.pack(cw), info_bits_pos=pos)
    ref_llr, ref_flips = mc_soft_ref.llr_frames(K, N, SEED, table, first, 150, cw_bits=cw, info_bits_pos=pos)
    assert f32_equal(llr, ref_llr) and flips.dtype == np.uint32 and flips.shape == ref_flips.shape and (flips == ref_flips).all()
    cls = mc_ref.classes(K, N, pos)
    assert (np.abs(llr[:, cls == 1]) == mc_soft_ref.PIN).all() and not mc_ref.unpack(flips, N)[:, cls == 1].any()      # parity_ber = 0
    if N % 32:
        assert not (flips[:, -1] & np.uint32((1 << (32 - N % 32)) - 1)).any()
    # every level that has a probability occurs, no other does
    cum = [np.concatenate([[0], np.asarray(c, np.uint64), [TWO32]]).astype(np.int64) for c in table[:2]]
    for b in (0, 1):
        seen = np.unique(llr[:, cls == 0][cw[:, cls == 0] == b])
        possible = np.asarray(table[2])[np.diff(cum[b]) * 150.0 * K / 2 / TWO32 > 40]
        assert np.isin(possible, seen).all() and np.isin(seen, np.asarray(table[2])[np.diff(cum[b]) > 0]).all()
    # the all-zero codeword is what a NULL row stands for; a range equals its parts
    zero = q.mc_llr_host(K, N, SEED, table, first, 60, info_bits_pos=pos)
    ref_zero = mc_soft_ref.llr_frames(K, N, SEED, table, first, 60, info_bits_pos=pos)
    assert f32_equal(zero[0], ref_zero[0]) and (zero[1] == ref_zero[1]).all()
    a = q.mc_llr_host(K, N, SEED, table, first, 23, info_bits_pos=pos)
    b = q.mc_llr_host(K, N, SEED, table, first + 23, 37, info_bits_pos=pos)
    for k in (0, 1):
        assert (np.concatenate([a[k], b[k]]).view(np.uint32) == zero[k].view(np.uint32)).all()
    if first == FAR:                                                      # the frames past 2^32 are not the frames from 0 again
        assert (llr[100:] != q.mc_llr_host(K, N, SEED, table, 0, 50, cw_words=mc_ref.pack(cw[100:]), info_bits_pos=pos)[0]).any()


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("parity_ber", [0.0, 0.25])
@pytest.mark.parametrize("shape", ["awgn64", "q256"])
def test_llr_host_mixed_classes(q, tables, name, parity_ber, shape):
    K, N, _ = CODES[name]
    cls = mc_soft_ref.mixed_classes(N)
    cw = np.random.default_rng(4).integers(0, 2, (64, N)).astype(np.uint8)
    llr, flips = q.mc_llr_host(K, N, SEED + 1, tables[shape], 5, 64, cw_words=mc_ref.pack(cw), vn_class=cls, parity_ber=parity_ber)
    ref_llr, ref_flips = mc_soft_ref.llr_frames(K, N, SEED + 1, tables[shape], 5, 64, cw_bits=cw, vn_class=cls, parity_ber=parity_ber)
    assert f32_equal(llr, ref_llr) and (flips == ref_flips).all()
    f = mc_ref.unpack(flips, N)
    assert (llr[:, cls == 2] == 0).all() and not f[:, cls == 2].any()
    pin = f[:, cls == 1]
    assert (np.abs(llr[:, cls == 1]) == mc_soft_ref.PIN).all()
    assert (pin == ((llr[:, cls == 1] < 0) != (cw[:, cls == 1] == 1))).all()
    assert abs(pin.mean() - parity_ber) <= 5 * np.sqrt(parity_ber * (1 - parity_ber) / pin.size)
    if shape == "q256":                                                   # LLR 0 (level 7) is no flip, whichever bit was sent
        chan = cls == 0
        assert (llr[:, chan] == 0).any() and not f[:, chan][llr[:, chan] == 0].any()
    # the BSC's frames are another stream: the info words and the BSC flips do not depend on anything here
    other = q.mc_llr_host(K, N, SEED, tables[shape], 5, 64, cw_words=mc_ref.pack(cw), vn_class=cls, parity_ber=parity_ber)
    assert (other[0] != llr).any()


def test_awgn_table_against_erfc(q):
    for sigma, rmax, maxq in ((0.8414, 3.0, 31), (1.0, 3.0, 31), (0.5, 2.0, 7), (0.05, 3.0, 127), (3.0, 1.0, 1)):
        c0, c1, value = q.mc_awgn_table(sigma, rmax, maxq)
        r0, r1, rvalue = mc_soft_ref.awgn_table(sigma, rmax, maxq)
        Q = 2 * maxq + 2
        assert c0.shape == c1.shape == (Q - 1,) and c0.dtype == np.uint64 and value.shape == (Q,)
        assert (value.view(np.uint32) == rvalue.view(np.uint32)).all() and value[0] == -maxq - 1 and value[-1] == maxq
        for got, ref in ((c0, r0), (c1, r1)):
            assert np.abs(got.astype(np.int64) - ref.astype(np.int64)).max() <= 2
            assert (np.diff(got.astype(np.int64)) >= 0).all() and int(got.max()) <= TWO32
            probs = np.diff(np.concatenate([[0], got, [TWO32]]).astype(np.int64))
            assert (probs >= 0).all() and int(probs.sum()) == TWO32           # the level probabilities of a row add up to exactly 1
        assert (c1 >= c0).all() and (c1 > c0).any()                           # a sent 1 (symbol -1) lies lower
    # sigma = 0.05: levels nothing reaches on either side (entries 0 and entries 2^32)
    c0, c1, _ = q.mc_awgn_table(0.05, 3.0, 127)
    assert c0[0] == 0 and c0[-1] == TWO32 and c1[0] == 0 and c1[-1] == TWO32
    # the hard-decision error rate of the table is Phi(-1 / sigma): the boundary at 0 is threshold maxq
    c0, _, value = q.mc_awgn_table(0.8414)
    assert value[31] == -1 and value[32] == 0
    import math
    assert abs(int(c0[31]) - math.floor(TWO32 * 0.5 * math.erfc(1 / 0.8414 / math.sqrt(2.0)))) <= 2
    for bad in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(rmax=0.0), dict(rmax=float("inf")),
                dict(maxq=0), dict(maxq=128), dict(maxq=-1)):
        with pytest.raises(q.QldpcError) as e:
            q.mc_awgn_table(**dict(dict(sigma=1.0, rmax=3.0, maxq=31), **bad))
        assert e.value.status == -6, bad
    assert abs(q.mc_awgn_sigma(1.5, 0.5) - 0.8414) < 5e-5


def test_llr_host_argument_checks(q, tables):
    K, N, pos = CODES["peg"]
    c0, c1, value = tables["awgn64"]
    good = q.mc_llr_host(K, N, SEED, (c0, c1, value), 0, 2, info_bits_pos=pos)

    def refused(status, table, **kw):
        with pytest.raises(q.QldpcError) as e:
            q.mc_llr_host(K, N, SEED, table, 0, 2, **dict(dict(info_bits_pos=pos), **kw))
        assert e.value.status == status, (table[2].size, kw)

    refused(-6, (c0[:0], c1[:0], value[:1]))                                  # Q = 1
    refused(-6, (np.zeros(256, np.uint64), np.zeros(256, np.uint64), np.zeros(257, np.float32)))      # Q = 257
    refused(-6, (c0, c1[:-1], value))                                         # rows of different length
    dec = c0.copy()
    dec[10] = dec[9] - 1
    refused(-1, (dec, c1, value))                                             # a decreasing row
    refused(-1, (c0, dec, value))
    over = c1.copy()
    over[-1] = TWO32 + 1
    refused(-1, (c0, over, value))                                            # an entry above 2^32
    refused(-6, (c0, c1, value), parity_ber=1.0)
    refused(-6, (c0, c1, value), parity_ber=-0.1)
    refused(-1, (c0, c1, value), vn_class=np.full(N, 3, np.uint8))
    with pytest.raises(q.QldpcError):
        q.mc_llr_host(K, N, SEED, (c0, c1, value), 0, 2, cw_words=np.zeros((2, 31), np.uint32), info_bits_pos=pos)
    with pytest.raises(q.QldpcError):
        q.mc_llr_host(K, N, SEED, (c0, c1, value), 0, -1, info_bits_pos=pos)
    t, keep = q._mc_channel_arg(c0, c1, value, "test")
    t.reserved[1] = 1
    llr = np.zeros((2, N), np.float32)
    assert q._L.qldpc_mc_llr_host(K, N, None, None, SEED, 0.0, t, None, 0, 2, llr.ctypes.data_as(q._fp), None) == -1 and not llr.any()
    full = np.full(255, TWO32, np.uint64)                                     # legal: every VN at level 0
    llr, flips = q.mc_llr_host(K, N, SEED, (full, full, np.arange(256, dtype=np.float32) - 3), 0, 2, info_bits_pos=np.arange(K))
    assert (llr[:, :K] == -3).all() and mc_ref.unpack(flips, N)[:, :K].all()
    none = np.zeros(1, np.uint64)                                             # and every VN at level 1
    llr, flips = q.mc_llr_host(K, N, SEED, (none, none, np.array([-1, 4], np.float32)), 0, 2, info_bits_pos=np.arange(K))
    assert (llr[:, :K] == 4).all() and not flips.any()
    empty = q.mc_llr_host(K, N, SEED, (c0, c1, value), 0, 0, info_bits_pos=pos)
    assert empty[0].shape == (0, N) and empty[1].shape == (0, 32)
    again = q.mc_llr_host(K, N, SEED, (c0, c1, value), 0, 2, info_bits_pos=pos)
    assert f32_equal(again[0], good[0])


def test_soft_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mc_soft_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "c", "mc_soft_sanitize.c"),
                           os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr

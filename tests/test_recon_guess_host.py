"""CPU suite: the verdict of a guessing round inside a reconciliation session -- the host mirror qldpc_recon_guess_settle_host (the functions the lanes of
rk_guess_crc and rk_guess_settle run, csrc/qldpc_recon_guess_core.h) against the restatement of tests/recon_guess_ref.py.  No GPU compute.

The issue names a hand-built case "two passing trials that differ only in the last valid bit (ambiguous)".  Two keys that differ in one bit never share a
CRC-32, so both cannot pass; the case is built with the nearest thing that exists: the second key differs by the CRC collision pattern inside the last 33
valid bits, which contains the last valid bit (recon_guess_ref.collision)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import recon_guess_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def settle_host(q, g, b):
    return q.recon_guess_settle_host(g, b["rows"], b["ok"], b["iters"], b["keys"], b["key_bits"], b["want"], b["first"])


def settle_ref(g, b):
    return R.settle(g, b["rows"], b["ok"], b["iters"], b["keys"], b["key_bits"], b["want"], b["first"])


def test_the_restated_crc_is_the_library_s(q):
    rng = np.random.default_rng(5)
    for kb in [1, 31, 32, 33, 1000, 4097]:
        w = rng.integers(0, 2 ** 32, (kb + 31) // 32, dtype=np.uint64).astype(np.uint32)
        assert R.crc(w, kb) == q.crc32_words(w, kb)
        if kb >= 33:
            pat = R.collision(kb)
            assert pat.any() and (pat[-1] >> np.uint32((-kb) % 32)) & 1 and not (pat & ~R.mask_words(kb)).any()      # holds the last valid bit, nothing past it
            assert q.crc32_words(w ^ pat, kb) == q.crc32_words(w, kb)


@pytest.mark.parametrize("g", [0, 1, 3, 7, 10])
@pytest.mark.parametrize("kb", [1, 31, 32, 33, 1000])
def test_settle_equals_the_restated_rule(q, g, kb):
    rng = np.random.default_rng(1000 * g + kb)
    T, Wk = 1 << g, (kb + 31) // 32 + 1                                            # key rows one word wider than the key, trial rows wider still
    for p_pass, p_wrong in [(0.0, 0.0), (0.0, 0.3), (1.0, 0.0), (0.05, 0.2), (0.4, 0.4)] + ([(2.0 / T, 8.0 / T)] if T > 16 else []):
        kbs = [kb, kb, max(1, kb - 1)]
        kinds = [R.random_kinds(rng, T, k, p_pass, p_wrong) for k in kbs]
        b = R.batch(rng, g, kbs, Wk, Wk + 3, kinds)
        got, want = settle_host(q, g, b), settle_ref(g, b)
        assert R.same(got, want) is None, (g, kb, p_pass, R.same(got, want))
        for s in range(3):                                                         # the verdict against the kinds the rows were built from
            assert kbs[s] >= 33 or not got["guess"]["ambiguous"][s]                # keys of fewer than 33 bits never collide
            passing = [t for t, k in enumerate(kinds[s]) if k in "ac"]
            assert got["guess"]["winner"][s] == (passing[0] if passing else -1) and got["guess"]["n_pass"][s] == len(passing)
            assert got["guess"]["n_ok"][s] == sum(k in "acw" for k in kinds[s])
            assert got["guess"]["ambiguous"][s] == (len({kinds[s][t] for t in passing}) == 2)


def test_hand_built_cases(q):
    rng = np.random.default_rng(11)
    for T in (8, 128):
        g = T.bit_length() - 1
        for name, (kinds, kb, verdict) in R.hand_built(T).items():
            Wk = (kb + 31) // 32 + 2
            b = R.batch(rng, g, [kb], Wk, Wk + 5, [kinds])
            got = settle_host(q, g, b)
            assert tuple(int(got["guess"][f][0]) for f in ("winner", "n_ok", "n_pass", "ambiguous")) == verdict, name
            assert got["guess"]["tried"][0] == 1 and got["guess"]["trial_iterations"][0] == b["iters"].sum()
            nw, m = (kb + 31) // 32, R.mask_words(kb)
            if verdict[0] >= 0:
                assert got["status"][0] == 0 and (got["keys"][0, :nw] == (b["rows"][verdict[0], :nw] & m)).all(), name
                assert got["iterations"][0] == b["first"][0] + b["iters"][verdict[0]] and R.crc(got["keys"][0], kb) == b["want"][0]
                assert got["corrected"][0] == sum(bin(int(x)).count("1") for x in (b["keys"][0, :nw] ^ got["keys"][0, :nw]) & m) > 0
            else:
                assert got["status"][0] == -9 and (got["keys"][0, :nw] == b["keys"][0, :nw]).all(), name      # the key handed in, padding and all
                assert got["iterations"][0] == b["first"][0] and got["corrected"][0] == 0
            assert not got["keys"][0, nw:].any()                                   # nothing is written past the key's words
            assert R.same(got, settle_ref(g, b)) is None, name


def test_argument_errors_and_struct_size(q):
    rng = np.random.default_rng(2)
    b = R.batch(rng, 3, [40], 2, 4, ["xaxxwxxx"])
    for g in (-1, 11):
        with pytest.raises(q.QldpcError) as e:
            settle_host(q, g, b)
        assert e.value.status == -6
    for kb in (0, 65):                                                             # outside 1 .. 32 Wk
        with pytest.raises(q.QldpcError) as e:
            settle_host(q, 3, dict(b, key_bits=np.array([kb], np.int32)))
        assert e.value.status == -6 and "key_bits" in str(e.value)
    with pytest.raises(q.QldpcError) as e:                                         # key rows wider than the trial rows
        settle_host(q, 3, dict(b, keys=np.zeros((1, 5), np.uint32)))
    assert e.value.status == -6
    L, one = q._L, C.c_void_p(64)
    up, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    u, i = (C.c_uint32 * 64)(), (C.c_int * 64)()
    args = [C.cast(u, up), C.cast(i, ip), C.cast(i, ip), C.cast(u, up), C.cast(i, ip), C.cast(u, up), C.cast(i, ip), C.cast(i, ip), C.cast(u, up), C.cast(u, up),
            C.cast(i, ip), C.cast(i, ip)]
    for missing in range(12):
        assert L.qldpc_recon_guess_settle_host(3, 1, 2, 4, *[None if k == missing else a for k, a in enumerate(args)]) == -1, missing
        assert L.qldpc_recon_guess_settle_dev(3, 1, 2, 4, *[None if k == missing else one for k in range(12)], None) == -1, missing
    for g, n, Wk, Wn in [(-1, 1, 2, 4), (11, 1, 2, 4), (3, -1, 2, 4), (3, 1, 0, 4), (3, 1, 5, 4), (10, (1 << 14) + 1, 2, 4)]:
        assert L.qldpc_recon_guess_settle_dev(g, n, Wk, Wn, *[one] * 12, None) == -6, (g, n, Wk, Wn)      # refused before the device is touched
    assert L.qldpc_recon_guess_settle_dev(3, 0, 2, 4, *[one] * 12, None) == 0      # no source queues nothing
    assert q.RECON_GUESS_DTYPE.itemsize == 24 and q.RECON_GUESS_DTYPE.names == R.FIELDS
    # the session call refuses a missing session before anything else
    assert L.qldpc_recon_decode_guess(None, 1, None, None, None, None, None, 3, None, None, None, None) == -1


def test_host_code_under_asan_ubsan(tmp_path):
    """the mirror over made-up sources against a bit-by-bit restatement in C, in buffers of exactly the sizes the call names, as a stand-alone program
    (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "recon_guess_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "recon_guess_sanitize.c"),
                           os.path.join(csrc, "qldpc_recon_guess_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr

"""Batched privacy amplification (qldpc_privamp_blocks*): the hash through the 32-bit key functional, bit-exact vs the oracle and vs the
one-block kernel.  The CPU tests run the host mirrors of the two halves (the same fold / expansion code the kernel is built from)."""
import ctypes as C
import json
import os
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_WORKBITS = (1, 31, 32, 33, 63, 64, 65, 1000, 4097)
SEEDS = (1, 0x80000000, 0xffffffff, 0xdeadbeef)


def _key(q, rng, workbits):
    key = q.pack_bits(rng.integers(0, 2, workbits))
    key[-1] |= np.uint32((1 << ((-workbits) % 32)) - 1)          # garbage past workbits must be ignored (priv_amp.c:196-198)
    return key


# ---- CPU: the two halves on the host -------------------------------------------------------------

@pytest.mark.parametrize("workbits", EDGE_WORKBITS)
def test_host_halves_equal_the_oracle(q, O, workbits):
    rng = np.random.default_rng(workbits)
    key = _key(q, rng, workbits)
    for seed in SEEDS:
        fb = int(rng.integers(1, 400))
        ref = O.privamp(key, workbits, seed, fb)
        for lanes in (1, 2, 8, 64, 256):
            v = q.privamp_key_functional(key, workbits, lanes)
            assert (q.privamp_expand_host(v, workbits, seed, fb) == ref).all(), (workbits, seed, fb, lanes)


def test_key_fold_is_chunk_invariant(q):
    rng = np.random.default_rng(20000)
    key = _key(q, rng, 20000)
    vals = {q.privamp_key_functional(key, 20000, lanes) for lanes in (1, 2, 3, 8, 64, 100, 256, 625, 1000)}
    assert len(vals) == 1 and vals != {0}


def test_key_functional_is_linear_and_ignores_the_tail(q):
    rng = np.random.default_rng(3)
    for wb in (33, 1000, 20000):
        k1, k2 = _key(q, rng, wb), _key(q, rng, wb)
        f = q.privamp_key_functional
        assert f(k1 ^ k2, wb, 8) == f(k1, wb, 8) ^ f(k2, wb, 8)
        clean = k1.copy()
        clean[-1] &= np.uint32((0xFFFFFFFF << ((-wb) % 32)) & 0xFFFFFFFF)
        assert f(clean, wb, 1) == f(k1, wb, 1)


def test_host_mirror_argument_checks(q):
    with pytest.raises(q.QldpcError):
        q.privamp_key_functional(np.zeros(1, np.uint32), 64, 1)          # too few words
    with pytest.raises(q.QldpcError):
        q.privamp_expand_host(1, 0, 1, 10)
    assert q.privamp_expand_host(1, 32, 1, 0).size == 0


# ---- GPU ------------------------------------------------------------------------------------------

class _Batch:
    """the mixed batch of 37 blocks and its oracle answers, computed once"""

    def __init__(self, q, O):
        rng = np.random.default_rng(37)
        wbs = list(EDGE_WORKBITS) + [20000, 65535] + [int(x) for x in rng.integers(1, 30001, 26)]
        fixed_fb = [0, 1, 31, 32, 33, 63, 64, 65, 257]
        fbs = []
        for i, wb in enumerate(wbs):
            fbs.append(fixed_fb[i % 9] if i % 2 == 0 else int(rng.integers(0, min(wb, 3000) + 1)))
        assert len(wbs) == 37 and set(fixed_fb) <= set(fbs)
        assert sum(fb * ((wb + 31) // 32) for wb, fb in zip(wbs, fbs)) <= 2 * 10 ** 7
        self.workbits, self.final_bits = wbs, fbs
        self.seeds = [SEEDS[i % 4] if i < 12 else int(rng.integers(1, 1 << 32)) for i in range(37)]
        self.keys = [_key(q, rng, wb) for wb in wbs]
        self.ref = [O.privamp(k, wb, s, fb) for k, wb, s, fb in zip(self.keys, wbs, self.seeds, fbs)]


@pytest.fixture(scope="module")
def batch(q, O):
    return _Batch(q, O)


@pytest.fixture(scope="module")
def pa(q):
    return q.PrivAmp(max_blocks=40, max_key_bits=65536, max_final_bits=65536)


def _same(got, ref):
    return len(got) == len(ref) and all(g.shape == r.shape and (g == r).all() for g, r in zip(got, ref))


@pytest.mark.gpu
def test_mixed_batch_equals_the_oracle(q, pa, batch):
    got = pa.blocks(batch.keys, batch.workbits, batch.seeds, batch.final_bits)
    bad = [i for i in range(37) if not (got[i] == batch.ref[i]).all()]
    assert not bad, [(i, batch.workbits[i], batch.final_bits[i]) for i in bad]


@pytest.mark.gpu
def test_full_size_batch_equals_the_one_block_kernel(q):
    rng = np.random.default_rng(1)
    keys = [_key(q, rng, 56880) for _ in range(8)]
    seeds = [0xb0b80000 + 977 * i for i in range(8)]
    p = q.PrivAmp(max_blocks=8, max_key_bits=56880, max_final_bits=41935)
    got = p.blocks(keys, [56880] * 8, seeds, [41935] * 8)
    for i in range(8):
        assert (got[i] == q.privamp(keys[i], 56880, seeds[i], 41935)).all(), i


@pytest.mark.gpu
@pytest.mark.parametrize("workbits,final_bits", [(96, (1 << 17) + 77), (200000, 300), (600000, 64)])
def test_past_the_limits_of_the_one_block_call(q, O, workbits, final_bits):
    rng = np.random.default_rng(workbits)
    key = _key(q, rng, workbits) if workbits & 31 else q.pack_bits(rng.integers(0, 2, workbits))
    p = q.PrivAmp(max_blocks=2, max_key_bits=workbits, max_final_bits=final_bits)
    got = p.blocks([key], [workbits], [0xdeadbeef], [final_bits])
    assert (got[0] == O.privamp(key, workbits, 0xdeadbeef, final_bits)).all()


@pytest.mark.gpu
def test_device_form_strided_rows_on_a_side_stream(q, pa, batch):
    import torch
    n = 37
    kstride, ostride = 2048 + 5, (3000 + 31) // 32 + 3
    keys = np.full((n, kstride), 0x5A5A5A5A, np.uint32)
    for i, k in enumerate(batch.keys):
        keys[i, :k.size] = k
    keys_t = torch.from_numpy(keys.view(np.int32)).cuda()
    out_t = torch.from_numpy(np.full((n, ostride), 0xA5A5A5A5, np.uint32).view(np.int32)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r = pa.blocks_dev(keys_t, batch.workbits, batch.seeds, batch.final_bits, out_t=out_t, stream=s)
    s.synchronize()
    assert r is out_t
    out = out_t.cpu().numpy().view(np.uint32)
    assert 0 in batch.final_bits
    for i in range(n):
        ow = (batch.final_bits[i] + 31) // 32
        assert (out[i, :ow] == batch.ref[i]).all(), i
        assert (out[i, ow:] == 0xA5A5A5A5).all(), i              # exactly ceil(final_bits/32) words change; none for final_bits == 0
    # out_t=None on the current stream
    out2 = pa.blocks_dev(keys_t, batch.workbits, batch.seeds, batch.final_bits)
    torch.cuda.synchronize()
    out2 = out2.cpu().numpy().view(np.uint32)
    assert all((out2[i, :batch.ref[i].size] == batch.ref[i]).all() for i in range(n))


@pytest.mark.gpu
def test_one_context_reused_for_other_shapes(q, O, pa, batch):
    bytes0 = pa.device_bytes
    assert bytes0 > 0
    rng = np.random.default_rng(5)
    first = pa.blocks(batch.keys[:1], batch.workbits[:1], batch.seeds[:1], batch.final_bits[:1])
    whole = pa.blocks(batch.keys, batch.workbits, batch.seeds, batch.final_bits)
    wbs = [65536, 7, 12345, 640, 33]
    fbs = [100, 65536, 0, 640, 1]
    keys5 = [_key(q, rng, wb) if wb & 31 else q.pack_bits(rng.integers(0, 2, wb)) for wb in wbs]
    five = pa.blocks(keys5, wbs, [9, 8, 7, 6, 5], fbs)
    assert _same(five, [O.privamp(k, wb, s, fb) for k, wb, s, fb in zip(keys5, wbs, [9, 8, 7, 6, 5], fbs)])
    assert _same(pa.blocks(batch.keys[:1], batch.workbits[:1], batch.seeds[:1], batch.final_bits[:1]), first)
    assert _same(whole, batch.ref) and _same(pa.blocks(batch.keys, batch.workbits, batch.seeds, batch.final_bits), batch.ref)
    assert pa.blocks([], [], [], []) == []
    assert pa.device_bytes == bytes0


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(q):
    p = q.PrivAmp(max_blocks=5, max_key_bits=1000, max_final_bits=500)
    rng = np.random.default_rng(2)
    keys = [_key(q, rng, 1000) for _ in range(6)]

    def refused(n, wbs, fbs, text=None):
        out = [np.full(16, 0xA5A5A5A5, np.uint32) for _ in range(n)]
        with pytest.raises(q.QldpcError) as e:
            p.blocks(keys[:n], wbs, [1] * n, fbs, out=out)
        assert e.value.status in (-1, -6)
        assert all((o == 0xA5A5A5A5).all() for o in out)
        if text:
            assert text in str(e.value), str(e.value)

    refused(6, [1000] * 6, [100] * 6)                                 # n > max_blocks
    refused(2, [1000, 1001], [100, 100], "block 1")                   # over max_key_bits
    refused(2, [1000, 1000], [501, 100], "block 0")                   # over max_final_bits
    refused(5, [1000, 1000, 1000, 0, 1000], [100] * 5, "block 3")
    refused(3, [1000] * 3, [100, 100, -1], "block 2")
    # NULL pointers, straight through the C ABI
    up, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    wb, sd, fb = np.full(2, 1000, np.int32), np.ones(2, np.uint32), np.full(2, 100, np.int32)
    outs = [np.full(16, 0xA5A5A5A5, np.uint32) for _ in range(2)]
    kp = (up * 2)(keys[0].ctypes.data_as(up), None)
    op = (up * 2)(*[o.ctypes.data_as(up) for o in outs])
    args = (wb.ctypes.data_as(ip), sd.ctypes.data_as(up), fb.ctypes.data_as(ip))
    assert q._L.qldpc_privamp_blocks(p._h, 2, kp, *args, op) == -1
    assert b"block 1" in q._L.qldpc_last_error()
    assert q._L.qldpc_privamp_blocks(p._h, 2, None, *args, op) == -1
    assert q._L.qldpc_privamp_blocks(None, 2, kp, *args, op) == -1
    assert q._L.qldpc_privamp_blocks_dev(p._h, 2, None, 64, *args, None, 16, None) == -1
    assert all((o == 0xA5A5A5A5).all() for o in outs)
    assert q._L.qldpc_privamp_blocks(p._h, 0, None, None, None, None, None) == 0
    with pytest.raises(q.QldpcError):
        q.PrivAmp(max_blocks=0)
    # and the context still works
    assert (p.blocks(keys[:1], [1000], [7], [500])[0] == q.privamp(keys[0], 1000, 7, 500)).all()


@pytest.mark.gpu
def test_one_batch_call_beats_64_one_block_calls(q):
    rng = np.random.default_rng(64)
    keys = [q.pack_bits(rng.integers(0, 2, 56880)) for _ in range(64)]
    seeds = list(range(1, 65))
    p = q.PrivAmp(max_blocks=64, max_key_bits=56880, max_final_bits=41935)
    p.blocks(keys, [56880] * 64, seeds, [41935] * 64)               # warm-up of each
    q.privamp(keys[0], 56880, 1, 41935)
    t0 = time.perf_counter()
    got = p.blocks(keys, [56880] * 64, seeds, [41935] * 64)
    t_batch = time.perf_counter() - t0
    t0 = time.perf_counter()
    old = [q.privamp(keys[i], 56880, seeds[i], 41935) for i in range(64)]
    t_old = time.perf_counter() - t0
    print("64 blocks 56880 -> 41935 bits: one PrivAmp.blocks call %.3f ms, 64 privamp calls %.3f ms" % (t_batch * 1e3, t_old * 1e3))
    assert _same(got, old)
    assert t_batch < t_old


@pytest.mark.gpu
def test_stream_harness_hash_stage(q):
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    assert os.path.exists(exe), "qldpc_stream is not built (build() makes it)"
    new = ("pa_ms_mean", "pa_ms_best", "distill_Mbit_s_mean")
    base = [exe, "-e", "64", "-k", "20000", "-b", "64", "-r", "1"]
    r = subprocess.run(base + ["-H"], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stdout[-1500:] + r.stderr[-1500:]      # 3: an epoch was not reconciled, which is the decoder's matter; it is not hashed
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(k in d for k in new) and d["pa_ms_mean"] > 0 and d["pa_ms_best"] > 0 and d["distill_Mbit_s_mean"] > 0
    assert d["reconciled"] >= 60
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stdout[-1500:] + r.stderr[-1500:]
    d0 = json.loads(r.stdout.strip().splitlines()[-1])
    assert not any(k in d0 for k in new)
    assert set(d) - set(d0) == set(new)

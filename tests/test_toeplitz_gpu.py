"""Toeplitz-hash privacy amplification on the device (qldpc_toeplitz_blocks*): every block against the numpy restatement of
y_i = XOR_{j < n} x_j t_(i+j), exact equality of words."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_N = (1, 31, 32, 33, 63, 64, 65, 1000, 4097)
EDGE_M = (1, 31, 32, 33, 63, 64, 65, 257)
FILL = 0xA5A5A5A5


def ref_words(q, x, t):
    """the reference of every test here: y = np.correlate(t, x, "valid") & 1, packed MSB-first"""
    if t.size < x.size:
        return np.zeros(0, np.uint32)
    return q.pack_bits((np.correlate(t.astype(np.int64), x.astype(np.int64), "valid") & 1).astype(np.uint8))


def key_words(q, x):
    key = q.pack_bits(x)
    key[-1] |= np.uint32((1 << ((-x.size) % 32)) - 1)               # garbage past key_bits must be ignored
    return key


class _Batch:
    """the mixed batch of 37 blocks, with a seed per block and with one seed for all, and the reference answers of both, computed once"""

    def __init__(self, q):
        rng = np.random.default_rng(37)
        ns = list(EDGE_N) + [20000, 65535] + [int(v) for v in rng.integers(1, 30001, 26)]
        fixed = [0] + list(EDGE_M)
        ms = []
        for i, n in enumerate(ns):
            ms.append(fixed[i % 9] if i % 2 == 0 else int(rng.integers(0, 801)))
        ms[9], ms[10] = 3000, 3000                                # (20 000, 3 000) and (65 535, 3 000)
        ms[11], ms[13] = 1, 257                                   # the edge out_bits the even slots did not reach
        assert len(ns) == 37 and set(fixed) <= set(ms) and (20000, 3000) in zip(ns, ms) and (65535, 3000) in zip(ns, ms)
        assert sum(n * m for n, m in zip(ns, ms)) <= 6.4e8
        self.key_bits, self.out_bits = ns, ms
        self.x = [rng.integers(0, 2, n) for n in ns]
        self.keys = [key_words(q, x) for x in self.x]
        self.t = [rng.integers(0, 2, max(n + m - 1, 1)) for n, m in zip(ns, ms)]
        self.seeds = [q.pack_bits(t) for t in self.t]
        for s, n, m in zip(self.seeds, ns, ms):
            if m:
                s[-1] |= np.uint32((1 << ((-(n + m - 1)) % 32)) - 1)        # and past key_bits + out_bits - 1
        self.ref = [ref_words(q, x, t[:n + m - 1]) if m else np.zeros(0, np.uint32) for x, t, n, m in zip(self.x, self.t, ns, ms)]
        self.t_one = rng.integers(0, 2, max(n + m - 1 for n, m in zip(ns, ms)))
        self.seed_one = q.pack_bits(self.t_one)
        self.ref_one = [ref_words(q, x, self.t_one[:n + m - 1]) if m else np.zeros(0, np.uint32) for x, n, m in zip(self.x, ns, ms)]


@pytest.fixture(scope="module")
def batch(q):
    return _Batch(q)


@pytest.fixture(scope="module")
def tz(q):
    return q.Toeplitz(max_blocks=40, max_key_bits=65536, max_out_bits=65536)


def _same(got, ref):
    return len(got) == len(ref) and all(g.shape == r.shape and (g == r).all() for g, r in zip(got, ref))


def _bad(batch, got, ref):
    return [(i, batch.key_bits[i], batch.out_bits[i]) for i in range(37) if got[i].shape != ref[i].shape or not (got[i] == ref[i]).all()]


@pytest.mark.gpu
def test_mixed_batch_with_a_seed_per_block(q, tz, batch):
    got = tz.blocks(batch.keys, batch.key_bits, batch.seeds, batch.out_bits)
    assert not _bad(batch, got, batch.ref)


@pytest.mark.gpu
def test_mixed_batch_with_one_shared_seed(q, tz, batch):
    got = tz.blocks(batch.keys, batch.key_bits, [batch.seed_one] * 37, batch.out_bits)       # all pointers equal
    assert not _bad(batch, got, batch.ref_one)
    assert not _bad(batch, tz.blocks(batch.keys, batch.key_bits, batch.seed_one, batch.out_bits), batch.ref_one)


@pytest.mark.gpu
def test_full_size_batch(q):
    n, m = 56880, 41935
    rng = np.random.default_rng(1)
    xs = [rng.integers(0, 2, n) for _ in range(8)]
    keys = [key_words(q, x) for x in xs]
    t = rng.integers(0, 2, n + m - 1)
    seed = q.pack_bits(t)
    p = q.Toeplitz(max_blocks=8, max_key_bits=n, max_out_bits=m)
    got = p.blocks(keys, [n] * 8, [seed] * 8, [m] * 8)
    for i in range(8):
        assert (got[i] == q.toeplitz_host(keys[i], n, seed, m)).all(), i
    assert (got[0] == ref_words(q, xs[0], t)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1500000, 64), (96, (1 << 17) + 77), (200000, 300)])
def test_past_one_seed_tile_and_past_one_output_chunk(q, n, m):
    rng = np.random.default_rng(n)
    x, t = rng.integers(0, 2, n), rng.integers(0, 2, n + m - 1)
    key = key_words(q, x) if n & 31 else q.pack_bits(x)
    p = q.Toeplitz(max_blocks=2, max_key_bits=n, max_out_bits=m)
    got = p.blocks([key], [n], [q.pack_bits(t)], [m])
    assert (got[0] == ref_words(q, x, t)).all()


def _device_rows(torch, rows, stride, fill):
    a = np.full((len(rows), stride), fill, np.uint32)
    for i, r in enumerate(rows):
        a[i, :r.size] = r
    return torch.from_numpy(a.view(np.int32)).cuda()


@pytest.mark.gpu
def test_device_form_strided_rows_on_a_side_stream(q, tz, batch):
    import torch
    n = 37
    kstride, sstride, ostride = 2048 + 5, (65535 + 3000 - 1 + 31) // 32 + 7, (3000 + 31) // 32 + 3
    keys_t = _device_rows(torch, batch.keys, kstride, 0x5A5A5A5A)
    seeds_t = _device_rows(torch, batch.seeds, sstride, 0x3C3C3C3C)
    one_t = torch.from_numpy(batch.seed_one.view(np.int32)).cuda()
    assert 0 in batch.out_bits

    def check(out_t, ref):
        out = out_t.cpu().numpy().view(np.uint32)
        for i in range(n):
            ow = (batch.out_bits[i] + 31) // 32
            assert (out[i, :ow] == ref[i]).all(), i
            assert (out[i, ow:] == FILL).all(), i                 # exactly ceil(out_bits/32) words change; none for out_bits == 0

    s = torch.cuda.Stream()
    for shared, seeds, ref in ((False, seeds_t, batch.ref), (True, one_t, batch.ref_one)):          # seed_stride > 0 and seed_stride == 0
        out_t = torch.from_numpy(np.full((n, ostride), FILL, np.uint32).view(np.int32)).cuda()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            r = tz.blocks_dev(keys_t, batch.key_bits, seeds, batch.out_bits, seed_shared=shared, out_t=out_t, stream=s)
        s.synchronize()
        assert r is out_t
        check(out_t, ref)
    # out_t=None on the current stream
    out2 = tz.blocks_dev(keys_t, batch.key_bits, seeds_t, batch.out_bits)
    torch.cuda.synchronize()
    out2 = out2.cpu().numpy().view(np.uint32)
    assert all((out2[i, :batch.ref[i].size] == batch.ref[i]).all() for i in range(n))


@pytest.mark.gpu
def test_one_context_reused_for_other_shapes(q, tz, batch):
    bytes0 = tz.device_bytes
    assert bytes0 > 0
    rng = np.random.default_rng(5)
    first = tz.blocks(batch.keys[:1], batch.key_bits[:1], batch.seeds[:1], batch.out_bits[:1])
    whole = tz.blocks(batch.keys, batch.key_bits, batch.seeds, batch.out_bits)
    ns = [65536, 7, 12345, 640, 33]
    ms = [100, 65536, 0, 640, 1]
    xs = [rng.integers(0, 2, n) for n in ns]
    ts = [rng.integers(0, 2, max(n + m - 1, 1)) for n, m in zip(ns, ms)]
    keys5 = [key_words(q, x) if x.size & 31 else q.pack_bits(x) for x in xs]
    five = tz.blocks(keys5, ns, [q.pack_bits(t) for t in ts], ms)
    assert _same(five, [ref_words(q, x, t) if m else np.zeros(0, np.uint32) for x, t, m in zip(xs, ts, ms)])
    assert _same(tz.blocks(batch.keys[:1], batch.key_bits[:1], batch.seeds[:1], batch.out_bits[:1]), first)
    assert _same(whole, batch.ref) and _same(tz.blocks(batch.keys, batch.key_bits, batch.seeds, batch.out_bits), batch.ref)
    assert tz.blocks([], [], [], []) == []
    assert tz.device_bytes == bytes0


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(q):
    p = q.Toeplitz(max_blocks=5, max_key_bits=1000, max_out_bits=500)
    rng = np.random.default_rng(2)
    xs = [rng.integers(0, 2, 1000) for _ in range(6)]
    keys = [q.pack_bits(x) for x in xs]
    t = rng.integers(0, 2, 1600)
    seed = q.pack_bits(t)

    def refused(n, kbs, obs, text=None):
        out = [np.full(16, FILL, np.uint32) for _ in range(n)]
        with pytest.raises(q.QldpcError) as e:
            p.blocks(keys[:n], kbs, [seed] * n, obs, out=out)
        assert e.value.status in (-1, -6)
        assert all((o == FILL).all() for o in out)
        if text:
            assert text in str(e.value), str(e.value)

    refused(6, [1000] * 6, [100] * 6)                                 # n > max_blocks
    refused(2, [1000, 1001], [100, 100], "block 1")                   # over max_key_bits
    refused(2, [1000, 1000], [501, 100], "block 0")                   # over max_out_bits
    refused(5, [1000, 1000, 1000, 0, 1000], [100] * 5, "block 3")
    refused(3, [1000] * 3, [100, 100, -1], "block 2")
    # NULL pointers, straight through the C ABI
    up, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    kb, ob = np.full(2, 1000, np.int32), np.full(2, 100, np.int32)
    outs = [np.full(16, FILL, np.uint32) for _ in range(2)]
    good_k = (up * 2)(*[k.ctypes.data_as(up) for k in keys[:2]])
    good_s = (up * 2)(seed.ctypes.data_as(up), seed.ctypes.data_as(up))
    good_o = (up * 2)(*[o.ctypes.data_as(up) for o in outs])
    kbp, obp = kb.ctypes.data_as(ip), ob.ctypes.data_as(ip)
    f = q._L.qldpc_toeplitz_blocks
    assert f(p._h, 2, (up * 2)(keys[0].ctypes.data_as(up), None), kbp, good_s, obp, good_o) == -1
    assert b"block 1" in q._L.qldpc_last_error() and b"key" in q._L.qldpc_last_error()
    assert f(p._h, 2, good_k, kbp, (up * 2)(None, seed.ctypes.data_as(up)), obp, good_o) == -1
    assert b"block 0" in q._L.qldpc_last_error() and b"seed" in q._L.qldpc_last_error()
    assert f(p._h, 2, good_k, kbp, good_s, obp, (up * 2)(outs[0].ctypes.data_as(up), None)) == -1
    assert b"block 1" in q._L.qldpc_last_error() and b"output" in q._L.qldpc_last_error()
    assert f(p._h, 2, None, kbp, good_s, obp, good_o) == -1
    assert f(None, 2, good_k, kbp, good_s, obp, good_o) == -1
    assert q._L.qldpc_toeplitz_blocks_dev(p._h, 2, None, 64, kbp, None, 0, obp, None, 16, None) == -1
    assert all((o == FILL).all() for o in outs)
    assert f(p._h, 0, None, None, None, None, None) == 0
    for bad in (dict(max_blocks=0), dict(max_blocks=65536), dict(max_blocks=65535, max_key_bits=1 << 24, max_out_bits=1 << 24)):
        with pytest.raises(q.QldpcError) as e:
            q.Toeplitz(**bad)
        assert e.value.status == -6
    # and the context still works
    assert (p.blocks(keys[:1], [1000], [seed], [500])[0] == ref_words(q, xs[0], t[:1499])).all()


@pytest.mark.gpu
def test_stream_harness_toeplitz_stage(q):
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    assert os.path.exists(exe), "qldpc_stream is not built (build() makes it)"
    new = ("tpa_ms_mean", "tpa_ms_best", "tdistill_Mbit_s_mean")
    old = ("pa_ms_mean", "pa_ms_best", "distill_Mbit_s_mean")
    base = [exe, "-e", "64", "-k", "20000", "-b", "64", "-r", "1"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode in (0, 3), r.stdout[-1500:] + r.stderr[-1500:]       # 3: an epoch was not reconciled, which is the decoder's matter; it is not hashed
        return json.loads(r.stdout.strip().splitlines()[-1])

    d = run(["-U"])
    assert all(k in d for k in new) and d["tpa_ms_mean"] > 0 and d["tpa_ms_best"] > 0 and d["tdistill_Mbit_s_mean"] > 0
    assert d["reconciled"] >= 60
    d0 = run([])
    assert not any(k in d0 for k in new + old)
    assert set(d) - set(d0) == set(new)
    both = run(["-H", "-U"])
    assert set(both) - set(d0) == set(new + old) and all(both[k] > 0 for k in new + old)

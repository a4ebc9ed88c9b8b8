"""The NTT method of the Toeplitz hash on the device (Toeplitz(method="ntt")): every block against the direct method's host mirror, a
direct context on the same inputs, or a closed form where the quadratic reference is out of reach; exact equality of words."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5A5A5A5
SMALL = 5
MAXN, MAXM = 70000, 50000


def key_words(q, x):
    key = q.pack_bits(x)
    key[-1] |= np.uint32((1 << ((-x.size) % 32)) - 1)               # garbage past key_bits must be ignored
    return key


class _Batch:
    """the mixed batch of 40 blocks, with a seed per block and with one seed for all, and the direct host mirror's answers to both, once"""

    def __init__(self, q):
        rng = np.random.default_rng(40)
        shapes = [(MAXN, MAXM), (56880, 41935), (1, 1), (1, MAXM), (MAXN, 1), (16, 17), (17, 17), (32, 1), (33, 32), (4097, 4096), (4096, 4097),
                  (65535, 2), (2, 33000), (31, 31)]
        while len(shapes) < 40:
            shapes.append((int(rng.integers(1, 30001)), int(rng.integers(1, 4001))))
        assert sum(n * m for n, m in shapes) < 1e10
        self.key_bits, self.out_bits = [n for n, _ in shapes], [m for _, m in shapes]
        self.n = len(shapes)
        self.lengths = len({q.toeplitz_ntt_length(n, m) for n, m in shapes})
        assert self.lengths >= 8
        self.keys = [key_words(q, rng.integers(0, 2, n)) for n in self.key_bits]
        self.seeds = [q.pack_bits(rng.integers(0, 2, n + m - 1)) for n, m in shapes]
        for s, (n, m) in zip(self.seeds, shapes):
            s[-1] |= np.uint32((1 << ((-(n + m - 1)) % 32)) - 1)    # and past key_bits + out_bits - 1
        self.seed_one = q.pack_bits(rng.integers(0, 2, max(n + m - 1 for n, m in shapes)))
        self.ref = [q.toeplitz_host(k, n, s, m) for k, s, (n, m) in zip(self.keys, self.seeds, shapes)]
        self.ref_one = [q.toeplitz_host(k, n, self.seed_one, m) for k, (n, m) in zip(self.keys, shapes)]


@pytest.fixture(scope="module")
def batch(q):
    return _Batch(q)


@pytest.fixture(scope="module")
def tz(q):
    return q.Toeplitz(max_blocks=40, max_key_bits=MAXN, max_out_bits=MAXM, method="ntt")


@pytest.fixture(scope="module")
def direct(q):
    return q.Toeplitz(max_blocks=40, max_key_bits=MAXN, max_out_bits=MAXM)


def _bad(batch, got, ref):
    return [(i, batch.key_bits[i], batch.out_bits[i]) for i in range(batch.n) if got[i].shape != ref[i].shape or not (got[i] == ref[i]).all()]


@pytest.mark.gpu
def test_mixed_batch_with_a_seed_per_block(q, tz, direct, batch):
    got = tz.blocks(batch.keys, batch.key_bits, batch.seeds, batch.out_bits)
    assert not _bad(batch, got, batch.ref)
    assert not _bad(batch, direct.blocks(batch.keys, batch.key_bits, batch.seeds, batch.out_bits), got)
    st = tz.stats()
    assert st["forward"] == 2 * batch.n and st["inverse"] == batch.n and st["lengths"] == batch.lengths and st["largest_length"] == 1 << 17
    assert st["rounds"] == batch.lengths and st["launches"] >= 3 * batch.lengths
    assert direct.stats() == dict(launches=1, forward=0, inverse=0, rounds=0, lengths=0, largest_length=0)


@pytest.mark.gpu
def test_mixed_batch_with_one_shared_seed(q, tz, direct, batch):
    got = tz.blocks(batch.keys, batch.key_bits, [batch.seed_one] * batch.n, batch.out_bits)           # all pointers equal
    assert not _bad(batch, got, batch.ref_one)
    st = tz.stats()
    assert st["forward"] == batch.n + batch.lengths and st["inverse"] == batch.n and st["lengths"] == batch.lengths
    assert not _bad(batch, tz.blocks(batch.keys, batch.key_bits, batch.seed_one, batch.out_bits), batch.ref_one)
    assert not _bad(batch, direct.blocks(batch.keys, batch.key_bits, batch.seed_one, batch.out_bits), got)


@pytest.mark.gpu
def test_a_work_area_of_one_block_runs_the_batch_in_rounds(q, batch):
    one = 8 * q.toeplitz_ntt_length(MAXN, MAXM)
    p = q.Toeplitz(max_blocks=40, max_key_bits=MAXN, max_out_bits=MAXM, method="ntt", work_bytes=one)
    assert p.device_bytes >= one
    assert not _bad(batch, p.blocks(batch.keys, batch.key_bits, batch.seeds, batch.out_bits), batch.ref)
    st = p.stats()
    assert st["rounds"] > st["lengths"] == batch.lengths and st["forward"] == 2 * batch.n
    assert not _bad(batch, p.blocks(batch.keys, batch.key_bits, batch.seed_one, batch.out_bits), batch.ref_one)
    st = p.stats()
    assert st["rounds"] > batch.lengths and st["forward"] == batch.n + batch.lengths


# (pass_log2, n, m): the small instance at L = 2^5, 2^7, 2^10, 2^13, 2^15 (one pass, ragged two, two, ragged three, three); the production one
# at one tile (2^14), one bit past it, 2^17 and 2^20 (ragged two: 5 + 9, 6 + 9, 8 + 9; ragged three: 2 + 9 + 9)
STRUCTURES = [(SMALL, 16, 17), (SMALL, 100, 29), (SMALL, 1000, 25), (SMALL, 8000, 193), (SMALL, 30000, 2769),
              (0, 300, 213), (0, 16000, 385), (0, 16000, 386), (0, 56880, 41935), (0, 1048000, 577)]


@pytest.mark.gpu
@pytest.mark.parametrize("b,n,m", STRUCTURES)
def test_every_pass_structure(q, b, n, m):
    rng = np.random.default_rng(n + m)
    L = q.toeplitz_ntt_length(n, m)
    assert n + m - 1 <= L < 2 * (n + m - 1)
    key, seed = key_words(q, rng.integers(0, 2, n)), q.pack_bits(rng.integers(0, 2, n + m - 1))
    p = q.Toeplitz(max_blocks=2, max_key_bits=n, max_out_bits=m, method="ntt", pass_log2=b)
    got = p.blocks([key, key], [n, n], [seed, seed], [m, m])
    ref = q.toeplitz_host(key, n, seed, m)
    assert (got[0] == ref).all() and (got[1] == ref).all()
    B = b if b else q.TOEPLITZ_PASS_LOG2
    passes = -(-(L.bit_length() - 1) // B)
    assert p.stats() == dict(launches=3 * passes, forward=3, inverse=2, rounds=1, lengths=1, largest_length=L)


@pytest.mark.gpu
def test_long_blocks_equal_the_direct_context(q):
    rng = np.random.default_rng(15)
    for n, m in ((1500000, 200000), (524288, 524288)):
        key, seed = key_words(q, rng.integers(0, 2, n)), q.pack_bits(rng.integers(0, 2, n + m - 1))
        got = q.Toeplitz(max_blocks=1, max_key_bits=n, max_out_bits=m, method="ntt").blocks([key], [n], [seed], [m])[0]
        ref = q.Toeplitz(max_blocks=1, max_key_bits=n, max_out_bits=m).blocks([key], [n], [seed], [m])[0]
        assert got.shape == ref.shape and (got == ref).all(), (n, m)


@pytest.mark.gpu
def test_full_size_against_closed_forms(q):
    """n = m = 2^24, L = 2^25, every production pass.  An all-ones key gives c_i = S[i + n] - S[i], the largest counts there are; a key
    of five bits gives the XOR of five windows of the seed"""
    n = m = 1 << 24
    rng = np.random.default_rng(24)
    seed = rng.integers(0, 1 << 32, (n + m - 1 + 31) // 32, dtype=np.uint32)
    t = np.unpackbits(seed.view(np.uint8).reshape(-1, 4)[:, ::-1].reshape(-1))           # MSB-first bits of the words
    assert t.size == 1 << 25 and t[0] == int(seed[0]) >> 31
    p = q.Toeplitz(max_blocks=1, max_key_bits=n, max_out_bits=m, method="ntt")
    assert q.toeplitz_ntt_length(n, m) == 1 << 25
    ones = p.blocks([np.full(n // 32, 0xFFFFFFFF, np.uint32)], [n], [seed], [m])[0]
    S = np.concatenate([[0], np.cumsum(t, dtype=np.int64)])
    assert int((S[n:n + m] - S[:m]).max()) > n // 2
    ref = np.packbits(((S[n:n + m] - S[:m]) & 1).astype(np.uint8)).view(">u4").astype(np.uint32)
    assert ones.shape == ref.shape and (ones == ref).all()
    assert p.stats() == dict(launches=9, forward=2, inverse=1, rounds=1, lengths=1, largest_length=1 << 25)
    x = np.zeros(n, np.uint8)
    x[[0, 1, 31, 32, n - 1]] = 1
    five = p.blocks([np.packbits(x).view(">u4").astype(np.uint32)], [n], [seed], [m])[0]
    t = np.concatenate([t, [0]])
    y = t[0:m] ^ t[1:m + 1] ^ t[31:m + 31] ^ t[32:m + 32] ^ t[n - 1:n - 1 + m]
    assert (five == np.packbits(y).view(">u4").astype(np.uint32)).all()


def _device_rows(torch, rows, stride, fill):
    a = np.full((len(rows), stride), fill, np.uint32)
    for i, r in enumerate(rows):
        a[i, :r.size] = r
    return torch.from_numpy(a.view(np.int32)).cuda()


@pytest.mark.gpu
def test_device_form_strided_rows_on_a_side_stream(q, tz, batch):
    import torch
    n = batch.n
    kstride, sstride, ostride = (MAXN + 31) // 32 + 5, (MAXN + MAXM - 1 + 31) // 32 + 7, (MAXM + 31) // 32 + 3
    keys_t = _device_rows(torch, batch.keys, kstride, 0x5A5A5A5A)
    seeds_t = _device_rows(torch, batch.seeds, sstride, 0x3C3C3C3C)
    one_t = torch.from_numpy(batch.seed_one.view(np.int32)).cuda()

    def check(out_t, ref):
        out = out_t.cpu().numpy().view(np.uint32)
        for i in range(n):
            ow = (batch.out_bits[i] + 31) // 32
            assert (out[i, :ow] == ref[i]).all(), i
            assert (out[i, ow:] == FILL).all(), i                 # exactly ceil(out_bits/32) words change

    s = torch.cuda.Stream()
    for shared, seeds, ref in ((False, seeds_t, batch.ref), (True, one_t, batch.ref_one)):          # seed_stride > 0 and seed_stride == 0
        out_t = torch.from_numpy(np.full((n, ostride), FILL, np.uint32).view(np.int32)).cuda()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            r = tz.blocks_dev(keys_t, batch.key_bits, seeds, batch.out_bits, seed_shared=shared, out_t=out_t, stream=s)
        s.synchronize()
        assert r is out_t
        check(out_t, ref)
        assert tz.stats()["forward"] == (n + batch.lengths if shared else 2 * n)
    out2 = tz.blocks_dev(keys_t, batch.key_bits, seeds_t, batch.out_bits)                            # out_t=None on the current stream
    torch.cuda.synchronize()
    out2 = out2.cpu().numpy().view(np.uint32)
    assert all((out2[i, :batch.ref[i].size] == batch.ref[i]).all() for i in range(n))


@pytest.mark.gpu
def test_one_context_reused_for_other_shapes(q, tz, batch):
    bytes0 = tz.device_bytes
    assert bytes0 >= 40 * 8 * (1 << 17)                           # the work area and the tables are counted
    rng = np.random.default_rng(5)
    first = tz.blocks(batch.keys[:1], batch.key_bits[:1], batch.seeds[:1], batch.out_bits[:1])
    ns = [MAXN, 7, 12345, 640, 33, 640]
    ms = [100, MAXM, 0, 640, 1, 640]
    xs = [rng.integers(0, 2, n) for n in ns]
    keys = [key_words(q, x) if x.size & 31 else q.pack_bits(x) for x in xs]
    seeds = [q.pack_bits(rng.integers(0, 2, max(n + m - 1, 1))) for n, m in zip(ns, ms)]
    got = tz.blocks(keys, ns, seeds, ms)
    assert all((g == q.toeplitz_host(k, n, s, m)).all() for g, k, n, s, m in zip(got, keys, ns, seeds, ms)) and got[2].size == 0
    assert tz.stats()["inverse"] == 5 and tz.stats()["lengths"] == 4                   # the block that asks for 0 bits takes no part
    again = tz.blocks(batch.keys[:1], batch.key_bits[:1], batch.seeds[:1], batch.out_bits[:1])
    assert (again[0] == first[0]).all() and (first[0] == batch.ref[0]).all()
    assert not _bad(batch, tz.blocks(batch.keys, batch.key_bits, batch.seeds, batch.out_bits), batch.ref)
    assert tz.blocks([], [], [], []) == []
    assert tz.blocks(keys[2:3], ns[2:3], seeds[2:3], ms[2:3])[0].size == 0
    assert tz.device_bytes == bytes0


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(q):
    p = q.Toeplitz(max_blocks=5, max_key_bits=1000, max_out_bits=500, method="ntt", pass_log2=SMALL)
    rng = np.random.default_rng(2)
    xs = [rng.integers(0, 2, 1000) for _ in range(6)]
    keys = [q.pack_bits(x) for x in xs]
    seed = q.pack_bits(rng.integers(0, 2, 1600))

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
    assert q._L.qldpc_toeplitz_blocks_dev(p._h, 2, None, 64, kbp, None, 0, obp, None, 16, None) == -1
    assert all((o == FILL).all() for o in outs)
    assert f(p._h, 0, None, None, None, None, None) == 0
    stats = (C.c_uint64 * 8)()
    assert q._L.qldpc_toeplitz_stats(None, stats) == -1 and q._L.qldpc_toeplitz_stats(p._h, None) == -1
    # the configuration: sizes as the direct method refuses them, a work area below one block, a pass size no instance has, a method nobody has
    one = 8 * q.toeplitz_ntt_length(1000, 500)
    for bad, status in ((dict(max_blocks=0), -6), (dict(max_blocks=65536), -6), (dict(max_blocks=65535, max_key_bits=1 << 24, max_out_bits=1 << 24), -6),
                        (dict(max_key_bits=1000, max_out_bits=500, work_bytes=one - 4), -6), (dict(work_bytes=1), -6),
                        (dict(pass_log2=6), -1), (dict(pass_log2=9), -1), (dict(pass_log2=-1), -1), (dict(pass_log2=1), -1)):
        with pytest.raises(q.QldpcError) as e:
            q.Toeplitz(method="ntt", **bad)
        assert e.value.status == status, bad
    with pytest.raises(q.QldpcError):
        q.Toeplitz(method="auto")
    with pytest.raises(q.QldpcError):
        q.Toeplitz(pass_log2=7)                                       # nor on a direct context
    cfg = q._ToeplitzCfg()
    q._L.qldpc_toeplitz_cfg_default(C.byref(cfg))
    assert (cfg.method, cfg.pass_log2, cfg.work_bytes, cfg.device) == (0, 0, 0, 0)
    cfg.method = 2
    h = C.c_void_p()
    assert q._L.qldpc_toeplitz_create_cfg(C.byref(cfg), C.byref(h)) == -1 and not h.value
    assert q._L.qldpc_toeplitz_create_cfg(None, C.byref(h)) == -1
    # a work area of exactly one block is enough, and the context still works
    ok = q.Toeplitz(max_blocks=5, max_key_bits=1000, max_out_bits=500, method="ntt", work_bytes=one)
    ref = q.toeplitz_host(keys[0], 1000, seed, 500)
    assert (ok.blocks(keys[:1], [1000], [seed], [500])[0] == ref).all()
    assert (p.blocks(keys[:1], [1000], [seed], [500])[0] == ref).all()


@pytest.mark.gpu
def test_stream_harness_ntt_stage_equals_the_direct_stage(q):
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    assert os.path.exists(exe), "qldpc_stream is not built (build() makes it)"
    r = subprocess.run([exe, "-e", "64", "-k", "20000", "-b", "64", "-r", "1", "-N"], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 3), r.stdout[-1500:] + r.stderr[-1500:]           # 3: an epoch was not reconciled, which is the decoder's matter; it is not hashed
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["tpa_method"] == "ntt" and d["tpa_equals_direct"] == 1 and len(d["tpa_checksum"]) == 16 and int(d["tpa_checksum"], 16) != 0xcbf29ce484222325
    assert d["tpa_ms_mean"] > 0 and d["tpa_ms_best"] > 0 and d["tdistill_Mbit_s_mean"] > 0 and d["reconciled"] >= 60

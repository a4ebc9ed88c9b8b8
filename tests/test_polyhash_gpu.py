"""GPU suite of the error-verification hash (qldpc_polyhash_*, qcrypto-ldpc_amd/csrc/qldpc_polyhash.hip).  The reference of every tag is
tests/polyhash_ref.py: the Horner loop of the definition in Python integers, or a closed form of it for the 2^24-bit block.  Equality is exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import polyhash_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5A5A5A5
P = R.P
TILES = [0, 1024]
MAX_BITS = 100000


def _words(rng, bits, ones=False):
    W = (bits + 31) // 32
    return np.full(W, 0xFFFFFFFF, np.uint32) if ones else rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)


@pytest.fixture(scope="module")
def edges():
    """the edge blocks (every other one all ones, the rest random with whatever lies in their tail bits), the edge keys, and the reference tag
    of every (block, key) pair: computed once and left as it is"""
    rng = np.random.default_rng(2061)
    bits = list(R.EDGE_BITS)
    words = [_words(rng, b, ones=i % 2 == 1) for i, b in enumerate(bits)]
    keys = R.edge_keys(rng)
    hk = [R.key_words(k) for k in keys]
    ref = {(i, j): R.tag(words[i], bits[i], hk[j]) for i in range(len(bits)) for j in range(len(keys))}
    return dict(bits=bits, words=words, keys=keys, hk=hk, ref=ref)


@pytest.fixture(scope="module")
def mixed(edges):
    """about 40 blocks for one call: the edges, three random lengths <= 30 000 and 65 535, each with n_keys <= 4 keys of its own"""
    rng = np.random.default_rng(2062)
    bits = list(edges["bits"]) + [int(b) for b in rng.integers(1, 30001, 3)] + [65535]
    words = list(edges["words"]) + [_words(rng, b) for b in bits[len(edges["bits"]):]]
    hk = [np.concatenate([edges["hk"][(i + q) % 8] for q in range(4)]) for i in range(len(bits))]
    ref = [R.tags(w, b, k) for w, b, k in zip(words, bits, hk)]
    shared = np.concatenate([R.key_words(int(rng.integers(1, 1 << 62))) for _ in range(4)])
    ref_shared = [R.tags(w, b, shared) for w, b in zip(words, bits)]
    return dict(bits=bits, words=words, hk=hk, ref=ref, shared=shared, ref_shared=ref_shared)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_edge_lengths_and_keys_one_block_at_a_time(q, edges, tile):
    """every edge length under every edge key with one key per block, then under 2, 3 and 4 keys (the edge keys in rotation)"""
    ctx = {r: q.PolyHash(max_blocks=1, max_key_bits=MAX_BITS, n_keys=r, tile_words=tile) for r in (1, 2, 3, 4)}
    for i, (b, w) in enumerate(zip(edges["bits"], edges["words"])):
        for j in range(8):
            got = ctx[1].blocks([w], [b], [edges["hk"][j]])[0]
            assert got.tolist() == edges["ref"][(i, j)].tolist(), (b, hex(edges["keys"][j]), tile)
        for r in (2, 3, 4):
            js = [(i + s) % 8 for s in range(r)]
            got = ctx[r].blocks([w], [b], [np.concatenate([edges["hk"][j] for j in js])])[0]
            assert got.tolist() == np.concatenate([edges["ref"][(i, j)] for j in js]).tolist(), (b, r, tile)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("n_keys", [1, 2, 3, 4])
def test_mixed_batch_in_one_call(q, mixed, n_keys, tile):
    """the edges, random lengths and 65 535 bits as ONE call (blocks of one, two, three and, with the small tile, up to 4 tiles side by side),
    with a key row per block and with one row shared by the call"""
    n = len(mixed["bits"])
    assert 38 <= n <= 42
    ph = q.PolyHash(max_blocks=n, max_key_bits=MAX_BITS, n_keys=n_keys, tile_words=tile)
    got = ph.blocks(mixed["words"], mixed["bits"], [k[:2 * n_keys] for k in mixed["hk"]])
    for i in range(n):
        assert got[i].size == 2 * n_keys and got[i].tolist() == mixed["ref"][i][:2 * n_keys].tolist(), (i, mixed["bits"][i])
    got = ph.blocks(mixed["words"], mixed["bits"], mixed["shared"][:2 * n_keys].copy())
    for i in range(n):
        assert got[i].tolist() == mixed["ref_shared"][i][:2 * n_keys].tolist(), (i, mixed["bits"][i])


def _device_rows(torch, rows, stride, mask_bits=None):
    """rows a stride apart, FILL in the padding and, with mask_bits, in the tail bits of every row"""
    a = np.full((len(rows), stride), FILL, np.uint32)
    for i, r in enumerate(rows):
        a[i, :r.size] = r
        if mask_bits is not None and mask_bits[i] % 32:
            keep = np.uint32((0xFFFFFFFF << (32 - mask_bits[i] % 32)) & 0xFFFFFFFF)
            a[i, r.size - 1] = (r[-1] & keep) | (np.uint32(FILL) & ~keep)
    return torch.from_numpy(a.view(np.int32)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_device_form_strided_rows_on_a_side_stream(q, mixed, tile):
    """strided rows with 0xA5A5A5A5 in the padding and the tail bits, a key row per block in the first call and one shared row in the second,
    which is queued straight behind the first on the same context; exactly 2 n_keys words of a tag row change, and they are the host form's"""
    import torch
    r, n = 2, len(mixed["bits"])
    ph = q.PolyHash(max_blocks=n, max_key_bits=MAX_BITS, n_keys=r, tile_words=tile)
    host = ph.blocks(mixed["words"], mixed["bits"], [k[:2 * r] for k in mixed["hk"]])
    host_shared = ph.blocks(mixed["words"], mixed["bits"], mixed["shared"][:2 * r].copy())
    stride = max(w.size for w in mixed["words"]) + 3
    keys_t = _device_rows(torch, mixed["words"], stride, mixed["bits"])
    hk_t = _device_rows(torch, [k[:2 * r] for k in mixed["hk"]], 2 * r + 1)
    shared_t = torch.from_numpy(mixed["shared"][:2 * r].copy().view(np.int32)).cuda()
    out1 = torch.from_numpy(np.full((n, 2 * r + 3), FILL, np.uint32).view(np.int32)).cuda()
    out2 = out1.clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    bytes0 = ph.device_bytes
    with torch.cuda.stream(side):
        ph.blocks_dev(keys_t, mixed["bits"], hk_t, out_t=out1, stream=side)
        ph.blocks_dev(keys_t, mixed["bits"], shared_t, key_shared=True, out_t=out2, stream=side)
    side.synchronize()
    for out, want, ref in ((out1, host, mixed["ref"]), (out2, host_shared, mixed["ref_shared"])):
        o = out.cpu().numpy().view(np.uint32)
        for i in range(n):
            assert o[i, :2 * r].tolist() == want[i].tolist() == ref[i][:2 * r].tolist(), (i, mixed["bits"][i])
            assert (o[i, 2 * r:] == FILL).all(), i
    assert ph.device_bytes == bytes0 > 0


@pytest.mark.gpu
@pytest.mark.parametrize("tile", TILES)
def test_one_block_of_2_to_the_24_bits_against_closed_forms(q, tile):
    """65 tiles of the production instance, 513 of the small one and the fold kernel over them: all zero (tag n k), all ones under k = p - 1
    and under a random key, a single one at bit 0 and at bit n - 1"""
    n = 1 << 24
    W = n // 32
    rng = np.random.default_rng(2063)
    k64 = int(rng.integers(1, 1 << 62))
    k, hk = R.key_of(k64 >> 32, k64), R.key_words(k64)
    ph = q.PolyHash(max_blocks=1, max_key_bits=n, tile_words=tile)
    zero, ones = np.zeros(W, np.uint32), np.full(W, 0xFFFFFFFF, np.uint32)
    first, last = zero.copy(), zero.copy()
    first[0], last[-1] = 0x80000000, 1
    cases = [("zero", zero, hk, R.closed_all_zero(n, k)), ("ones, k = p - 1", ones, R.key_words(P - 1), R.closed_all_ones(n, P - 1)),
             ("ones", ones, hk, R.closed_all_ones(n, k)), ("bit 0", first, hk, R.closed_single_bit(n, 0, k)), ("bit n - 1", last, hk, R.closed_single_bit(n, n - 1, k))]
    assert R.as_words(cases[1][3]).tolist() == [0x1FFFFFFF, 0xFEFFFFFF]
    for name, w, key, want in cases:
        assert ph.blocks([w], [n], [key])[0].tolist() == R.as_words(want).tolist(), (name, tile)


@pytest.mark.gpu
def test_one_flipped_bit_changes_the_tag(q):
    """a block of 4 097 bits under a fixed key and its 64 neighbours at distance one, the first and the last bit among them, in one call:
    every tag differs from the original's, on the reference first, so that no lucky key passes the test"""
    bits = 4097
    rng = np.random.default_rng(2064)
    w = _words(rng, bits)
    hk = np.array([0x0BADC0DE, 0x12345679], np.uint32)
    pos = sorted({0, bits - 1} | {int(x) for x in rng.choice(np.arange(1, bits - 1), 62, replace=False)})
    assert len(pos) == 64
    blocks = [w]
    for p in pos:
        f = w.copy()
        f[p // 32] ^= np.uint32(1 << (31 - p % 32))
        blocks.append(f)
    ref = [R.tag(b, bits, hk).tolist() for b in blocks]
    assert all(r != ref[0] for r in ref[1:])
    got = q.PolyHash(max_blocks=65, max_key_bits=bits).blocks(blocks, [bits] * 65, hk)
    assert [g.tolist() for g in got] == ref


@pytest.mark.gpu
def test_end_to_end_tags_of_decoded_frames(q, O, gold):
    """a layered NMS decode of 96 frames of PEGReg504x1008 at a QBER where the CPU oracle gets some frames right and some wrong (checked
    here); the decoder's packed output is tagged where it lies (fetch_packed -> blocks_dev) and compared with the tag of the sent word"""
    import torch
    alist = os.path.join(gold, "PEGReg504x1008.alist")
    code, og = q.Code.from_alist(alist), O.Graph.from_alist(alist)
    rng = np.random.default_rng(61)
    F, N = 96, 1008
    frames = np.where(rng.random((F, N)) < 0.07, -2.75, 2.75).astype(np.float32)      # the all-zero word through a BSC
    order, _, _ = code.layer_order()
    var, chk = og.edges()
    inv = np.empty(code.M, np.int32)
    inv[order] = np.arange(code.M, dtype=np.int32)
    newc = inv[chk]
    idx = np.argsort(newc, kind="stable")
    ogl = O.Graph.from_edges(code.N, code.M, var[idx], newc[idx])
    ref = O.decode(ogl, frames, "NMS", 0.75, 30, "hlayered", False, 1)
    right = ~(ref["hard"] != 0).any(axis=1)
    assert 8 <= int(right.sum()) <= F - 8                         # both kinds occur on the oracle
    dec = q.Decoder(code, N, 30, rule="NMS", rule_param=0.75, n_frames=F, schedule="hlayered", enable_syndrome=False)
    dec.load_llr(torch.from_numpy(frames).cuda())
    dec.run()
    packed = dec.fetch_packed()
    hk = np.array([0x13572468, 0x9ABCDEF1], np.uint32)
    ph = q.PolyHash(max_blocks=F, max_key_bits=N)
    tags = ph.blocks_dev(packed, [N] * F, torch.from_numpy(hk.view(np.int32)).cuda(), key_shared=True)
    torch.cuda.synchronize()
    tags = tags.cpu().numpy().view(np.uint32)
    sent = R.tag(np.zeros(32, np.uint32), N, hk).tolist()
    assert sent == ph.blocks([np.zeros(32, np.uint32)], [N], hk)[0].tolist()
    for f in range(F):
        want = R.tag(q.pack_bits(ref["hard"][f]), N, hk).tolist()
        assert (want == sent) == bool(right[f])                   # on the reference: a wrong word has another tag
        assert tags[f].tolist() == want, f
        assert (tags[f].tolist() == sent) == bool(right[f]), f


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(q):
    for bad in (dict(n_keys=0), dict(n_keys=5), dict(tile_words=512), dict(tile_words=-1), dict(tile_words=2048)):
        with pytest.raises(q.QldpcError) as e:
            q.PolyHash(max_blocks=4, max_key_bits=1000, **bad)
        assert e.value.status == -1, bad
    for bad in (dict(max_blocks=0), dict(max_blocks=65536), dict(max_key_bits=0), dict(max_key_bits=(1 << 24) + 1), dict(max_blocks=65535, max_key_bits=1 << 24)):
        with pytest.raises(q.QldpcError) as e:
            q.PolyHash(**bad)
        assert e.value.status == -6, bad
    rng = np.random.default_rng(2065)
    ph = q.PolyHash(max_blocks=5, max_key_bits=1000, n_keys=2)
    keys = [_words(rng, 1000) for _ in range(6)]
    hk = np.array([1, 2, 3, 4], np.uint32)

    def refused(n, kbs, text=None):
        out = [np.full(4, FILL, np.uint32) for _ in range(n)]
        with pytest.raises(q.QldpcError) as e:
            ph.blocks(keys[:n], kbs, [hk] * n, out=out)
        assert e.value.status in (-1, -6)
        assert all((o == FILL).all() for o in out)
        if text:
            assert text in str(e.value), str(e.value)

    refused(6, [1000] * 6)                                        # n > max_blocks
    refused(2, [1000, 1001], "block 1")                           # over max_key_bits
    refused(5, [1000, 1000, 1000, 0, 1000], "block 3")
    refused(3, [1000, 1000, -1], "block 2")
    # NULL pointers, straight through the C ABI
    up, ip = C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    kb = np.full(2, 1000, np.int32)
    outs = [np.full(4, FILL, np.uint32) for _ in range(2)]
    good_k = (up * 2)(*[k.ctypes.data_as(up) for k in keys[:2]])
    good_h = (up * 2)(hk.ctypes.data_as(up), hk.ctypes.data_as(up))
    good_o = (up * 2)(*[o.ctypes.data_as(up) for o in outs])
    kbp = kb.ctypes.data_as(ip)
    f, err = q._L.qldpc_polyhash_blocks, q._L.qldpc_last_error
    assert f(ph._h, 2, (up * 2)(keys[0].ctypes.data_as(up), None), kbp, good_h, good_o) == -1 and b"block 1" in err() and b"key" in err()
    assert f(ph._h, 2, good_k, kbp, (up * 2)(None, hk.ctypes.data_as(up)), good_o) == -1 and b"block 0" in err()
    assert f(ph._h, 2, good_k, kbp, good_h, (up * 2)(outs[0].ctypes.data_as(up), None)) == -1 and b"block 1" in err() and b"output" in err()
    assert f(ph._h, 2, None, kbp, good_h, good_o) == -1 and f(ph._h, 2, good_k, None, good_h, good_o) == -1
    assert f(None, 2, good_k, kbp, good_h, good_o) == -1
    assert q._L.qldpc_polyhash_blocks_dev(ph._h, 2, None, 64, kbp, None, 0, None, 4, None) == -1
    assert f(ph._h, 0, None, None, None, None) == 0
    assert all((o == FILL).all() for o in outs)
    # device rows shorter than their blocks: the key row, the hash-key row, the tag row
    import torch
    keys_t = torch.zeros((2, 32), dtype=torch.int32, device="cuda")
    hk_t = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    out_t = torch.from_numpy(np.full((2, 4), FILL, np.uint32).view(np.int32)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    g = q._L.qldpc_polyhash_blocks_dev
    assert g(ph._h, 2, keys_t.data_ptr(), 31, kbp, hk_t.data_ptr(), 4, out_t.data_ptr(), 4, s) == -6 and b"block 0" in err()
    assert g(ph._h, 2, keys_t.data_ptr(), 32, kbp, hk_t.data_ptr(), 3, out_t.data_ptr(), 4, s) == -6 and b"block 0" in err()
    assert g(ph._h, 2, keys_t.data_ptr(), 32, kbp, hk_t.data_ptr(), 4, out_t.data_ptr(), 3, s) == -6 and b"block 0" in err()
    with pytest.raises(q.QldpcError):
        ph.blocks_dev(keys_t[:, :31], [1000, 1000], hk_t, out_t=out_t)
    torch.cuda.synchronize()
    assert (out_t.cpu().numpy().view(np.uint32) == FILL).all()
    # and the context still works: the device, the mirror with the kernel's own lanes and tile, and the reference agree
    got = ph.blocks(keys[:1], [1000], [hk])[0]
    mirror = np.concatenate([q.polyhash_host(keys[0], 1000, hk[2 * i:2 * i + 2], q.POLYHASH_LANES, ph.tile_words) for i in range(2)])
    assert got.tolist() == mirror.tolist() == R.tags(keys[0], 1000, hk).tolist()


@pytest.mark.gpu
def test_stream_harness_verification_stage(q):
    """qldpc_stream -V on a small stream of blocks so short (1 000 bits) that the plan's efficiency leaves some of them unreconciled: the tags
    agree exactly on the reconciled blocks and differ exactly on the failed blocks whose words differ; without -V the JSON has none of the fields"""
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    assert os.path.exists(exe), "qldpc_stream is not built (build() makes it)"
    new = ("vt_ms_mean", "vt_ms_best", "vt_agree", "vt_failed_differ", "vt_failed_words_differ", "vt_equals_host", "vt_leak_bits")
    base = [exe, "-e", "24", "-k", "1000", "-b", "24", "-r", "1", "-q", "0.01:0.06"]

    def run(extra):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode in (0, 3), r.stdout[-1500:] + r.stderr[-1500:]      # 3: an epoch was not reconciled, which this stream is chosen for
        return json.loads(r.stdout.strip().splitlines()[-1])

    d = run(["-V"])
    assert all(k in d for k in new)
    assert d["epochs"] == 24 and 1 <= d["reconciled"] <= 23          # both kinds of block occur
    assert d["vt_equals_host"] == 1 and d["vt_agree"] == d["reconciled"] and d["vt_leak_bits"] == 61
    assert d["vt_failed_differ"] == d["vt_failed_words_differ"] and 1 <= d["vt_failed_differ"] <= 24 - d["reconciled"]
    assert d["vt_ms_mean"] > 0 and d["vt_ms_best"] > 0
    plain = run([])
    assert not any(k in plain for k in new) and plain["reconciled"] == d["reconciled"]

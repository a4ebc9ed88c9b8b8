"""The hashes of the post-processing chain: privacy amplification (qldpc_privamp*, qldpc_toeplitz_*) and error verification
(qldpc_polyhash_*), their batch contexts and host mirrors."""
import ctypes as C

import numpy as np

from ._lib import _L, _Handle, _chk, _create, _default, _ip, _sig, _torch, _up, _vp, QldpcError

_sig("qldpc_privamp", C.c_int, [C.c_int, _up, C.c_int, C.c_uint32, C.c_int, _up])
_sig("qldpc_privamp_dev", C.c_int, [_vp, C.c_int, C.c_uint32, C.c_int, _vp, _vp])
_sig("qldpc_privamp_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_privamp_free", None, [_vp])
_sig("qldpc_privamp_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_privamp_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _up, _ip, C.POINTER(_up)])
_sig("qldpc_privamp_blocks_dev", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _ip, _up, _ip, _vp, C.c_size_t, _vp])
_sig("qldpc_privamp_key_functional", C.c_uint32, [_up, C.c_int, C.c_int])
_sig("qldpc_privamp_expand_host", C.c_int, [C.c_uint32, C.c_int, C.c_uint32, C.c_int, _up])


def privamp(key_words, workbits, seed, final_bits, device=0):
    """privAmp_doPrivAmp's hash (priv_amp.c:213-218) on the GPU: -> ceil(final_bits/32) words, MSB-first."""
    kw = np.ascontiguousarray(key_words, dtype=np.uint32)
    out = np.zeros((int(final_bits) + 31) // 32, np.uint32)
    _chk(_L.qldpc_privamp(int(device), kw.ctypes.data_as(_up), int(workbits), int(seed) & 0xFFFFFFFF, int(final_bits),
                          out.ctypes.data_as(_up)), "privamp")
    return out


def privamp_key_functional(words, workbits, lanes=1):
    """v_key = XOR_j (A^T)^(j+1) key[j]: the 32 bits of the key the hash depends on, folded in `lanes` equal chunks (host mirror)"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    if int(workbits) <= 0 or w.size < (int(workbits) + 31) // 32 or int(lanes) < 1:
        raise QldpcError(-6, "privamp_key_functional: %d words, workbits = %d, lanes = %d" % (w.size, workbits, lanes))
    return int(_L.qldpc_privamp_key_functional(w.ctypes.data_as(_up), int(workbits), int(lanes)))


def privamp_expand_host(v, workbits, seed, final_bits):
    """final key bit i = parity(v & R^i seed), R = A^numwords (host mirror) -> ceil(final_bits/32) words, MSB-first"""
    out = np.zeros((max(int(final_bits), 0) + 31) // 32, np.uint32)
    _chk(_L.qldpc_privamp_expand_host(int(v) & 0xFFFFFFFF, int(workbits), int(seed) & 0xFFFFFFFF, int(final_bits), out.ctypes.data_as(_up)),
         "privamp_expand_host")
    return out


# ---- what the batch contexts of the hashes (PrivAmp, Toeplitz, PolyHash) do with the arguments of a call ---------------------------------

def _hb_words(bits):
    return [(b + 31) >> 5 if b > 0 else 0 for b in bits.tolist()]


def _hb_args(who, n, **arrays):
    """the per-block argument arrays of a call of n blocks: int32, `seeds` uint32 from any integers"""
    got = [(np.asarray(v, dtype=np.int64).ravel() & 0xFFFFFFFF).astype(np.uint32) if k == "seeds" else np.ascontiguousarray(v, dtype=np.int32).ravel()
           for k, v in arrays.items()]
    for a in got:
        if a.size != n:
            raise QldpcError(-6, "%s: %d blocks, %s" % (who, n, ", ".join("%d %s" % (a.size, k) for a, k in zip(got, arrays))))
    return got


def _hb_ptr(a, ctype):
    """an argument array as its pointer argument; from_buffer costs a third of data_as, which a call of one block notices"""
    return (ctype * a.size).from_buffer(a) if a.size and a.flags.writeable else a.ctypes.data_as(C.POINTER(ctype))


def _hb_rows(who, what, n, rows, need):
    """host rows as uint32 arrays (such an array stays the same object; what "out": the caller's as they are, or made here) of the words `need`, and their pointers"""
    if what == "out":
        rows = [np.zeros(w, np.uint32) for w in need] if rows is None else rows
    else:
        rows = [np.ascontiguousarray(r, dtype=np.uint32) for r in rows]
    for i, r in enumerate(rows):
        if r.dtype != np.uint32 or not r.flags.c_contiguous or r.size < need[i]:
            raise QldpcError(-6, "%s: %s[%d] must be a contiguous uint32 array of at least %d words" % (who, what, i, need[i]) if what == "out" else
                             "%s: block %d has %d %s words, needs %d" % (who, i, r.size, what, need[i]))
    return rows, (_up * max(n, 1))(*[r.ctypes.data_as(_up) for r in rows])


def _hb_dev_rows(torch, who, device, rows, stream):
    """the device rows of a call, rows = [(name, tensor, rows it must have, words each block needs, note)] with the output rows last (None: made
    here, as wide as the longest) -> (the output rows, the row stride of every tensor, the stream: torch's current one by default)"""
    if rows[-1][1] is None:
        name, _, n, need, note = rows[-1]
        rows[-1] = (name, torch.zeros((n, max(need, default=1) or 1), dtype=torch.int32, device=rows[0][1].device), n, need, note)
    strides = []
    for name, t, count, need, note in rows:
        if t.dtype != torch.int32 or t.dim() != 2 or t.stride(1) != 1 or not t.is_cuda or t.shape[0] != count:
            raise QldpcError(-6, "%s: %s must be a device int32 [n, stride] tensor with unit column stride%s" % (who, name, note))
        strides.append(int(t.stride(0)) if count > 1 else int(t.shape[1]))
    for name, t, count, need, note in rows:
        if t.device.index != device:
            raise QldpcError(-1, "%s: %s are on %s, the context is on device %d" % (who, " / ".join(r[0] for r in rows), " / ".join(str(r[1].device) for r in rows), device))
    # a row holds shape[1] words even where the rows lie further apart, so the library's row checks use the shape
    for name, t, count, need, note in rows:
        if need and max(need) > t.shape[1]:
            raise QldpcError(-6, "%s: block %d does not fit its rows" % (who, min(i for r in rows for i, w in enumerate(r[3]) if w > r[1].shape[1])))
    return rows[-1][1], strides, stream if stream is not None else torch.cuda.current_stream(device)


class PrivAmp(_Handle):
    """privAmp_doPrivAmp's hash for batches of blocks of any mix of lengths, one launch per call (qldpc_privamp_blocks*).
    Everything is allocated here; blocks() / blocks_dev() allocate nothing on the device."""
    _free = _L.qldpc_privamp_free

    def __init__(self, device=0, max_blocks=64, max_key_bits=1 << 16, max_final_bits=1 << 16):
        self._h = _create("PrivAmp", _L.qldpc_privamp_create, int(device), int(max_blocks), int(max_key_bits), int(max_final_bits))
        self.device, self.max_blocks, self.max_key_bits, self.max_final_bits = int(device), int(max_blocks), int(max_key_bits), int(max_final_bits)

    @property
    def device_bytes(self):
        return int(_L.qldpc_privamp_device_bytes(self._h))

    def blocks(self, keys, workbits, seeds, final_bits, out=None):
        """keys: list of uint32 word arrays (bits past workbits[i] are ignored) -> list of ceil(final_bits[i]/32)-word arrays.
        out: arrays to write into instead (a refused call leaves them untouched)"""
        n = len(keys)
        wb, sd, fb = _hb_args("PrivAmp", n, workbits=workbits, seeds=seeds, final_bits=final_bits)
        kws, kp = _hb_rows("PrivAmp.blocks", "key", n, keys, _hb_words(wb))
        out, op = _hb_rows("PrivAmp.blocks", "out", n, out, _hb_words(fb))
        _chk(_L.qldpc_privamp_blocks(self._h, n, kp, _hb_ptr(wb, C.c_int), _hb_ptr(sd, C.c_uint32), _hb_ptr(fb, C.c_int), op), "PrivAmp.blocks")
        return out

    def blocks_dev(self, keys_t, workbits, seeds, final_bits, out_t=None, stream=None):
        """keys_t: torch int32 [n, key_stride] on the device -> out_t int32 [n, out_stride] (row i: ceil(final_bits[i]/32) words written,
        the rest left as it is); asynchronous on `stream` (default: torch's current stream)"""
        n = int(keys_t.shape[0])
        wb, sd, fb = _hb_args("PrivAmp", n, workbits=workbits, seeds=seeds, final_bits=final_bits)
        out_t, (ks, os_), s = _hb_dev_rows(_torch(), "PrivAmp.blocks_dev", self.device,
                                           [("keys_t", keys_t, n, _hb_words(wb), ""), ("out_t", out_t, n, _hb_words(fb), "")], stream)
        _chk(_L.qldpc_privamp_blocks_dev(self._h, n, keys_t.data_ptr(), ks, _hb_ptr(wb, C.c_int), _hb_ptr(sd, C.c_uint32), _hb_ptr(fb, C.c_int),
                                         out_t.data_ptr(), os_, s.cuda_stream), "PrivAmp.blocks_dev")
        return out_t


# ---- Toeplitz-hash privacy amplification (qldpc_toeplitz_*): y_i = XOR_j x_j t_(i+j), the caller's seed of n + m - 1 bits ----------

class _ToeplitzCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("max_blocks", C.c_int), ("max_key_bits", C.c_int), ("max_out_bits", C.c_int),
                ("method", C.c_int), ("pass_log2", C.c_int), ("work_bytes", C.c_size_t)]


_sig("qldpc_toeplitz_seed_words", C.c_size_t, [C.c_int, C.c_int])
_sig("qldpc_toeplitz_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_toeplitz_free", None, [_vp])
_sig("qldpc_toeplitz_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_toeplitz_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, C.POINTER(_up), _ip, C.POINTER(_up)])
_sig("qldpc_toeplitz_blocks_dev", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _ip, _vp, C.c_size_t, _ip, _vp, C.c_size_t, _vp])
_sig("qldpc_toeplitz_host", C.c_int, [_up, C.c_int, _up, C.c_int, C.c_int, _up])
_sig("qldpc_toeplitz_cfg_default", None, [C.POINTER(_ToeplitzCfg)])
_sig("qldpc_toeplitz_create_cfg", C.c_int, [C.POINTER(_ToeplitzCfg), C.POINTER(_vp)])
_sig("qldpc_toeplitz_ntt_length", C.c_size_t, [C.c_int, C.c_int])
_sig("qldpc_toeplitz_stats", C.c_int, [_vp, C.POINTER(C.c_uint64)])
_sig("qldpc_toeplitz_ntt_host", C.c_int, [_up, C.c_int, _up, C.c_int, C.c_int, _up])
_sig("qldpc_toeplitz_ntt_mul_host", C.c_uint32, [C.c_uint32, C.c_uint32])
_sig("qldpc_toeplitz_ntt_root_host", C.c_uint32, [C.c_int])
TOEPLITZ_METHODS = {"direct": 0, "ntt": 1}
TOEPLITZ_NTT_PRIME = 2013265921
TOEPLITZ_PASS_LOG2, TOEPLITZ_PASS_LOG2_SMALL = 9, 5


def toeplitz_seed_words(key_bits, out_bits):
    """words of a seed of key_bits + out_bits - 1 bits; 0 for key_bits <= 0 or out_bits <= 0"""
    return int(_L.qldpc_toeplitz_seed_words(int(key_bits), int(out_bits)))


def _toeplitz_mirror(fn, who, key_words, key_bits, seed_words, out_bits, how):
    kw = np.ascontiguousarray(key_words, dtype=np.uint32)
    sw = np.ascontiguousarray(seed_words, dtype=np.uint32)
    key_bits, out_bits = int(key_bits), int(out_bits)
    if key_bits <= 0 or out_bits < 0 or kw.size < (key_bits + 31) // 32 or sw.size < toeplitz_seed_words(key_bits, out_bits):
        raise QldpcError(-6, "%s: %d key words, key_bits = %d, %d seed words, out_bits = %d" % (who, kw.size, key_bits, sw.size, out_bits))
    out = np.zeros((out_bits + 31) // 32, np.uint32)
    _chk(fn(kw.ctypes.data_as(_up), key_bits, sw.ctypes.data_as(_up), out_bits, int(how), out.ctypes.data_as(_up)), who)
    return out


def toeplitz_host(key_words, key_bits, seed_words, out_bits, tile_words=0):
    """y_i = XOR_{j < key_bits} x_j t_(i+j) on the host with the kernel's own window / fold functions, the key consumed in tiles of
    tile_words (0: the kernel's tile) -> ceil(out_bits/32) words, MSB-first"""
    return _toeplitz_mirror(_L.qldpc_toeplitz_host, "toeplitz_host", key_words, key_bits, seed_words, out_bits, tile_words)


def toeplitz_ntt_length(key_bits, out_bits):
    """the transform length L of the NTT method for a block: the smallest power of two >= key_bits + out_bits - 1, at least 32; 0 where
    toeplitz_seed_words gives 0"""
    return int(_L.qldpc_toeplitz_ntt_length(int(key_bits), int(out_bits)))


def toeplitz_ntt_mul(a, b):
    """a b mod TOEPLITZ_NTT_PRIME with the core header's Montgomery multiply"""
    return int(_L.qldpc_toeplitz_ntt_mul_host(int(a), int(b)))


def toeplitz_ntt_root(log2_len):
    """a primitive 2^log2_len-th root of unity mod TOEPLITZ_NTT_PRIME, log2_len 0 .. 25"""
    if not 0 <= int(log2_len) <= 25:
        raise QldpcError(-6, "toeplitz_ntt_root: log2_len = %d" % log2_len)
    return int(_L.qldpc_toeplitz_ntt_root_host(int(log2_len)))


def toeplitz_ntt_host(key_words, key_bits, seed_words, out_bits, pass_log2=0):
    """toeplitz_host by the NTT method on the host: the pass kernels' own functions over the same tiles, the transform in passes of
    pass_log2 index bits (0: the production kernels' 9; every value 1 .. 25 gives the same words)"""
    return _toeplitz_mirror(_L.qldpc_toeplitz_ntt_host, "toeplitz_ntt_host", key_words, key_bits, seed_words, out_bits, pass_log2)


class Toeplitz(_Handle):
    """Toeplitz hashing for batches of blocks of any mix of lengths, one launch per call (qldpc_toeplitz_blocks*).  The seeds are the
    caller's: key_bits + out_bits - 1 uniformly random bits per block, which may be public and shared by the blocks of a call.
    Everything is allocated here; blocks() / blocks_dev() allocate nothing on the device.  method "direct" is the n x m product;
    "ntt" gives the same words by three number-theoretic transforms per block, for long keys (pass_log2: 0 = the production pass kernels,
    TOEPLITZ_PASS_LOG2_SMALL = the small instance; work_bytes: the work area, 0 = the library's default).  Nothing picks the method for
    the caller."""
    _free = _L.qldpc_toeplitz_free

    def __init__(self, max_blocks=64, max_key_bits=1 << 16, max_out_bits=1 << 16, device=0, method="direct", pass_log2=0, work_bytes=0):
        if method not in TOEPLITZ_METHODS:
            raise QldpcError(-1, "Toeplitz: method %r (one of %s)" % (method, sorted(TOEPLITZ_METHODS)))
        if int(work_bytes) < 0:
            raise QldpcError(-6, "Toeplitz: work_bytes = %d" % work_bytes)
        cfg = _default(_ToeplitzCfg, _L.qldpc_toeplitz_cfg_default)
        cfg.device, cfg.max_blocks, cfg.max_key_bits, cfg.max_out_bits = int(device), int(max_blocks), int(max_key_bits), int(max_out_bits)
        cfg.method, cfg.pass_log2, cfg.work_bytes = TOEPLITZ_METHODS[method], int(pass_log2), int(work_bytes)
        self._h = _create("Toeplitz", _L.qldpc_toeplitz_create_cfg, C.byref(cfg))
        self.device, self.max_blocks, self.max_key_bits, self.max_out_bits = int(device), int(max_blocks), int(max_key_bits), int(max_out_bits)
        self.method = method

    def stats(self):
        """the last call: kernel launches, forward and inverse transforms, rounds, distinct transform lengths and the largest one (a
        direct context: one launch and zeros)"""
        v = (C.c_uint64 * 8)()
        _chk(_L.qldpc_toeplitz_stats(self._h, v), "Toeplitz.stats")
        return dict(launches=int(v[0]), forward=int(v[1]), inverse=int(v[2]), rounds=int(v[3]), lengths=int(v[4]), largest_length=int(v[5]))

    @property
    def device_bytes(self):
        return int(_L.qldpc_toeplitz_device_bytes(self._h))

    def blocks(self, keys, key_bits, seeds, out_bits, out=None):
        """keys, seeds: lists of uint32 word arrays (key bits past key_bits[i] and seed bits past key_bits[i] + out_bits[i] - 1 are
        ignored) -> list of ceil(out_bits[i]/32)-word arrays.  seeds may also be ONE array: it is uploaded once and shared by the blocks.
        out: arrays to write into instead (a refused call leaves them untouched)"""
        n = len(keys)
        kb, ob = _hb_args("Toeplitz", n, key_bits=key_bits, out_bits=out_bits)
        if isinstance(seeds, np.ndarray) and seeds.ndim == 1:
            seeds = [seeds] * n
        elif len(seeds) != n:
            raise QldpcError(-6, "Toeplitz.blocks: %d blocks, %d seeds" % (n, len(seeds)))
        if n > 0 and all(s is seeds[0] for s in seeds):           # one object: one row for the library, whatever it converts to
            seeds = [np.ascontiguousarray(seeds[0], dtype=np.uint32)] * n
        kws, kp = _hb_rows("Toeplitz.blocks", "key", n, keys, _hb_words(kb))
        sws, sp = _hb_rows("Toeplitz.blocks", "seed", n, seeds, [toeplitz_seed_words(k, o) for k, o in zip(kb.tolist(), ob.tolist())])
        out, op = _hb_rows("Toeplitz.blocks", "out", n, out, _hb_words(ob))
        _chk(_L.qldpc_toeplitz_blocks(self._h, n, kp, _hb_ptr(kb, C.c_int), sp, _hb_ptr(ob, C.c_int), op), "Toeplitz.blocks")
        return out

    def blocks_dev(self, keys_t, key_bits, seeds_t, out_bits, seed_shared=False, out_t=None, stream=None):
        """keys_t: torch int32 [n, key_stride] on the device; seeds_t: int32 [n, seed_stride], or with seed_shared a 1-D tensor or
        one row that every block reads -> out_t int32 [n, out_stride] (row i: ceil(out_bits[i]/32) words written, the rest left as it
        is); asynchronous on `stream` (default: torch's current stream)"""
        n = int(keys_t.shape[0])
        kb, ob = _hb_args("Toeplitz", n, key_bits=key_bits, out_bits=out_bits)
        if seed_shared and seeds_t.dim() == 1:
            seeds_t = seeds_t.unsqueeze(0)
        rows = [("keys_t", keys_t, n, _hb_words(kb), ""),
                ("seeds_t", seeds_t, 1 if seed_shared else n, [toeplitz_seed_words(k, o) for k, o in zip(kb.tolist(), ob.tolist())], " (one row with seed_shared)"),
                ("out_t", out_t, n, _hb_words(ob), "")]
        out_t, (ks, ss, os_), s = _hb_dev_rows(_torch(), "Toeplitz.blocks_dev", self.device, rows, stream)
        _chk(_L.qldpc_toeplitz_blocks_dev(self._h, n, keys_t.data_ptr(), ks, _hb_ptr(kb, C.c_int), seeds_t.data_ptr(), 0 if seed_shared else ss,
                                          _hb_ptr(ob, C.c_int), out_t.data_ptr(), os_, s.cuda_stream), "Toeplitz.blocks_dev")
        return out_t


# ---- error verification by a universal hash (qldpc_polyhash_*): tag = SUM_j c_j k^(W+1-j) mod 2^61 - 1, the caller's keys ---------------

class _PolyHashCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("max_blocks", C.c_int), ("max_key_bits", C.c_int), ("n_keys", C.c_int), ("tile_words", C.c_int)]


_sig("qldpc_polyhash_cfg_default", None, [C.POINTER(_PolyHashCfg)])
_sig("qldpc_polyhash_create_cfg", C.c_int, [C.POINTER(_PolyHashCfg), C.POINTER(_vp)])
_sig("qldpc_polyhash_free", None, [_vp])
_sig("qldpc_polyhash_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_polyhash_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, C.POINTER(_up), C.POINTER(_up)])
_sig("qldpc_polyhash_blocks_dev", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _ip, _vp, C.c_size_t, _vp, C.c_size_t, _vp])
_sig("qldpc_polyhash_bound_log2", C.c_double, [C.c_int, C.c_int])
_sig("qldpc_polyhash_leaked_bits", C.c_int, [C.c_int])
_sig("qldpc_polyhash_host", C.c_int, [_up, C.c_int, _up, C.c_int, C.c_int, _up])
_sig("qldpc_polyhash_mul_host", C.c_uint64, [C.c_uint64, C.c_uint64])
_sig("qldpc_polyhash_key_host", C.c_uint64, [C.c_uint32, C.c_uint32])
POLYHASH_PRIME = (1 << 61) - 1
POLYHASH_TILE_WORDS, POLYHASH_TILE_WORDS_SMALL = 8192, 1024
POLYHASH_LANES = 256


def polyhash_mul(a, b):
    """a b mod POLYHASH_PRIME with the core header's multiply, for any 64-bit a, b"""
    return int(_L.qldpc_polyhash_mul_host(int(a) & 0xFFFFFFFFFFFFFFFF, int(b) & 0xFFFFFFFFFFFFFFFF))


def polyhash_key(hi, lo):
    """the field element of a key's two words: ((hi << 32) | lo) & POLYHASH_PRIME, the prime itself taken as 0"""
    return int(_L.qldpc_polyhash_key_host(int(hi) & 0xFFFFFFFF, int(lo) & 0xFFFFFFFF))


def polyhash_bound_log2(key_bits, n_keys=1):
    """log2 of the probability bound that two different blocks of up to key_bits bits give equal tags: n_keys (log2(W + 2) - 61)"""
    if int(key_bits) <= 0 or not 1 <= int(n_keys) <= 4:
        raise QldpcError(-6, "polyhash_bound_log2: key_bits = %d, n_keys = %d" % (key_bits, n_keys))
    return float(_L.qldpc_polyhash_bound_log2(int(key_bits), int(n_keys)))


def polyhash_leaked_bits(n_keys=1):
    """bits of a block that its tag discloses at the most: 61 n_keys"""
    if not 1 <= int(n_keys) <= 4:
        raise QldpcError(-6, "polyhash_leaked_bits: n_keys = %d" % n_keys)
    return int(_L.qldpc_polyhash_leaked_bits(int(n_keys)))


def polyhash_host(key_words, key_bits, hash_key, lanes=POLYHASH_LANES, tile_words=0):
    """the tag of one block under one key (hash_key: its two words hi, lo) on the host, by the kernels' own decomposition with `lanes` lanes
    per workgroup and tiles of tile_words (0: the production tile) -> the tag's two words (hi, lo); every lanes >= 1 and either tile
    give the same tag"""
    kw = np.ascontiguousarray(key_words, dtype=np.uint32)
    hk = np.ascontiguousarray(hash_key, dtype=np.uint32)
    key_bits = int(key_bits)
    if key_bits <= 0 or kw.size < (key_bits + 31) // 32 or hk.size < 2:
        raise QldpcError(-6, "polyhash_host: %d key words, key_bits = %d, %d hash key words" % (kw.size, key_bits, hk.size))
    out = np.zeros(2, np.uint32)
    _chk(_L.qldpc_polyhash_host(kw.ctypes.data_as(_up), key_bits, hk.ctypes.data_as(_up), int(lanes), int(tile_words), out.ctypes.data_as(_up)), "polyhash_host")
    return out


class PolyHash(_Handle):
    """Error verification for batches of blocks of any mix of lengths, one launch per call (qldpc_polyhash_blocks*): polynomial evaluation
    over 2^61 - 1 with the length as a coefficient, n_keys independent keys per block.  The keys are the caller's: two uniformly random words
    (hi, lo) per key, chosen after the blocks are fixed; the blocks of a call may share them.  A tag is 2 n_keys words.  Everything is
    allocated here; blocks() / blocks_dev() allocate nothing on the device.  tile_words: 0 = the production tile,
    POLYHASH_TILE_WORDS_SMALL = the small instance; the tags do not depend on it."""
    _free = _L.qldpc_polyhash_free

    def __init__(self, max_blocks=64, max_key_bits=1 << 16, n_keys=1, device=0, tile_words=0):
        cfg = _default(_PolyHashCfg, _L.qldpc_polyhash_cfg_default)
        cfg.device, cfg.max_blocks, cfg.max_key_bits, cfg.n_keys, cfg.tile_words = int(device), int(max_blocks), int(max_key_bits), int(n_keys), int(tile_words)
        self._h = _create("PolyHash", _L.qldpc_polyhash_create_cfg, C.byref(cfg))
        self.device, self.max_blocks, self.max_key_bits, self.n_keys = int(device), int(max_blocks), int(max_key_bits), int(n_keys)
        self.tile_words = int(tile_words) or POLYHASH_TILE_WORDS

    @property
    def device_bytes(self):
        return int(_L.qldpc_polyhash_device_bytes(self._h))

    def blocks(self, keys, key_bits, hash_keys, out=None):
        """keys: list of uint32 word arrays (bits past key_bits[i] are ignored); hash_keys: list of arrays of 2 n_keys words (hi, lo per
        key), or ONE such array, uploaded once and shared by the blocks -> list of 2 n_keys-word tags.
        out: arrays to write into instead (a refused call leaves them untouched)"""
        n = len(keys)
        kb, = _hb_args("PolyHash", n, key_bits=key_bits)
        if isinstance(hash_keys, np.ndarray) and hash_keys.ndim == 1:
            hash_keys = [hash_keys] * n
        elif len(hash_keys) != n:
            raise QldpcError(-6, "PolyHash.blocks: %d blocks, %d hash keys" % (n, len(hash_keys)))
        if n > 0 and all(s is hash_keys[0] for s in hash_keys):     # one object: one row for the library, whatever it converts to
            hash_keys = [np.ascontiguousarray(hash_keys[0], dtype=np.uint32)] * n
        tag = [2 * self.n_keys] * n
        kws, kp = _hb_rows("PolyHash.blocks", "key", n, keys, _hb_words(kb))
        hws, hp = _hb_rows("PolyHash.blocks", "hash key", n, hash_keys, tag)
        out, op = _hb_rows("PolyHash.blocks", "out", n, out, tag)
        _chk(_L.qldpc_polyhash_blocks(self._h, n, kp, _hb_ptr(kb, C.c_int), hp, op), "PolyHash.blocks")
        return out

    def blocks_dev(self, keys_t, key_bits, hash_keys_t, key_shared=False, out_t=None, stream=None):
        """keys_t: torch int32 [n, key_stride] on the device; hash_keys_t: int32 [n, >= 2 n_keys], or with key_shared a 1-D tensor or one
        row that every block reads -> out_t int32 [n, tag_stride] (row i: 2 n_keys words written, the rest left as it is); asynchronous
        on `stream` (default: torch's current stream)"""
        n = int(keys_t.shape[0])
        kb, = _hb_args("PolyHash", n, key_bits=key_bits)
        if key_shared and hash_keys_t.dim() == 1:
            hash_keys_t = hash_keys_t.unsqueeze(0)
        tag = [2 * self.n_keys] * n
        rows = [("keys_t", keys_t, n, _hb_words(kb), ""),
                ("hash_keys_t", hash_keys_t, 1 if key_shared else n, tag, " (one row with key_shared)"),
                ("out_t", out_t, n, tag, "")]
        out_t, (ks, hs, os_), s = _hb_dev_rows(_torch(), "PolyHash.blocks_dev", self.device, rows, stream)
        _chk(_L.qldpc_polyhash_blocks_dev(self._h, n, keys_t.data_ptr(), ks, _hb_ptr(kb, C.c_int), hash_keys_t.data_ptr(), 0 if key_shared else hs,
                                          out_t.data_ptr(), os_, s.cuda_stream), "PolyHash.blocks_dev")
        return out_t

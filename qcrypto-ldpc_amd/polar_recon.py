"""Polar reconciliation sessions (qldpc_polar_recon_*): Alice's syndrome and CRC, Bob's prior, decode and verdict on the device around an existing
Polar or PolarList, the host mirrors of both calls, and the two building blocks (prior, verdict) on the device and on the host; incremental
freezing rounds on a ladder; SC-Flip trials for the blocks that failed (decode_flip, polar_flip_select) and their mirrors."""
import ctypes as C

import numpy as np

from ._lib import _L, _Handle, _chk, _create, _dev_empty, _dev_rows, _dev_vec, _ip, _ptr, _sig, _stream_arg, _torch, _up, _vp, QldpcError
from .polar import POLAR_I8, POLAR_LIST_MAX_LOG2N, POLAR_MAX_LOG2N, PolarList, _form, _messages, _rule, _words

POLAR_RECON_F32_PIN = float(1 << 24)      # the default pin with float messages; with int8 it is the context's maxq

_sig("qldpc_polar_recon_create", C.c_int, [_vp, _vp, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_int, C.POINTER(_vp)])
_sig("qldpc_polar_recon_free", None, [_vp])
_sig("qldpc_polar_recon_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_polar_recon_syndrome_words", C.c_int, [_vp])
_sig("qldpc_polar_recon_leaked_bits", C.c_int, [_vp])
_sig("qldpc_polar_recon_encode_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_recon_decode_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_recon_prior_dev", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_recon_verdict_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_recon_tables_host", C.c_int, [C.c_int, C.c_int, _ip, _up, _ip, _ip])
_sig("qldpc_polar_recon_encode_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_uint32, C.c_int, _up, _ip, _up, _up])
_sig("qldpc_polar_recon_decode_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_double, C.c_double,
                                               C.c_int, _up, _ip, _up, _up, _ip, _ip, _ip])
_sig("qldpc_polar_recon_prior_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _up, _ip, _up, _vp, _up])
_sig("qldpc_polar_recon_verdict_host", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, _up, _up, _ip, _up, _ip, _up, _ip, _ip])
_sig("qldpc_polar_recon_create_ladder", C.c_int, [_vp, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_int, C.c_int, _ip, C.POINTER(_vp)])
_sig("qldpc_polar_recon_extra_words", C.c_int, [_vp])
_sig("qldpc_polar_recon_encode_ladder_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_recon_decode_rounds", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _ip])
_sig("qldpc_polar_recon_encode_ladder_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_uint32, C.c_int, _ip, C.c_int, _up, _ip, _up, _up, _up])
_sig("qldpc_polar_recon_decode_rounds_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_int, _ip, C.c_int,
                                                      _up, _ip, _up, _up, _up, _ip, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip, _ip])
_sig("qldpc_polar_recon_ladder_extra_host", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double])
_sig("qldpc_polar_recon_create_flip", C.c_int, [_vp, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_int, C.c_int, _ip, C.c_int, C.POINTER(_vp)])
_sig("qldpc_polar_recon_max_flips", C.c_int, [_vp])
_sig("qldpc_polar_recon_decode_flip", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _ip])
_sig("qldpc_polar_flip_select_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, _vp])
_sig("qldpc_polar_flip_select_host", C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _up, _ip, _ip, C.c_int, _ip])
_sig("qldpc_polar_recon_decode_flip_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_double, C.c_double, C.c_int, _ip, C.c_int,
                                                    _up, _ip, _up, _up, _up, _ip, C.c_int, C.c_int, _ip, _ip, _ip, _ip, _ip])


def _levels(kind, maxq, prior, pin):
    """the defaults of the two levels: prior 1; pin maxq with int8 messages, 2^24 with floats"""
    return (1.0 if prior is None else float(prior)), ((float(maxq) if kind == POLAR_I8 else POLAR_RECON_F32_PIN) if pin is None else float(pin))


def _code(log2_n, info_pos, max_log2_n=POLAR_MAX_LOG2N):
    """-> n, N (1: a size the library will refuse), W, pos int32 [K]"""
    n = int(log2_n)
    return n, (1 << n) if 0 <= n <= max_log2_n else 1, _words(n), np.ascontiguousarray(info_pos, dtype=np.int32).ravel()


def _rows(who, a, cols, name, dtype=np.uint32):
    """a host array [blocks, cols] of words; None stays None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 2 or a.shape[1] != cols:
        raise QldpcError(-6, "%s: %s must be [blocks, %d]" % (who, name, cols))
    return a


def _vec(who, a, n, name, dtype):
    """a host vector of n entries; None stays None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype).ravel()
    if a.size != n:
        raise QldpcError(-6, "%s: %s must hold %d entries" % (who, name, n))
    return a


def polar_recon_tables(log2_n, info_pos):
    """the tables of a code (qldpc_polar_recon_tables_host) -> frozen_mask uint32 [W] (1 = frozen), frozen_prefix int32 [W] (the frozen positions
    before each word), frozen_pos int32 [N - K] ascending"""
    n, N, W, pos = _code(log2_n, info_pos)
    mask, prefix, fpos = np.zeros(W, np.uint32), np.zeros(W, np.int32), np.zeros(max(N - pos.size, 1), np.int32)
    _chk(_L.qldpc_polar_recon_tables_host(n, pos.size, pos.ctypes.data_as(_ip), mask.ctypes.data_as(_up), prefix.ctypes.data_as(_ip), fpos.ctypes.data_as(_ip)),
         "polar_recon_tables")
    return mask, prefix, fpos[:max(N - pos.size, 0)].copy()


def polar_recon_encode_host(log2_n, info_pos, keys, key_bits=None, crc_len=0, crc_poly=0):
    """Alice's mirror (qldpc_polar_recon_encode_host): keys uint32 [B, W], key_bits int32 [B] or None (every block is N bits)
    -> (syndrome uint32 [B, ceil((N - K) / 32)], crc uint32 [B])"""
    who = "polar_recon_encode_host"
    n, N, W, pos = _code(log2_n, info_pos)
    keys = _rows(who, keys, W, "keys")
    B = keys.shape[0]
    kb = _vec(who, key_bits, B, "key_bits", np.int32)
    syn, crc = np.zeros((B, (max(N - pos.size, 0) + 31) // 32), np.uint32), np.zeros(B, np.uint32)
    _chk(_L.qldpc_polar_recon_encode_host(n, pos.size, pos.ctypes.data_as(_ip), int(crc_len), int(crc_poly) & 0xffffffff, B, keys.ctypes.data_as(_up), _ptr(kb, _ip),
                                          syn.ctypes.data_as(_up), crc.ctypes.data_as(_up)), who)
    return syn, crc


def polar_recon_decode_host(log2_n, info_pos, keys, syndrome, crc, key_bits=None, messages="i8", maxq=31, form="lanes", rule="sc", list_size=0, crc_len=0,
                            crc_poly=0, prior=None, pin=None, want_pick=False):
    """Bob's mirror (qldpc_polar_recon_decode_host): the prior mirror, the host decoder that (form, rule, list_size) name (list_size 0: SC) and the
    verdict mirror -> dict(keys uint32 [B, W] corrected where OK (a copy), status int32 [B], corrected int32 [B] and, with want_pick, pick int32 [B])"""
    who = "polar_recon_decode_host"
    kind, _ = _messages(messages)
    n, N, W, pos = _code(log2_n, info_pos, POLAR_LIST_MAX_LOG2N if list_size else POLAR_MAX_LOG2N)
    keys = _rows(who, keys, W, "keys").copy()
    B = keys.shape[0]
    syn = _rows(who, syndrome, (max(N - pos.size, 0) + 31) // 32, "syndrome")
    cr, kb = _vec(who, crc, B, "crc", np.uint32), _vec(who, key_bits, B, "key_bits", np.int32)
    p, q = _levels(kind, maxq, prior, pin)
    out = dict(keys=keys, status=np.zeros(B, np.int32), corrected=np.zeros(B, np.int32))
    if want_pick:
        out["pick"] = np.zeros(B, np.int32)
    _chk(_L.qldpc_polar_recon_decode_host(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), _form(form), _rule(rule), int(list_size), int(crc_len),
                                          int(crc_poly) & 0xffffffff, p, q, B, keys.ctypes.data_as(_up), _ptr(kb, _ip), _ptr(syn, _up), _ptr(cr, _up),
                                          out["status"].ctypes.data_as(_ip), out["corrected"].ctypes.data_as(_ip), _ptr(out.get("pick"), _ip)), who)
    return out


def polar_recon_prior_host(log2_n, info_pos, keys, syndrome, key_bits=None, messages="i8", maxq=31, prior=None, pin=None):
    """the prior's mirror (qldpc_polar_recon_prior_host) -> (llr [B, N] int8 or float32, frozen uint32 [B, W])"""
    who = "polar_recon_prior_host"
    kind, dt = _messages(messages)
    n, N, W, pos = _code(log2_n, info_pos)
    keys = _rows(who, keys, W, "keys")
    B = keys.shape[0]
    syn, kb = _rows(who, syndrome, (max(N - pos.size, 0) + 31) // 32, "syndrome"), _vec(who, key_bits, B, "key_bits", np.int32)
    p, q = _levels(kind, maxq, prior, pin)
    llr, frozen = np.zeros((B, N), dt), np.zeros((B, W), np.uint32)
    _chk(_L.qldpc_polar_recon_prior_host(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), p, q, B, keys.ctypes.data_as(_up), _ptr(kb, _ip), _ptr(syn, _up),
                                         llr.ctypes.data_as(_vp), frozen.ctypes.data_as(_up)), who)
    return llr, frozen


def polar_recon_verdict_host(log2_n, n_info, info, x, keys, crc=None, pick=None, key_bits=None, crc_len=0, crc_poly=0):
    """the verdict's mirror (qldpc_polar_recon_verdict_host): info uint32 [B, ceil(K/32)] and x uint32 [B, W] as a decoder gave them, pick int32 [B]
    or None (then the CRC decides), keys uint32 [B, W] Bob's, crc uint32 [B] Alice's -> dict(keys (a copy, rewritten where OK), status, corrected)"""
    who = "polar_recon_verdict_host"
    n, W = int(log2_n), _words(log2_n)
    x = _rows(who, x, W, "x")
    B = x.shape[0]
    info, keys = _rows(who, info, (max(int(n_info), 0) + 31) // 32, "info"), _rows(who, keys, W, "keys").copy()
    cr, pk, kb = _vec(who, crc, B, "crc", np.uint32), _vec(who, pick, B, "pick", np.int32), _vec(who, key_bits, B, "key_bits", np.int32)
    out = dict(keys=keys, status=np.zeros(B, np.int32), corrected=np.zeros(B, np.int32))
    _chk(_L.qldpc_polar_recon_verdict_host(n, int(n_info), int(crc_len), int(crc_poly) & 0xffffffff, B, _ptr(info, _up), x.ctypes.data_as(_up), _ptr(pk, _ip),
                                           keys.ctypes.data_as(_up), _ptr(kb, _ip), _ptr(cr, _up), out["status"].ctypes.data_as(_ip),
                                           out["corrected"].ctypes.data_as(_ip)), who)
    return out


# ---- incremental freezing: the mirrors ------------------------------------------------------------------------------------------------------

def polar_recon_encode_ladder_host(log2_n, info_pos, extra_pos, keys, key_bits=None, crc_len=0, crc_poly=0):
    """Alice's mirror with a ladder (qldpc_polar_recon_encode_ladder_host): extra_pos int32 [E] the disclosure order
    -> (syndrome, crc, extra_bits uint32 [B, ceil(E / 32)]: the bits of u at extra_pos, MSB-first)"""
    who = "polar_recon_encode_ladder_host"
    n, N, W, pos = _code(log2_n, info_pos)
    xp = np.ascontiguousarray(extra_pos, dtype=np.int32).ravel()
    keys = _rows(who, keys, W, "keys")
    B = keys.shape[0]
    kb = _vec(who, key_bits, B, "key_bits", np.int32)
    syn, crc, xb = np.zeros((B, (max(N - pos.size, 0) + 31) // 32), np.uint32), np.zeros(B, np.uint32), np.zeros((B, (xp.size + 31) // 32), np.uint32)
    _chk(_L.qldpc_polar_recon_encode_ladder_host(n, pos.size, pos.ctypes.data_as(_ip), int(crc_len), int(crc_poly) & 0xffffffff, xp.size, xp.ctypes.data_as(_ip), B,
                                                 keys.ctypes.data_as(_up), _ptr(kb, _ip), syn.ctypes.data_as(_up), crc.ctypes.data_as(_up), xb.ctypes.data_as(_up)), who)
    return syn, crc, xb


def polar_recon_decode_rounds_host(log2_n, info_pos, extra_pos, keys, syndrome, crc, extra_bits, extra, step=16, max_rounds=1, key_bits=None, resume=False,
                                   status=None, messages="i8", maxq=31, crc_len=0, crc_poly=0, prior=None, pin=None):
    """Bob's rounds mirror (qldpc_polar_recon_decode_rounds_host): extra int32 [B] the start counts, status int32 [B] read with resume
    -> dict(keys (a copy, corrected where OK), status, corrected, extra (the count of each block's last decode), decodes, open_per_round int32
    [max_rounds]); with resume the rows of the blocks that are not open come back as they were given (corrected: -1 where none was given)"""
    who = "polar_recon_decode_rounds_host"
    kind, _ = _messages(messages)
    n, N, W, pos = _code(log2_n, info_pos)
    xp = np.ascontiguousarray(extra_pos, dtype=np.int32).ravel()
    keys = _rows(who, keys, W, "keys").copy()
    B = keys.shape[0]
    syn, xb = _rows(who, syndrome, (max(N - pos.size, 0) + 31) // 32, "syndrome"), _rows(who, extra_bits, (xp.size + 31) // 32, "extra_bits")
    cr, kb = _vec(who, crc, B, "crc", np.uint32), _vec(who, key_bits, B, "key_bits", np.int32)
    ex = _vec(who, extra, B, "extra", np.int32).copy()
    st = np.zeros(B, np.int32) if status is None else _vec(who, status, B, "status", np.int32).copy()
    if resume and status is None:
        raise QldpcError(-1, "%s: resume needs the status of the call before" % who)
    p, q = _levels(kind, maxq, prior, pin)
    out = dict(keys=keys, status=st, corrected=np.full(B, -1, np.int32), extra=ex, decodes=np.zeros(B, np.int32),
               open_per_round=np.zeros(max(int(max_rounds), 1), np.int32))
    _chk(_L.qldpc_polar_recon_decode_rounds_host(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), int(crc_len), int(crc_poly) & 0xffffffff, p, q, xp.size,
                                                 xp.ctypes.data_as(_ip), B, keys.ctypes.data_as(_up), _ptr(kb, _ip), _ptr(syn, _up), _ptr(cr, _up), _ptr(xb, _up),
                                                 ex.ctypes.data_as(_ip), int(step), int(max_rounds), int(resume), st.ctypes.data_as(_ip),
                                                 out["corrected"].ctypes.data_as(_ip), out["decodes"].ctypes.data_as(_ip), out["open_per_round"].ctypes.data_as(_ip)), who)
    return out


def polar_recon_ladder_extra(log2_n, n_info, n_extra, key_bits, qber, f=1.0):
    """a starting count for a block of key_bits bits at a given QBER (qldpc_polar_recon_ladder_extra_host): clamp(ceil(f h2(qber) key_bits) -
    (N - K), 0, n_extra).  A suggestion: no session calls it"""
    return _chk(_L.qldpc_polar_recon_ladder_extra_host(int(log2_n), int(n_info), int(n_extra), int(key_bits), float(qber), float(f)), "polar_recon_ladder_extra")


# ---- SC-Flip trials: the mirrors ------------------------------------------------------------------------------------------------------------

def _select_args(who, log2_n, leaf, frozen_mask, rank, extra, messages):
    kind, dt = _messages(messages)
    n = int(log2_n)
    N, W = (1 << n) if 0 <= n <= POLAR_MAX_LOG2N else 1, _words(n)
    leaf = np.ascontiguousarray(leaf, dtype=dt)
    if leaf.ndim != 2 or leaf.shape[1] != N:
        raise QldpcError(-6, "%s: leaf must be [frames, %d]" % (who, N))
    F = leaf.shape[0]
    return kind, n, F, leaf, _vec(who, frozen_mask, W, "frozen_mask", np.uint32), _vec(who, rank, N, "rank", np.int32), _vec(who, extra, F, "extra", np.int32)


def polar_flip_select_host(log2_n, leaf, frozen_mask, n_flips, rank=None, extra=None, messages="i8"):
    """the flips of each frame (qldpc_polar_flip_select_host): leaf [F, N] int8 or float32 the SC decoder's leaf beliefs, frozen_mask uint32 [W]
    (1 = frozen), rank int32 [N] a ladder's rank table or None, extra int32 [F] the frames' ladder counts or None -> pos int32 [F, n_flips]: the
    n_flips candidates of the smallest (|leaf|, position), ascending, -1 where there are fewer"""
    who = "polar_flip_select_host"
    kind, n, F, leaf, mask, rk, ex = _select_args(who, log2_n, leaf, frozen_mask, rank, extra, messages)
    pos = np.zeros((F, max(int(n_flips), 0)), np.int32)
    _chk(_L.qldpc_polar_flip_select_host(n, kind, F, leaf.ctypes.data_as(_vp), _ptr(mask, _up), _ptr(rk, _ip), _ptr(ex, _ip), int(n_flips), pos.ctypes.data_as(_ip)), who)
    return pos


def polar_recon_decode_flip_host(log2_n, info_pos, keys, syndrome, crc, n_flips=8, extra_pos=(), extra_bits=None, extra=None, key_bits=None, resume=False, status=None,
                                 messages="i8", maxq=31, crc_len=0, crc_poly=0, prior=None, pin=None):
    """Bob's flip mirror (qldpc_polar_recon_decode_flip_host): the first pass (or, with resume, the EDECODE blocks of `status`), then for each open
    block a probe and n_flips trials -> dict(keys (a copy, corrected where OK), status, corrected, flip_pos (-1 where no flip rescued the block),
    decodes, n_tried)"""
    who = "polar_recon_decode_flip_host"
    kind, _ = _messages(messages)
    n, N, W, pos = _code(log2_n, info_pos)
    xp = np.ascontiguousarray(extra_pos, dtype=np.int32).ravel()
    keys = _rows(who, keys, W, "keys").copy()
    B = keys.shape[0]
    syn, xb = _rows(who, syndrome, (max(N - pos.size, 0) + 31) // 32, "syndrome"), _rows(who, extra_bits, (xp.size + 31) // 32, "extra_bits")
    cr, kb, ex = _vec(who, crc, B, "crc", np.uint32), _vec(who, key_bits, B, "key_bits", np.int32), _vec(who, extra, B, "extra", np.int32)
    if resume and status is None:
        raise QldpcError(-1, "%s: resume needs the status of the call before" % who)
    st = np.zeros(B, np.int32) if status is None else _vec(who, status, B, "status", np.int32).copy()
    p, q = _levels(kind, maxq, prior, pin)
    out = dict(keys=keys, status=st, corrected=np.full(B, -1, np.int32), flip_pos=np.full(B, -1, np.int32), decodes=np.zeros(B, np.int32))
    tried = C.c_int(0)
    _chk(_L.qldpc_polar_recon_decode_flip_host(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), int(crc_len), int(crc_poly) & 0xffffffff, p, q, xp.size,
                                               xp.ctypes.data_as(_ip), B, keys.ctypes.data_as(_up), _ptr(kb, _ip), _ptr(syn, _up), _ptr(cr, _up), _ptr(xb, _up), _ptr(ex, _ip),
                                               int(n_flips), int(resume), st.ctypes.data_as(_ip), out["corrected"].ctypes.data_as(_ip), out["flip_pos"].ctypes.data_as(_ip),
                                               out["decodes"].ctypes.data_as(_ip), C.byref(tried)), who)
    out["n_tried"] = tried.value
    return out


def _up_dev(a, device=0):
    """a host array on the device (uint32 words as int32); None stays None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return _torch().from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:%d" % device)


def _p(t):
    return _vp(t.data_ptr()) if t is not None and t.numel() else None


def polar_recon_prior(log2_n, info_pos, keys, syndrome, key_bits=None, messages="i8", maxq=31, prior=None, pin=None, device=0):
    """the prior kernel on its own (qldpc_polar_recon_prior_dev) on torch's current stream: host arrays in, the code's tables sent up, host arrays
    out, as polar_recon_prior_host -> (llr, frozen)"""
    who = "polar_recon_prior"
    torch = _torch()
    kind, dt = _messages(messages)
    n, N, W, pos = _code(log2_n, info_pos)
    keys = _rows(who, keys, W, "keys")
    B = keys.shape[0]
    syn, kb = _rows(who, syndrome, (max(N - pos.size, 0) + 31) // 32, "syndrome"), _vec(who, key_bits, B, "key_bits", np.int32)
    mask, prefix, _ = polar_recon_tables(n, pos)
    p, q = _levels(kind, maxq, prior, pin)
    with torch.cuda.device(device):
        d_mask, d_prefix, d_keys, d_kb, d_syn = (_up_dev(a, device) for a in (mask, prefix, keys, kb, syn))
        llr = _dev_empty(device, (B, N), torch.int8 if kind == POLAR_I8 else torch.float32)
        frozen = _dev_empty(device, (B, W), torch.int32)
        _chk(_L.qldpc_polar_recon_prior_dev(_stream_arg(None, device), n, N - pos.size, _p(d_mask), _p(d_prefix), kind, int(maxq), p, q, B, _p(d_keys), _p(d_kb), _p(d_syn),
                                            _p(llr), _p(frozen)), who)
        return llr.cpu().numpy(), frozen.cpu().numpy().view(np.uint32)


def polar_recon_verdict(log2_n, n_info, info, x, keys, crc=None, pick=None, key_bits=None, crc_len=0, crc_poly=0, device=0):
    """the verdict kernel on its own (qldpc_polar_recon_verdict_dev) on torch's current stream: host arrays in, host arrays out, as
    polar_recon_verdict_host -> dict(keys, status, corrected)"""
    who = "polar_recon_verdict"
    torch = _torch()
    n, W = int(log2_n), _words(log2_n)
    x = _rows(who, x, W, "x")
    B = x.shape[0]
    info, keys = _rows(who, info, (max(int(n_info), 0) + 31) // 32, "info"), _rows(who, keys, W, "keys")
    cr, pk, kb = _vec(who, crc, B, "crc", np.uint32), _vec(who, pick, B, "pick", np.int32), _vec(who, key_bits, B, "key_bits", np.int32)
    with torch.cuda.device(device):
        d_info, d_x, d_keys, d_cr, d_pk, d_kb = (_up_dev(a, device) for a in (info, x, keys, cr, pk, kb))
        status, corrected = _dev_empty(device, (B,), torch.int32), _dev_empty(device, (B,), torch.int32)
        _chk(_L.qldpc_polar_recon_verdict_dev(_stream_arg(None, device), n, int(n_info), int(crc_len), int(crc_poly) & 0xffffffff, B, _p(d_info), _p(d_x), _p(d_pk),
                                              _p(d_keys), _p(d_kb), _p(d_cr), _p(status), _p(corrected)), who)
        return dict(keys=d_keys.cpu().numpy().view(np.uint32), status=status.cpu().numpy(), corrected=corrected.cpu().numpy())


def polar_flip_select(log2_n, leaf, frozen_mask, n_flips, rank=None, extra=None, messages="i8", device=0):
    """the select kernel on its own (qldpc_polar_flip_select_dev) on torch's current stream: host arrays in, host array out, as
    polar_flip_select_host -> pos int32 [F, n_flips]"""
    who = "polar_flip_select"
    torch = _torch()
    kind, n, F, leaf, mask, rk, ex = _select_args(who, log2_n, leaf, frozen_mask, rank, extra, messages)
    with torch.cuda.device(device):
        d_leaf, d_mask, d_rk, d_ex = (_up_dev(a, device) for a in (leaf, mask, rk, ex))
        pos = _dev_empty(device, (F, max(int(n_flips), 0)), torch.int32)
        _chk(_L.qldpc_polar_flip_select_dev(_stream_arg(None, device), n, kind, F, _p(d_leaf), _p(d_mask), _p(d_rk), _p(d_ex), int(n_flips), _p(pos)), who)
        return pos.cpu().numpy()


class PolarRecon(_Handle):
    """A reconciliation session around `decoder`, a Polar (any form, any rule) or a PolarList with a CRC, which it does not own.  With a Polar the
    CRC is (crc_len, crc_poly); with a PolarList it is the decoder's and both stay 0.  prior and pin: Bob's levels of an unknown and of a padded
    position (None: 1, and maxq with int8 messages, 2^24 with floats).  max_blocks = 0: the decoder's max_frames.  Device tensors in, device
    tensors out, asynchronous on torch's current stream.  extra_pos: a ladder session (decode_rounds).  max_flips > 0: a flip session
    (decode_flip), a ladder session (extra_pos None: an empty ladder) that also owns the scratch of SC-Flip trials."""
    _free = _L.qldpc_polar_recon_free

    def __init__(self, decoder, crc_len=0, crc_poly=0, prior=None, pin=None, max_blocks=0, extra_pos=None, max_flips=0):
        is_list = isinstance(decoder, PolarList)
        self.decoder = decoder
        self.prior, self.pin = _levels(decoder.messages, decoder.maxq, prior, pin)
        if max_flips and extra_pos is None:
            extra_pos = ()
        self.extra_pos = None if extra_pos is None else np.ascontiguousarray(extra_pos, dtype=np.int32).ravel()
        if max_flips:                       # a flip session: a ladder session with the scratch of the trials
            if is_list:
                raise QldpcError(-7, "PolarRecon: a flip session needs an SC Polar (the list decoder has no rows form)")
            self._h = _create("PolarRecon", _L.qldpc_polar_recon_create_flip, decoder._h, int(crc_len), int(crc_poly) & 0xffffffff, self.prior, self.pin,
                              int(max_blocks), self.extra_pos.size, self.extra_pos.ctypes.data_as(_ip), int(max_flips))
        elif self.extra_pos is not None:      # a ladder session (incremental freezing): an SC Polar of the lanes form only
            if is_list:
                raise QldpcError(-7, "PolarRecon: a ladder session needs an SC Polar (the list decoder has no rows form)")
            self._h = _create("PolarRecon", _L.qldpc_polar_recon_create_ladder, decoder._h, int(crc_len), int(crc_poly) & 0xffffffff, self.prior, self.pin,
                              int(max_blocks), self.extra_pos.size, self.extra_pos.ctypes.data_as(_ip))
        else:
            self._h = _create("PolarRecon", _L.qldpc_polar_recon_create, None if is_list else decoder._h, decoder._h if is_list else None, int(crc_len),
                              int(crc_poly) & 0xffffffff, self.prior, self.pin, int(max_blocks))
        self.extra_words = int(_L.qldpc_polar_recon_extra_words(self._h))
        self.max_flips = int(_L.qldpc_polar_recon_max_flips(self._h))
        self.max_blocks = int(max_blocks) or decoder.max_frames
        self.crc_len, self.crc_poly = (decoder.crc_len, decoder.crc_poly) if is_list else (int(crc_len), int(crc_poly))
        self.syndrome_words = int(_L.qldpc_polar_recon_syndrome_words(self._h))
        self.leaked_bits = int(_L.qldpc_polar_recon_leaked_bits(self._h))

    def device_bytes(self):
        return int(_L.qldpc_polar_recon_device_bytes(self._h))

    def _inputs(self, keys, key_bits):
        torch = _torch()
        pk = _dev_rows(keys, None, self.decoder.W, (torch.int32, torch.uint32), "keys")
        return torch, keys.shape[0], pk, _dev_vec(key_bits, keys.shape[0], torch.int32, "key_bits")

    def encode(self, keys, key_bits=None, want_extra=False):
        """Alice: keys int32 / uint32 [B, W] packed rows on the device, key_bits int32 [B] or None (every block is N bits)
        -> (syndrome int32 [B, syndrome_words], crc int32 [B]) on the device and, with want_extra (a ladder session), extra_bits int32
        [B, extra_words]: the bits of u at extra_pos, of which she sends a prefix per round"""
        torch, B, pk, pb = self._inputs(keys, key_bits)
        syn, crc = _dev_empty(keys.device, (B, self.syndrome_words), torch.int32), _dev_empty(keys.device, (B,), torch.int32)
        self.decoder._on_current_stream()
        if want_extra:
            xb = _dev_empty(keys.device, (B, self.extra_words), torch.int32)
            _chk(_L.qldpc_polar_recon_encode_ladder_dev(self._h, B, pk, pb, _p(syn), _p(crc), _p(xb)), "PolarRecon.encode")
            return syn, crc, xb
        _chk(_L.qldpc_polar_recon_encode_dev(self._h, B, pk, pb, _p(syn), _p(crc)), "PolarRecon.encode")
        return syn, crc

    def decode(self, keys, syndrome, crc, key_bits=None, want_pick=False):
        """Bob: keys [B, W] corrected IN PLACE where a block is OK, syndrome [B, syndrome_words] and crc [B] Alice's
        -> dict of device tensors: status int32 [B] (0 OK, -9 EDECODE, -6 a key_bits out of range), corrected int32 [B] (the flips, -1 where not
        OK) and, with want_pick (a PolarList only), pick int32 [B]"""
        torch, B, pk, pb = self._inputs(keys, key_bits)
        words = (torch.int32, torch.uint32)
        ps = _dev_rows(syndrome, B, self.syndrome_words, words, "syndrome") if self.syndrome_words else None
        assert crc.is_cuda and crc.dtype in words and crc.is_contiguous() and tuple(crc.shape) == (B,), "crc"
        out = dict(status=_dev_empty(keys.device, (B,), torch.int32), corrected=_dev_empty(keys.device, (B,), torch.int32))
        if want_pick:
            out["pick"] = _dev_empty(keys.device, (B,), torch.int32)
        self.decoder._on_current_stream()
        _chk(_L.qldpc_polar_recon_decode_dev(self._h, B, pk, pb, ps, _vp(crc.data_ptr()), _p(out["status"]), _p(out["corrected"]), _p(out.get("pick"))),
             "PolarRecon.decode")
        return out

    def decode_rounds(self, keys, syndrome, crc, extra_bits, extra, step=16, max_rounds=1, key_bits=None, resume=False, status=None):
        """Bob, incremental freezing (a ladder session; qldpc_polar_recon_decode_rounds): up to max_rounds rounds over the blocks that are open,
        each failed block frozen `step` positions further along extra_pos before its next decode.  keys [B, W] corrected IN PLACE where a block
        is OK; extra int32 [B] the start counts, rewritten IN PLACE to the count of each block's last decode; extra_bits [B, extra_words] Alice's
        row, of which only the first extra[b] bits of a block are looked at; resume: `status` int32 [B] of the call before is read and rewritten
        IN PLACE, and only its EDECODE blocks are open.  THIS CALL WAITS for the stream once a round (the open count)
        -> dict(status, corrected, decodes int32 [B] on the device, open_per_round: a list of max_rounds ints)"""
        torch, B, pk, pb = self._inputs(keys, key_bits)
        words = (torch.int32, torch.uint32)
        ps = _dev_rows(syndrome, B, self.syndrome_words, words, "syndrome") if self.syndrome_words else None
        px = _dev_rows(extra_bits, B, self.extra_words, words, "extra_bits") if self.extra_words else None
        assert crc.is_cuda and crc.dtype in words and crc.is_contiguous() and tuple(crc.shape) == (B,), "crc"
        pe = _dev_vec(extra, B, torch.int32, "extra")
        if resume and status is None:
            raise QldpcError(-1, "PolarRecon.decode_rounds: resume needs the status of the call before")
        st = _dev_empty(keys.device, (B,), torch.int32) if status is None else status
        _dev_vec(st, B, torch.int32, "status")
        out = dict(status=st, corrected=torch.full((B,), -1, dtype=torch.int32, device=keys.device) if resume else _dev_empty(keys.device, (B,), torch.int32),
                   decodes=_dev_empty(keys.device, (B,), torch.int32))
        rounds = (C.c_int * max(int(max_rounds), 1))()
        self.decoder._on_current_stream()
        _chk(_L.qldpc_polar_recon_decode_rounds(self._h, B, pk, pb, ps, _vp(crc.data_ptr()), px, pe, int(step), int(max_rounds), int(resume), _p(st),
                                                _p(out["corrected"]), _p(out["decodes"]), rounds), "PolarRecon.decode_rounds")
        out["open_per_round"] = list(rounds)
        return out

    def decode_flip(self, keys, syndrome, crc, n_flips=8, extra_bits=None, extra=None, key_bits=None, resume=False, status=None):
        """Bob, SC-Flip trials (a flip session; qldpc_polar_recon_decode_flip): every block once (or, with resume, nothing: `status` int32 [B] of the
        call before is read and rewritten IN PLACE and only its EDECODE blocks are open), then each failed block again with the decision at one of
        its n_flips least reliable information leaves inverted; the first trial that passes the verdict is kept.  Local to Bob: nothing is
        disclosed.  keys [B, W] corrected IN PLACE where a block is OK; extra int32 [B] the blocks' ladder counts (only read; None: all 0) and
        extra_bits [B, extra_words] as in decode_rounds.  THIS CALL WAITS for the stream once (the open count)
        -> dict(keys, status, corrected, flip_pos int32 [B] (-1 where no flip rescued the block), decodes on the device, n_tried: an int)"""
        torch, B, pk, pb = self._inputs(keys, key_bits)
        words = (torch.int32, torch.uint32)
        ps = _dev_rows(syndrome, B, self.syndrome_words, words, "syndrome") if self.syndrome_words else None
        px = _dev_rows(extra_bits, B, self.extra_words, words, "extra_bits") if self.extra_words and extra_bits is not None else None
        assert crc.is_cuda and crc.dtype in words and crc.is_contiguous() and tuple(crc.shape) == (B,), "crc"
        pe = _dev_vec(extra, B, torch.int32, "extra")
        if resume and status is None:
            raise QldpcError(-1, "PolarRecon.decode_flip: resume needs the status of the call before")
        st = _dev_empty(keys.device, (B,), torch.int32) if status is None else status
        _dev_vec(st, B, torch.int32, "status")
        out = dict(keys=keys, status=st, corrected=torch.full((B,), -1, dtype=torch.int32, device=keys.device) if resume else _dev_empty(keys.device, (B,), torch.int32),
                   flip_pos=_dev_empty(keys.device, (B,), torch.int32), decodes=_dev_empty(keys.device, (B,), torch.int32))
        tried = C.c_int(0)
        self.decoder._on_current_stream()
        _chk(_L.qldpc_polar_recon_decode_flip(self._h, B, pk, pb, ps, _vp(crc.data_ptr()), px, pe, int(n_flips), int(resume), _p(st), _p(out["corrected"]),
                                              _p(out["flip_pos"]), _p(out["decodes"]), C.byref(tried)), "PolarRecon.decode_flip")
        out["n_tried"] = tried.value
        return out

"""Reconciliation sessions (qldpc_recon_*): the engine of the ecd2 LDPC handler, with blind and guessing rounds and their host mirrors."""
import ctypes as C

import numpy as np

from ._lib import _L, _Handle, _chk, _create, _default, _fp, _ip, _np_i32, _ptr, _sig, _torch, _u8p, _up, _vp, QldpcError
from .codes import RULES, SCHEDULES
from .decoder import KernelStat, _profile_rows
from .qber import QBER_MAX_DEGREE
from .mc import GUESS_MAX_BITS, _guess_dev


class ReconCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("efficiency", C.c_float), ("n_rates", C.c_int), ("rates", C.c_float * 8),
                ("n_ite", C.c_int), ("rule", C.c_int), ("rule_param", C.c_float), ("key_quantum", C.c_int),
                ("max_blocks", C.c_int), ("seed", C.c_uint64), ("schedule", C.c_int), ("mother_step", C.c_int), ("mother_max", C.c_int),
                ("rate_gap", C.c_float), ("puncture", C.c_int), ("preload", C.c_int), ("peg_depth", C.c_int), ("gap_profile", C.c_int)]


class ReconMsg(C.Structure):
    _fields_ = [("rate_index", C.c_uint32), ("key_bits", C.c_uint32), ("code_k", C.c_uint32), ("code_m", C.c_uint32),
                ("crc32", C.c_uint32), ("n_punct", C.c_uint32)]


class ReconBlind(C.Structure):
    _fields_ = [("n_known", C.c_int), ("cap", C.c_int), ("pos", _ip), ("bit", _u8p), ("n_ask", C.c_int), ("ask", _ip)]


# a qldpc_recon_guess per block, as a structured array
RECON_GUESS_DTYPE = np.dtype([(f, np.int32) for f in ("tried", "winner", "n_ok", "n_pass", "ambiguous", "trial_iterations")])

_sig("qldpc_recon_cfg_default", None, [C.POINTER(ReconCfg)])
_sig("qldpc_recon_create", C.c_int, [C.POINTER(ReconCfg), C.POINTER(_vp)])
_sig("qldpc_recon_free", None, [_vp])
_sig("qldpc_recon_plan", C.c_int, [_vp, C.c_int, C.c_float, C.POINTER(ReconMsg)])
_sig("qldpc_recon_encode", C.c_int, [_vp, _up, C.c_int, C.c_float, C.POINTER(ReconMsg), _up, C.c_int])
_sig("qldpc_recon_encode_planned", C.c_int, [_vp, _up, C.c_int, C.POINTER(ReconMsg), _up, C.c_int])
_sig("qldpc_recon_decode", C.c_int, [_vp, _up, C.c_int, C.c_float, C.POINTER(ReconMsg), _up, _ip, _ip, _ip])
_sig("qldpc_recon_decode_batch", C.c_int, [_vp, C.c_int, _up, C.c_int, _fp, C.POINTER(ReconMsg), _up, _ip, _ip, _ip])
_sig("qldpc_recon_encode_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), _ip])
_sig("qldpc_recon_decode_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), _ip, _ip, _ip])
_sig("qldpc_crc32_words", C.c_uint32, [_up, C.c_int])
_sig("qldpc_recon_estimate_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, C.POINTER(ReconMsg), C.POINTER(_up), _fp, _up, _fp])
_sig("qldpc_recon_estimate_blocks_merged", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, C.POINTER(ReconMsg), C.POINTER(_up), _fp, _up, _fp])
_sig("qldpc_recon_decode_blind", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), C.POINTER(ReconBlind), C.c_int, _ip, _ip, _ip, _ip])
_sig("qldpc_recon_disclose_host", C.c_int, [_up, C.c_int, _ip, C.c_int, _u8p])
_sig("qldpc_recon_decode_guess", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), C.c_int, _vp, _ip, _ip, _ip])
_sig("qldpc_recon_guess_settle_dev", C.c_int, [C.c_int] * 4 + [_vp] * 12 + [_vp])
_sig("qldpc_recon_guess_settle_host", C.c_int, [C.c_int] * 4 + [_up, _ip, _ip, _up, _ip, _up, _ip, _ip, _up, _up, _ip, _ip])
_sig("qldpc_recon_decode_blocks_tagged", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), C.c_int, C.POINTER(_up), C.POINTER(_up),
                                                   _ip, _ip, _ip])
_sig("qldpc_recon_decode_guess_tagged", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), C.c_int, _vp, C.c_int, C.POINTER(_up),
                                                  C.POINTER(_up), _ip, _ip, _ip])
_sig("qldpc_recon_tag_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, C.c_int, C.POINTER(_up), C.POINTER(_up)])
_sig("qldpc_recon_verify_tag_dev", C.c_int, [C.c_int] * 4 + [_vp] * 7 + [C.c_size_t] + [_vp] * 3 + [_vp])
_sig("qldpc_recon_verify_tag_host", C.c_int, [C.c_int] * 4 + [_up, _up, _ip, _up, _ip, _ip, _up, C.c_size_t, _up, _ip, _up])
_sig("qldpc_recon_tag_host", C.c_int, [_up, C.c_int, _up, C.c_int, _up])
_sig("qldpc_recon_leaked_bits_tagged", C.c_int, [C.POINTER(ReconMsg), C.c_int])
_sig("qldpc_crc32_words_chunked", C.c_uint32, [_up, C.c_int, C.c_int])
RECON_TAG_MAX_KEYS = 4
RECON_TAG_MAX_BITS = 1 << 18
RECON_TAG_LANES = 256
_sig("qldpc_recon_parity_words", C.c_int, [C.POINTER(ReconMsg)])
_sig("qldpc_recon_leaked_bits", C.c_int, [C.POINTER(ReconMsg)])
_sig("qldpc_recon_entries_created", C.c_long, [_vp])
_sig("qldpc_recon_check_header", C.c_int, [_vp, C.POINTER(ReconMsg), C.c_int])
_sig("qldpc_recon_profile_enable", C.c_int, [_vp, C.c_int])
_sig("qldpc_recon_profile_read", C.c_int, [_vp, C.POINTER(KernelStat), C.c_int])


def crc32_words(words, n_bits, lanes=0):
    """CRC-32 of the key bits; lanes > 0: the chunked fold the device verification uses (same value)"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    if lanes:
        return int(_L.qldpc_crc32_words_chunked(w.ctypes.data_as(_up), int(n_bits), int(lanes)))
    return int(_L.qldpc_crc32_words(w.ctypes.data_as(_up), int(n_bits)))


def recon_disclose(key_words, key_bits, pos):
    """Alice's answer to a request for key bits (qldpc_recon_disclose_host): uint8 array, bit pos[i] of her key"""
    kw = np.ascontiguousarray(key_words, dtype=np.uint32)
    p_ = _np_i32(pos)
    out = np.zeros(max(p_.size, 1), np.uint8)
    _chk(_L.qldpc_recon_disclose_host(kw.ctypes.data_as(_up), int(key_bits), p_.ctypes.data_as(_ip), p_.size, out.ctypes.data_as(_u8p)), "recon_disclose")
    return out[:p_.size]


def _settle_result(n, res_keys, res, guess, passed, crc):
    return dict(status=res[0], corrected=res[1], iterations=res[2], crc=res[3], keys=res_keys, guess=guess.view(RECON_GUESS_DTYPE).reshape(n) if n else
                np.zeros(0, RECON_GUESS_DTYPE), passed=passed, trial_crc=crc)


def recon_guess_settle_host(g, trial_rows, ok, iters, keys, key_bits, crc_want, first_iters):
    """the verdict of a guessing round of a session on the host (qldpc_recon_guess_settle_host): trial_rows uint32 [n_src 2^g, Wn], ok and iters
    [n_src 2^g], keys uint32 [n_src, Wk] (the keys handed in), key_bits, crc_want, first_iters [n_src] -> dict(status, corrected, iterations, crc [n_src],
    keys uint32 [n_src, Wk] (words past a key's length stay 0), guess (RECON_GUESS_DTYPE [n_src]), passed int32 and trial_crc uint32 [n_src 2^g])"""
    rows, kw = np.ascontiguousarray(trial_rows, dtype=np.uint32), np.ascontiguousarray(keys, dtype=np.uint32)
    if rows.ndim != 2 or kw.ndim != 2:
        raise QldpcError(-6, "recon_guess_settle_host: trial_rows and keys are 2-D arrays")
    n, slots = kw.shape[0], rows.shape[0]
    ok, it = np.ascontiguousarray(ok, dtype=np.int32).ravel(), np.ascontiguousarray(iters, dtype=np.int32).ravel()
    kb, want, first = _np_i32(key_bits).ravel(), np.ascontiguousarray(crc_want, dtype=np.uint32).ravel(), _np_i32(first_iters).ravel()
    if 0 <= int(g) <= GUESS_MAX_BITS and (slots != n << int(g) or ok.size != slots or it.size != slots or kb.size != n or want.size != n or first.size != n):
        raise QldpcError(-6, "recon_guess_settle_host: %d sources of %d trials with %d rows, %d / %d flags and counts, %d / %d / %d scalars" %
                         (n, 1 << int(g), slots, ok.size, it.size, kb.size, want.size, first.size))
    passed, crc = np.zeros(max(slots, 1), np.int32), np.zeros(max(slots, 1), np.uint32)
    res_keys, res, guess = np.zeros((n, kw.shape[1]), np.uint32), np.zeros((4, max(n, 1)), np.int32), np.zeros((max(n, 1), 6), np.int32)
    _chk(_L.qldpc_recon_guess_settle_host(int(g), n, kw.shape[1], rows.shape[1], _ptr(rows, _up), _ptr(ok, _ip), _ptr(it, _ip), _ptr(kw, _up), _ptr(kb, _ip), _ptr(want, _up),
                                          _ptr(first, _ip), _ptr(passed, _ip), _ptr(crc, _up), _ptr(res_keys, _up), _ptr(res, _ip), _ptr(guess, _ip)),
         "recon_guess_settle_host")
    return _settle_result(n, res_keys, res[:, :n], guess[:n], passed[:slots], crc[:slots])


def recon_guess_settle(g, trial_rows, ok, iters, keys, key_bits, crc_want, first_iters, stream=None):
    """qldpc_recon_guess_settle_dev: the same over contiguous device int32 tensors (trial_rows [n_src 2^g, Wn], ok, iters [n_src 2^g], keys [n_src, Wk], key_bits,
    crc_want, first_iters [n_src]) -> the dict of recon_guess_settle_host as numpy arrays (the call is asynchronous on `stream`; the copies back wait for it)"""
    torch = _torch()
    g, n, slots, Wk, Wn = int(g), int(keys.shape[0]), int(trial_rows.shape[0]), int(keys.shape[1]), int(trial_rows.shape[1])
    if 0 <= g <= GUESS_MAX_BITS and slots != n << g:
        raise QldpcError(-6, "recon_guess_settle: %d sources of %d trials with %d rows" % (n, 1 << g, slots))
    ptrs = [_guess_dev(trial_rows, slots, Wn, "recon_guess_settle", "trial_rows"), _guess_dev(ok, slots, 0, "recon_guess_settle", "ok"),
            _guess_dev(iters, slots, 0, "recon_guess_settle", "iters"), _guess_dev(keys, n, Wk, "recon_guess_settle", "keys")]
    ptrs += [_guess_dev(t, n, 0, "recon_guess_settle", name) for t, name in ((key_bits, "key_bits"), (crc_want, "crc_want"), (first_iters, "first_iters"))]
    dev = keys.device
    passed, crc = (torch.zeros(max(slots, 1), dtype=torch.int32, device=dev) for _ in range(2))
    res_keys, res, guess = torch.zeros((n, Wk), dtype=torch.int32, device=dev), torch.zeros((4, max(n, 1)), dtype=torch.int32, device=dev), torch.zeros((max(n, 1), 6), dtype=torch.int32, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream(dev)      # the stream itself: the copies back are put on it
    with torch.cuda.device(dev), torch.cuda.stream(s):
        _chk(_L.qldpc_recon_guess_settle_dev(g, n, Wk, Wn, *ptrs, _vp(passed.data_ptr()), _vp(crc.data_ptr()), _vp(res_keys.data_ptr()), _vp(res.data_ptr()),
                                             _vp(guess.data_ptr()), _vp(s.cuda_stream)), "recon_guess_settle")
        host = [t.cpu().numpy() for t in (res_keys, res, guess, passed, crc)]
    return _settle_result(n, host[0].view(np.uint32), host[1][:, :n], np.ascontiguousarray(host[2][:n]), host[3][:slots], host[4][:slots].view(np.uint32))


def recon_tag_host(key_words, key_bits, hash_key, lanes=RECON_TAG_LANES):
    """the sessions' keyed tag of one block under one key (hash_key: its two words hi, lo) on the host (qldpc_recon_tag_host), by the kernels' chunked
    Horner and fold with `lanes` lanes (a power of two) -> the tag's two words (hi, lo): polyhash_host's tag for every such lanes"""
    kw, hk = np.ascontiguousarray(key_words, dtype=np.uint32), np.ascontiguousarray(hash_key, dtype=np.uint32)
    key_bits = int(key_bits)
    if key_bits <= 0 or kw.size < (key_bits + 31) // 32 or hk.size < 2:
        raise QldpcError(-6, "recon_tag_host: %d key words, key_bits = %d, %d hash key words" % (kw.size, key_bits, hk.size))
    out = np.zeros(2, np.uint32)
    _chk(_L.qldpc_recon_tag_host(_ptr(kw, _up), key_bits, _ptr(hk, _up), int(lanes), _ptr(out, _up)), "recon_tag_host")
    return out


def recon_leaked_bits_tagged(msg, n_keys=1):
    """what a tagged block discloses at the most: Recon.leaked_bits(msg) + 61 n_keys (the CRC and the tags are both charged)"""
    if not 1 <= int(n_keys) <= RECON_TAG_MAX_KEYS:
        raise QldpcError(-6, "recon_leaked_bits_tagged: n_keys = %d" % n_keys)
    return int(_L.qldpc_recon_leaked_bits_tagged(C.byref(msg), int(n_keys)))


def _verify_tag_result(n, res_keys, res, tags):
    return dict(status=res[0], corrected=res[1], iterations=res[2], crc=res[3].view(np.uint32), keys=res_keys, tags=tags)


def _hash_key_rows(who, n, hash_keys):
    """hash_keys of a call over n blocks: ONE row of 2 r words, shared, or n rows -> (rows uint32 [1 or n, 2 r], r, shared)"""
    hk = np.ascontiguousarray(hash_keys, dtype=np.uint32)
    shared = hk.ndim == 1
    hk = hk.reshape(1, -1) if shared else hk
    if hk.ndim != 2 or hk.shape[1] % 2 or (not shared and hk.shape[0] != n):
        raise QldpcError(-6, "%s: hash_keys of shape %s for %d blocks: one row of 2 r words or one row per block" % (who, hk.shape, n))
    return hk, hk.shape[1] // 2, shared


def recon_verify_tag_host(out_rows, keys, key_bits, crc_want, ok, iters, hash_keys):
    """the verdict of a tagged verify step on the host (qldpc_recon_verify_tag_host): out_rows uint32 [n, Wn] decoded rows, keys uint32 [n, Wk] the keys
    handed in, key_bits, crc_want, ok, iters [n], hash_keys one shared row of 2 r words or [n, 2 r] -> dict(status, corrected, iterations, crc [n], keys
    uint32 [n, Wk] (words past a key's length stay 0), tags uint32 [n, 2 r], zeros for a block that is not ok with the wanted CRC)"""
    rows, kw = np.ascontiguousarray(out_rows, dtype=np.uint32), np.ascontiguousarray(keys, dtype=np.uint32)
    if rows.ndim != 2 or kw.ndim != 2 or rows.shape[0] != kw.shape[0]:
        raise QldpcError(-6, "recon_verify_tag_host: out_rows and keys are 2-D arrays of as many rows")
    n = kw.shape[0]
    hk, r, shared = _hash_key_rows("recon_verify_tag_host", n, hash_keys)
    kb, want = _np_i32(key_bits).ravel(), np.ascontiguousarray(crc_want, dtype=np.uint32).ravel()
    ok, it = _np_i32(ok).ravel(), _np_i32(iters).ravel()
    if not kb.size == want.size == ok.size == it.size == n:
        raise QldpcError(-6, "recon_verify_tag_host: %d blocks with %d / %d / %d / %d scalars" % (n, kb.size, want.size, ok.size, it.size))
    res_keys, res, tags = np.zeros((n, kw.shape[1]), np.uint32), np.zeros((4, max(n, 1)), np.int32), np.zeros((max(n, 1), max(2 * r, 1)), np.uint32)
    _chk(_L.qldpc_recon_verify_tag_host(n, r, kw.shape[1], rows.shape[1], _ptr(rows, _up), _ptr(kw, _up), _ptr(kb, _ip), _ptr(want, _up), _ptr(ok, _ip), _ptr(it, _ip),
                                        _ptr(hk, _up), 0 if shared else hk.shape[1], _ptr(res_keys, _up), _ptr(res, _ip), _ptr(tags, _up)), "recon_verify_tag_host")
    return _verify_tag_result(n, res_keys, res[:, :n], tags[:n])


def recon_verify_tag(out_rows, keys, key_bits, crc_want, ok, iters, hash_keys, stream=None):
    """qldpc_recon_verify_tag_dev: the same over contiguous device int32 tensors (out_rows [n, Wn], keys [n, Wk], key_bits, crc_want, ok, iters [n],
    hash_keys 1-D of 2 r words, shared, or [n, 2 r]) -> the dict of recon_verify_tag_host as numpy arrays (the call is asynchronous on `stream`; the
    copies back wait for it)"""
    torch = _torch()
    n, Wk, Wn = int(keys.shape[0]), int(keys.shape[1]), int(out_rows.shape[1])
    shared = hash_keys.dim() == 1
    hk = hash_keys.unsqueeze(0) if shared else hash_keys
    if hk.dim() != 2 or hk.shape[1] % 2 or (not shared and hk.shape[0] != n):
        raise QldpcError(-6, "recon_verify_tag: hash_keys of shape %s for %d blocks" % (tuple(hk.shape), n))
    r = int(hk.shape[1]) // 2
    ptrs = [_guess_dev(out_rows, n, Wn, "recon_verify_tag", "out_rows"), _guess_dev(keys, n, Wk, "recon_verify_tag", "keys")]
    ptrs += [_guess_dev(t, n, 0, "recon_verify_tag", name) for t, name in ((key_bits, "key_bits"), (crc_want, "crc_want"), (ok, "ok"), (iters, "iters"))]
    ptrs.append(_guess_dev(hk, int(hk.shape[0]), 2 * r, "recon_verify_tag", "hash_keys"))
    dev = keys.device
    res_keys, res = torch.zeros((n, Wk), dtype=torch.int32, device=dev), torch.zeros((4, max(n, 1)), dtype=torch.int32, device=dev)
    tags = torch.zeros((max(n, 1), max(2 * r, 1)), dtype=torch.int32, device=dev)
    s = stream if stream is not None else torch.cuda.current_stream(dev)      # the stream itself: the copies back are put on it
    with torch.cuda.device(dev), torch.cuda.stream(s):
        _chk(_L.qldpc_recon_verify_tag_dev(n, r, Wk, Wn, *ptrs, 0 if shared else 2 * r, _vp(res_keys.data_ptr()), _vp(res.data_ptr()), _vp(tags.data_ptr()),
                                           _vp(s.cuda_stream)), "recon_verify_tag")
        host = [t.cpu().numpy() for t in (res_keys, res, tags)]
    return _verify_tag_result(n, host[0].view(np.uint32), host[1][:, :n], np.ascontiguousarray(host[2][:n]).view(np.uint32))


def _tag_args(who, n, hash_keys):
    """the tag arguments of a session call over n blocks -> (what the caller keeps alive, r, hp, tags uint32 [n, 2 r], tp); a shared row is ONE pointer n times"""
    hk, r, shared = _hash_key_rows(who, n, hash_keys)
    tags = np.zeros((n, 2 * r), np.uint32)
    hp = (_up * n)(*[hk[0 if shared else i].ctypes.data_as(_up) for i in range(n)])
    tp = (_up * n)(*[tags[i].ctypes.data_as(_up) for i in range(n)])
    return hk, r, hp, tags, tp


def _block_args(keys, key_bits, qber, msgs, parities, copy_keys):
    """the arguments of a call over a list of blocks -> (the key arrays, copies where the call corrects them in place, and the parity arrays:
    the caller keeps them alive), then what the call takes: kp, kb, qb, arr, pp (kb and qb as arrays; qber None: no qb)"""
    n = len(keys)
    kws = [np.array(k, dtype=np.uint32, copy=True) if copy_keys else np.ascontiguousarray(k, dtype=np.uint32) for k in keys]
    pars = [np.ascontiguousarray(p, dtype=np.uint32) for p in parities]
    kp = (_up * n)(*[k.ctypes.data_as(_up) for k in kws])
    pp = (_up * n)(*[p.ctypes.data_as(_up) for p in pars])
    kb = np.ascontiguousarray(key_bits, dtype=np.int32)
    qb = np.ascontiguousarray(qber, dtype=np.float32) if qber is not None else None
    return (kws, pars), kp, kb, qb, (ReconMsg * n)(*msgs), pp


def _block_results(n, count=3):
    """status, corrected, iterations (and what else a call writes per block): int32 [n] each"""
    return [np.empty(n, np.int32) for _ in range(count)]


class Recon(_Handle):
    """One side's reconciliation engine: what an ecd2 LDPC handler calls (qber_estim.c:337-340,420-423)."""
    _free = _L.qldpc_recon_free

    def __init__(self, device=0, efficiency=1.4, rates=(0.5, 0.7, 0.8, 0.9), n_ite=None, rule=None, rule_param=None,
                 key_quantum=1024, max_blocks=1, seed=7, schedule="auto", mother_step=None, mother_max=None, rate_gap=None,
                 puncture=True, preload=False, peg_depth=None, gap_profile=0):
        cfg = _default(ReconCfg, _L.qldpc_recon_cfg_default)
        cfg.device, cfg.efficiency, cfg.n_rates = int(device), float(efficiency), len(rates)
        for i, r in enumerate(rates):
            cfg.rates[i] = float(r)
        if n_ite is not None:
            cfg.n_ite = int(n_ite)
        if rule is not None:
            cfg.rule, cfg.rule_param = RULES[rule], float(rule_param or 0.0)
        cfg.key_quantum, cfg.max_blocks, cfg.seed = int(key_quantum), int(max_blocks), int(seed)
        cfg.schedule = 2 if schedule == "auto" else SCHEDULES[schedule]      # QLDPC_RECON_SCHED_AUTO: layered for batches (max_blocks > 8), flooding (edge engine) below
        if mother_step is not None:
            cfg.mother_step = int(mother_step)
        if mother_max is not None:
            cfg.mother_max = int(mother_max)
        if rate_gap is not None:
            cfg.rate_gap = float(rate_gap)
        cfg.puncture, cfg.preload = (1 if puncture else 2), int(bool(preload))
        cfg.gap_profile = int(gap_profile)
        if peg_depth is not None:      # library default: 2 (mother codes by progressive edge growth)
            cfg.peg_depth = int(peg_depth)
        self._h = _create("Recon", _L.qldpc_recon_create, C.byref(cfg))
        self.rates = tuple(rates)

    def plan(self, key_bits, qber):
        m = ReconMsg()
        _chk(_L.qldpc_recon_plan(self._h, int(key_bits), float(qber), C.byref(m)), "Recon.plan")
        return m

    @staticmethod
    def parity_words(msg):
        """words of disclosed parity a message carries"""
        return int(_L.qldpc_recon_parity_words(C.byref(msg)))

    @staticmethod
    def leaked_bits(msg):
        return int(_L.qldpc_recon_leaked_bits(C.byref(msg)))

    @property
    def entries_created(self):
        return int(_L.qldpc_recon_entries_created(self._h))

    def profile(self, on=True):
        _chk(_L.qldpc_recon_profile_enable(self._h, int(on)), "Recon.profile")

    def profile_read(self):
        return _profile_rows(_L.qldpc_recon_profile_read, self._h, "Recon.profile_read")

    def encode(self, key_words, key_bits, qber):
        """Alice: -> (msg, parity_words)."""
        kw = np.ascontiguousarray(key_words, dtype=np.uint32)
        m = self.plan(key_bits, qber)
        par = np.zeros(self.parity_words(m), np.uint32)
        _chk(_L.qldpc_recon_encode(self._h, kw.ctypes.data_as(_up), int(key_bits), float(qber), C.byref(m),
                                   par.ctypes.data_as(_up), par.size), "Recon.encode")
        return m, par

    def encode_planned(self, key_words, key_bits, msg, n_punct=0):
        """Alice, second round: the parity bits of the plan in `msg` with only `n_punct` of them withheld (0 = all) -> (msg2, parity_words)."""
        kw = np.ascontiguousarray(key_words, dtype=np.uint32)
        m = ReconMsg.from_buffer_copy(msg)
        m.n_punct = int(n_punct)
        par = np.zeros(self.parity_words(m), np.uint32)
        _chk(_L.qldpc_recon_encode_planned(self._h, kw.ctypes.data_as(_up), int(key_bits), C.byref(m), par.ctypes.data_as(_up), par.size), "Recon.encode_planned")
        return m, par

    def decode(self, key_words, key_bits, qber, msg, parity_words):
        """Bob: -> (ok, key_words, corrected_bits, leaked_bits, iterations); the returned copy is corrected."""
        kw = np.array(key_words, dtype=np.uint32, copy=True)
        par = np.ascontiguousarray(parity_words, dtype=np.uint32)
        c, l, it = C.c_int(0), C.c_int(0), C.c_int(0)
        rc = _L.qldpc_recon_decode(self._h, kw.ctypes.data_as(_up), int(key_bits), float(qber), C.byref(msg),
                                   par.ctypes.data_as(_up), C.byref(c), C.byref(l), C.byref(it))
        if rc not in (0, -9):
            _chk(rc, "Recon.decode")
        return rc == 0, kw, c.value, l.value, it.value

    def decode_batch(self, key_words, key_bits, qber, msgs, parity_words):
        """n blocks of one length on one code; parity_words: one uint32 array per block (they differ in length when the blocks
        are punctured differently) or a 2-D array with ceil(code_m / 32) columns"""
        kw = np.array(key_words, dtype=np.uint32, copy=True)
        n = kw.shape[0]
        Wm = (int(msgs[0].code_m) + 31) // 32
        par = np.zeros((n, Wm), np.uint32)
        for i in range(n):
            row = np.asarray(parity_words[i], dtype=np.uint32).ravel()
            par[i, :min(Wm, row.size)] = row[:Wm]
        qb = np.ascontiguousarray(qber, dtype=np.float32)
        arr = (ReconMsg * n)(*msgs)
        st, co, it = _block_results(n)
        _chk(_L.qldpc_recon_decode_batch(self._h, n, kw.ctypes.data_as(_up), int(key_bits), qb.ctypes.data_as(_fp), arr,
                                         par.ctypes.data_as(_up), st.ctypes.data_as(_ip), co.ctypes.data_as(_ip),
                                         it.ctypes.data_as(_ip)), "Recon.decode_batch")
        return st, kw, co, it

    def encode_blocks(self, keys, key_bits, qber):
        """Alice's side for a list of blocks: returns (msgs, parities), one ReconMsg / uint32 array per block"""
        kb, qb = np.ascontiguousarray(key_bits, dtype=np.int32), np.ascontiguousarray(qber, dtype=np.float32)
        pars = [np.zeros(self.parity_words(self.plan(int(b), float(p))), np.uint32) for b, p in zip(kb, qb)]
        keep, kp, kb, qb, arr, pp = _block_args(keys, kb, qb, (), pars, False)
        caps = np.array([p.size for p in pars], np.int32)
        _chk(_L.qldpc_recon_encode_blocks(self._h, len(keys), kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, caps.ctypes.data_as(_ip)),
             "Recon.encode_blocks")
        return [arr[i] for i in range(len(keys))], pars

    def decode_blocks(self, keys, key_bits, qber, msgs, parities):
        """blocks of any mix of lengths / plans: lists of per-block uint32 arrays; returns (status[], corrected keys, corrected[], iterations[])"""
        (kws, pars), kp, kb, qb, arr, pp = _block_args(keys, key_bits, qber, msgs, parities, True)
        st, co, it = _block_results(len(kws))
        _chk(_L.qldpc_recon_decode_blocks(self._h, len(kws), kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, st.ctypes.data_as(_ip),
                                          co.ctypes.data_as(_ip), it.ctypes.data_as(_ip)), "Recon.decode_blocks")
        return st, kws, co, it

    def estimate_blocks(self, keys, key_bits, msgs, parities, merge=False):
        """Bob's QBER estimate of every block out of its parity message (qldpc_recon_estimate_blocks), before any decode: returns (qber float32 [n],
        counts uint32 [n, QBER_MAX_DEGREE + 1, 2], pooled qber over the call); keys are not touched.  merge=True (qldpc_recon_estimate_blocks_merged):
        runs of checks across punctured parity bits count as one observation each, so a block with half of its parity punctured or more has an estimate"""
        keep, kp, kb, _, arr, pp = _block_args(keys, key_bits, None, msgs, parities, False)
        n = len(keys)
        qb, counts, pool = np.zeros(n, np.float32), np.zeros((n, QBER_MAX_DEGREE + 1, 2), np.uint32), C.c_float(0.0)
        fn = _L.qldpc_recon_estimate_blocks_merged if merge else _L.qldpc_recon_estimate_blocks
        _chk(fn(self._h, n, kp, kb.ctypes.data_as(_ip), arr, pp, qb.ctypes.data_as(_fp), counts.ctypes.data_as(_up), C.byref(pool)), "Recon.estimate_blocks")
        return qb, counts, float(pool.value)

    def decode_blind(self, keys, key_bits, qber, msgs, parities, known, ask_bits):
        """one round of blind reconciliation (qldpc_recon_decode_blind): decode_blocks with known[i] = (positions, Alice's bits there) pinned;
        returns (status[], corrected keys, corrected[], iterations[], leaked[], asks) where asks[i] = the ascending positions block i asks for
        next (empty unless its status is QLDPC_EDECODE)"""
        (kws, pars), kp, kb, qb, arr, pp = _block_args(keys, key_bits, qber, msgs, parities, True)
        n = len(kws)
        pos = [_np_i32(k[0]).ravel() for k in known]
        bit = [np.ascontiguousarray(k[1], dtype=np.uint8).ravel() for k in known]
        ask = [np.zeros(max(1, int(ask_bits)), np.int32) for _ in range(n)]
        bl = (ReconBlind * n)()
        for i in range(n):
            if pos[i].size != bit[i].size:
                raise QldpcError(-1, "Recon.decode_blind: block %d has %d positions and %d bits" % (i, pos[i].size, bit[i].size))
            bl[i].n_known = bl[i].cap = pos[i].size
            bl[i].pos, bl[i].bit, bl[i].ask = pos[i].ctypes.data_as(_ip), bit[i].ctypes.data_as(_u8p), ask[i].ctypes.data_as(_ip)
        st, co, it, lk = _block_results(n, 4)
        _chk(_L.qldpc_recon_decode_blind(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, bl, int(ask_bits), st.ctypes.data_as(_ip),
                                         co.ctypes.data_as(_ip), it.ctypes.data_as(_ip), lk.ctypes.data_as(_ip)), "Recon.decode_blind")
        return st, kws, co, it, lk, [ask[i][:bl[i].n_ask].copy() for i in range(n)]

    def decode_guess(self, keys, key_bits, qber, msgs, parities, guess_bits):
        """decode_blocks with guessing rounds (qldpc_recon_decode_guess): a block whose first decode fails is decoded again with its guess_bits weakest key
        positions pinned to each of the 2^guess_bits values, and the lowest trial with a zero syndrome and Alice's CRC is kept; nothing is disclosed.
        Returns (status[], corrected keys, corrected[], iterations[], guess) with guess a RECON_GUESS_DTYPE array, one row per block"""
        (kws, pars), kp, kb, qb, arr, pp = _block_args(keys, key_bits, qber, msgs, parities, True)
        n = len(kws)
        st, co, it = _block_results(n)
        guess = np.zeros(n, RECON_GUESS_DTYPE)
        guess["winner"] = -1
        _chk(_L.qldpc_recon_decode_guess(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, int(guess_bits), _vp(guess.ctypes.data),
                                         st.ctypes.data_as(_ip), co.ctypes.data_as(_ip), it.ctypes.data_as(_ip)), "Recon.decode_guess")
        return st, kws, co, it, guess

    def decode_blocks_tagged(self, keys, key_bits, qber, msgs, parities, hash_keys):
        """decode_blocks with the keyed tag of every verified block, hashed on the device in the verify step (qldpc_recon_decode_blocks_tagged).
        hash_keys: ONE row of 2 r words (hi, lo per key, r = 1 .. 4), shared by the blocks, or one row per block; the caller draws them after the
        parity messages have arrived.  Returns (status[], corrected keys, corrected[], iterations[], tags) with tags uint32 [n, 2 r]: polyhash_host's
        tag of the key returned for a block that ends QLDPC_OK, zeros for every other"""
        (kws, pars), kp, kb, qb, arr, pp = _block_args(keys, key_bits, qber, msgs, parities, True)
        n = len(kws)
        hk, r, hp, tags, tp = _tag_args("Recon.decode_blocks_tagged", n, hash_keys)
        st, co, it = _block_results(n)
        _chk(_L.qldpc_recon_decode_blocks_tagged(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, r, hp, tp, st.ctypes.data_as(_ip),
                                                 co.ctypes.data_as(_ip), it.ctypes.data_as(_ip)), "Recon.decode_blocks_tagged")
        return st, kws, co, it, tags

    def decode_guess_tagged(self, keys, key_bits, qber, msgs, parities, guess_bits, hash_keys):
        """decode_guess with the keyed tags (qldpc_recon_decode_guess_tagged): a block decoded at once as in decode_blocks_tagged, a rescued block the
        tag of the winner's key, a block still failed zeros.  Returns (status[], corrected keys, corrected[], iterations[], guess, tags)"""
        (kws, pars), kp, kb, qb, arr, pp = _block_args(keys, key_bits, qber, msgs, parities, True)
        n = len(kws)
        hk, r, hp, tags, tp = _tag_args("Recon.decode_guess_tagged", n, hash_keys)
        st, co, it = _block_results(n)
        guess = np.zeros(n, RECON_GUESS_DTYPE)
        guess["winner"] = -1
        _chk(_L.qldpc_recon_decode_guess_tagged(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, int(guess_bits), _vp(guess.ctypes.data), r, hp, tp,
                                                st.ctypes.data_as(_ip), co.ctypes.data_as(_ip), it.ctypes.data_as(_ip)), "Recon.decode_guess_tagged")
        return st, kws, co, it, guess, tags

    def tag_blocks(self, keys, key_bits, hash_keys):
        """the keyed tags of host keys (qldpc_recon_tag_blocks), for either side -- Alice tags her keys once Bob's hash key has arrived: keys a list of
        uint32 word arrays of 1 .. 2^18 bits (bits past key_bits[i] are ignored), hash_keys as in decode_blocks_tagged -> tags uint32 [n, 2 r]"""
        n = len(keys)
        kb = np.ascontiguousarray(key_bits, dtype=np.int32).ravel()
        if kb.size != n:
            raise QldpcError(-6, "Recon.tag_blocks: %d blocks, %d lengths" % (n, kb.size))
        kws = [np.ascontiguousarray(k, dtype=np.uint32) for k in keys]
        for i, k in enumerate(kws):
            if 0 < int(kb[i]) <= RECON_TAG_MAX_BITS and k.size < (int(kb[i]) + 31) // 32:
                raise QldpcError(-6, "Recon.tag_blocks: block %d has %d words for key_bits = %d" % (i, k.size, kb[i]))
        hk, r, hp, tags, tp = _tag_args("Recon.tag_blocks", n, hash_keys)
        kp = (_up * n)(*[k.ctypes.data_as(_up) for k in kws])
        _chk(_L.qldpc_recon_tag_blocks(self._h, n, kp, kb.ctypes.data_as(_ip), r, hp, tp), "Recon.tag_blocks")
        return tags

    def prepare_decode(self, keys, key_bits, qber, msgs, parities):
        """decode_blocks with the argument marshalling done once: returns an object whose run() is the one C call
        (qldpc_recon_decode_blocks) and nothing else -- what a C caller's timed region contains"""
        return _PreparedDecode(self, keys, key_bits, qber, msgs, parities)


class _PreparedDecode:
    def __init__(self, recon, keys, key_bits, qber, msgs, parities):
        self._r = recon
        (self.keys, self._pars), self._kp, self._kb, self._qb, self._msgs, self._pp = _block_args(keys, key_bits, qber, msgs, parities, True)
        self.n = len(self.keys)
        self._orig = [k.copy() for k in self.keys]
        self.status, self.corrected, self.iterations = _block_results(self.n)

    def reset(self):
        """Bob's uncorrected keys again (the decode works in place)"""
        for k, o in zip(self.keys, self._orig):
            k[:] = o

    def run(self):
        _chk(_L.qldpc_recon_decode_blocks(self._r._h, self.n, self._kp, self._kb.ctypes.data_as(_ip), self._qb.ctypes.data_as(_fp), self._msgs, self._pp,
                                          self.status.ctypes.data_as(_ip), self.corrected.ctypes.data_as(_ip), self.iterations.ctypes.data_as(_ip)),
             "Recon.decode_blocks")

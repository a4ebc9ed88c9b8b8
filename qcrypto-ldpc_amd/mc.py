"""Monte-Carlo FER loop (qldpc_mc_*): frame i is a pure function of (seed, i); source, channel and monitor run on the device.  With the
guessing rounds' device calls (qldpc_guess_*) and the host mirrors of every definition."""
import ctypes as C

import numpy as np

from ._lib import (_L, _Handle, _chk, _create, _default, _dev_empty, _dp, _fp, _ip, _np_i32, _ptr, _sig, _stream_arg, _torch, _u8p, _u64p, _up, _vp,
                   QldpcError)


class McCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("batch", C.c_int), ("fail_cap", C.c_int), ("parity_ber", C.c_double), ("reserved", C.c_int * 2)]


class McResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("frames", "bit_errors", "frame_errors", "undetected", "not_converged", "iter_sum", "iter_max",
                                          "channel_flips", "channel_bits", "batches", "next_frame")] + [(n, C.c_double) for n in ("decode_ms", "source_ms", "encode_ms", "channel_ms", "load_ms", "monitor_ms", "total_ms")]


_sig("qldpc_mc_cfg_default", None, [C.POINTER(McCfg)])
_sig("qldpc_mc_philox_host", C.c_int, [_up, _up, _up])
_sig("qldpc_mc_frames_host", C.c_int, [C.c_int, C.c_int, _ip, _u8p, C.c_uint64, C.c_double, C.c_double, C.c_uint64, C.c_int, _up, _up])
_sig("qldpc_mc_create", C.c_int, [_vp, _vp, _u8p, C.POINTER(McCfg), C.POINTER(_vp)])
_sig("qldpc_mc_free", None, [_vp])
_sig("qldpc_mc_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_mc_frames_dev", C.c_int, [_vp, C.c_uint64, C.c_int, C.c_double, _vp, _vp, _vp])
_sig("qldpc_mc_run", C.c_int, [_vp, C.c_double, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(McResult)])
_sig("qldpc_mc_iter_hist", C.c_int, [_vp, _u64p, C.c_int])
_sig("qldpc_mc_failed_frames", C.c_int, [_vp, _u64p, C.c_int])


class McSearchCfg(C.Structure):
    _fields_ = [("n_punct", C.c_int), ("frames_per_pattern", C.c_int), ("key_bits", C.c_int), ("stop_at_goal", C.c_int), ("first_frame", C.c_uint64),
                ("reserved", C.c_int * 2)]


class McSearchResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("patterns", "frames", "batches", "goal", "best", "best_frame_errors", "best_bit_errors", "next_pattern")] + [
        (n, C.c_double) for n in ("decode_ms", "pattern_ms", "expand_ms", "generate_ms", "load_ms", "erase_ms", "monitor_ms", "total_ms")]


MC_PATTERN_STAT = np.dtype([(n, np.uint64) for n in ("pattern", "frames", "frame_errors", "bit_errors", "undetected", "not_converged", "iter_sum")])
MC_NO_PATTERN = 0xFFFFFFFFFFFFFFFF          # goal / best of a search that found none

_sig("qldpc_mc_pattern_host", C.c_int, [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, _ip])
_sig("qldpc_mc_set_candidates", C.c_int, [_vp, _ip, C.c_int])
_sig("qldpc_mc_patterns_dev", C.c_int, [_vp, C.c_uint64, C.c_int, C.c_int, C.c_int, _vp])
_sig("qldpc_mc_pattern_vns", C.c_int, [_vp, C.c_uint64, C.c_int, C.c_int, _ip])
_sig("qldpc_mc_set_puncture", C.c_int, [_vp, _ip, C.c_int])
_sig("qldpc_mc_search", C.c_int, [_vp, C.c_double, C.POINTER(McSearchCfg), C.c_uint64, C.c_uint64, C.POINTER(McSearchResult)])
_sig("qldpc_mc_search_stats", C.c_int, [_vp, _vp, C.c_int])


class McPoint(C.Structure):
    _fields_ = [("qber", C.c_double), ("n_punct", C.c_int), ("reserved", C.c_int)]


class McSweepCfg(C.Structure):
    _fields_ = [("points", C.POINTER(McPoint)), ("n_points", C.c_int), ("punct_order", _ip), ("n_order", C.c_int), ("chunk", C.c_int),
                ("first_frame", C.c_uint64), ("max_frames", C.c_uint64), ("max_frame_errors", C.c_uint64), ("reserved", C.c_int * 2)]


class McSweepResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rounds", "frames", "batches")] + [
        (n, C.c_double) for n in ("decode_ms", "source_ms", "encode_ms", "channel_ms", "load_ms", "erase_ms", "monitor_ms", "total_ms")]


_MC_ROW_COUNTERS = [(n, np.uint64) for n in ("frames", "frame_errors", "bit_errors", "undetected", "not_converged", "iter_sum", "iter_max", "channel_flips",
                                              "channel_bits", "last_round")]          # the tail of a point row and of a stratum row
MC_POINT_STAT = np.dtype([("qber", np.float64), ("n_punct", np.int32), ("closed_by", np.int32)] + _MC_ROW_COUNTERS)
MC_SWEEP_MAX_POINTS = 4096
MC_CLOSED_MAX_FE, MC_CLOSED_MAX_FRAMES = 1, 2          # closed_by of a point row

_sig("qldpc_mc_sweep", C.c_int, [_vp, C.POINTER(McSweepCfg), C.POINTER(McSweepResult)])
_sig("qldpc_mc_sweep_stats", C.c_int, [_vp, _vp, C.c_int])
_sig("qldpc_mc_sweep_hist", C.c_int, [_vp, C.c_int, _u64p, C.c_int])
_sig("qldpc_mc_sweep_deal_host", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, _u64p, _u64p, _ip])


class McStrataCfg(C.Structure):
    _fields_ = [("weights", _ip), ("n_strata", C.c_int), ("design_qber", C.c_double), ("key_bits", C.c_int), ("chunk", C.c_int),
                ("first_frame", C.c_uint64), ("max_frames", C.c_uint64), ("max_frame_errors", C.c_uint64), ("reserved", C.c_int * 2)]


McStrataResult = McSweepResult          # rounds, frames, batches, the stage times; channel_ms is the fixed-weight channel
MC_STRATUM_STAT = np.dtype([("weight", np.int32), ("closed_by", np.int32)] + _MC_ROW_COUNTERS)

_sig("qldpc_mc_weight_frames_host", C.c_int, [C.c_int, C.c_int, _ip, _u8p, C.c_uint64, C.c_double, C.c_uint64, C.c_int, _ip, C.c_int, _up, _up])
_sig("qldpc_mc_weight_frames_dev", C.c_int, [_vp, C.c_uint64, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp])
_sig("qldpc_mc_strata", C.c_int, [_vp, C.POINTER(McStrataCfg), C.POINTER(McStrataResult)])
_sig("qldpc_mc_strata_stats", C.c_int, [_vp, _vp, C.c_int])
_sig("qldpc_mc_strata_hist", C.c_int, [_vp, C.c_int, _u64p, C.c_int])
_sig("qldpc_mc_strata_fer_host", C.c_int, [C.c_int, C.c_int, _ip, _u64p, _u64p, C.c_double, _dp])


class McBlindCfg(C.Structure):
    _fields_ = [("qber", C.c_double), ("ask_bits", C.c_int), ("max_rounds", C.c_int), ("first_frame", C.c_uint64), ("max_frames", C.c_uint64),
                ("max_frame_errors", C.c_uint64), ("reserved", C.c_int * 2)]


class McBlindResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("frames", "frame_errors", "undetected", "open", "disclosed", "decodes", "launches", "next_frame")] + [
        (n, C.c_double) for n in ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "select_ms", "advance_ms", "total_ms")]


# a round's row: the counters of a run's result, in its order, and the key bits asked for
MC_BLIND_ROUND_STAT = np.dtype([(n, np.uint64) for n, _ in McResult._fields_[:9]] + [("disclosed", np.uint64)])
MC_BLIND_MAX_ROUNDS = 64

_sig("qldpc_mc_blind", C.c_int, [_vp, C.POINTER(McBlindCfg), C.POINTER(McBlindResult)])
_sig("qldpc_mc_blind_stats", C.c_int, [_vp, _vp, C.c_int])
_sig("qldpc_mc_blind_open", C.c_int, [_vp, _u64p, _up, C.c_int])
_sig("qldpc_mc_blind_next_host", C.c_int, [C.c_int, C.c_int, _u64p, C.c_uint64, _ip, _ip])
_sig("qldpc_mc_blind_efficiency_host", C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_double, _dp])


class McGuessCfg(C.Structure):
    _fields_ = [("qber", C.c_double), ("guess_bits", C.c_int), ("first_frame", C.c_uint64), ("max_frames", C.c_uint64), ("max_frame_errors", C.c_uint64),
                ("reserved", C.c_int * 2)]


class McGuessResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("frames", "frame_errors", "undetected", "rescued", "open", "trials", "trial_iter_sum", "n_ok_sum", "ambiguous", "decodes",
                                          "launches", "next_frame")] + [
        (n, C.c_double) for n in ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "select_ms", "advance_ms", "expand_ms", "pick_ms", "total_ms")]


GUESS_MAX_BITS = 10
MC_GUESS_FRESH, MC_GUESS_TRIALS = 1, 2          # kind of a launch of mc_guess_next
MC_GUESS_ROWS = ("closed", "rescued", "open")   # the three MC_BLIND_ROUND_STAT rows of MonteCarlo.guess, disclosed = 0

_sig("qldpc_guess_expand_dev", C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_guess_pick_dev", C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_guess_trial_host", C.c_int, [C.c_int, C.c_int, C.c_int, _up, _up, _up, _up])
_sig("qldpc_guess_pick_host", C.c_int, [C.c_int, C.c_int, _ip, _up, _ip, _ip, _ip])
_sig("qldpc_mc_guess", C.c_int, [_vp, C.POINTER(McGuessCfg), C.POINTER(McGuessResult)])
_sig("qldpc_mc_guess_stats", C.c_int, [_vp, _vp, C.c_int])
_sig("qldpc_mc_guess_open", C.c_int, [_vp, _u64p, _up, C.c_int])
_sig("qldpc_mc_guess_next_host", C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_uint64, _ip, _ip])


class McChannel(C.Structure):
    _fields_ = [("levels", C.c_int), ("cum", _u64p * 2), ("value", C.POINTER(C.c_float)), ("reserved", C.c_int * 2)]


MC_SOURCE = {"random": 0, "zero": 1}
_sig("qldpc_mc_set_channel", C.c_int, [_vp, C.POINTER(McChannel)])
_sig("qldpc_mc_set_source", C.c_int, [_vp, C.c_int])
_sig("qldpc_mc_awgn_table", C.c_int, [C.c_double, C.c_double, C.c_int, _u64p, _u64p, _fp])
_sig("qldpc_mc_llr_host", C.c_int, [C.c_int, C.c_int, _ip, _u8p, C.c_uint64, C.c_double, C.POINTER(McChannel), _up, C.c_uint64, C.c_int, _fp, _up])
_sig("qldpc_mc_llr_dev", C.c_int, [_vp, C.c_uint64, C.c_int, _vp, _vp, _vp, _vp])


class McTablePoint(C.Structure):
    _fields_ = [("table", McChannel), ("label", C.c_double), ("n_punct", C.c_int), ("reserved", C.c_int)]


class McSweepTablesCfg(C.Structure):
    _fields_ = [("points", C.POINTER(McTablePoint)), ("n_points", C.c_int), ("punct_order", _ip), ("n_order", C.c_int), ("chunk", C.c_int),
                ("first_frame", C.c_uint64), ("max_frames", C.c_uint64), ("max_frame_errors", C.c_uint64), ("reserved", C.c_int * 2)]


_sig("qldpc_mc_sweep_tables", C.c_int, [_vp, C.POINTER(McSweepTablesCfg), C.POINTER(McSweepResult)])
_sig("qldpc_mc_sweep_tables_check_host", C.c_int, [C.c_int, C.c_int, C.POINTER(McSweepTablesCfg)])


def mc_philox_host(counter, key):
    """Philox4x32-10 of a (counter[4], key[2]) -> 4 uint32 words (host mirror of the kernels' generator)"""
    c = np.ascontiguousarray(counter, dtype=np.uint32).ravel()
    k = np.ascontiguousarray(key, dtype=np.uint32).ravel()
    if c.size != 4 or k.size != 2:
        raise QldpcError(-6, "mc_philox_host: %d counter words, %d key words" % (c.size, k.size))
    out = np.empty(4, np.uint32)
    _chk(_L.qldpc_mc_philox_host(c.ctypes.data_as(_up), k.ctypes.data_as(_up), out.ctypes.data_as(_up)), "mc_philox_host")
    return out


def _mc_class_arg(vn_class, N, where):
    if vn_class is None:
        return None
    cls = np.ascontiguousarray(vn_class, dtype=np.uint8).ravel()
    if cls.size != N:
        raise QldpcError(-6, "%s: %d VN classes, N = %d" % (where, cls.size, N))
    return cls


def _u64(x):
    return int(x) & 0xFFFFFFFFFFFFFFFF


def _fields(res):
    return {name: getattr(res, name) for name, _ in res._fields_}


def _mc_host_args(K, N, n_frames, info_bits_pos, vn_class, where):
    """the prologue of the host mirrors -> (K, N, n, pos, cls, zeroed info words [n, ceil(K/32)], zeroed word rows [n, ceil(N/32)])"""
    K, N, n = int(K), int(N), int(n_frames)
    pos = None
    if info_bits_pos is not None:
        pos = _np_i32(info_bits_pos).ravel()
        if pos.size != K:
            raise QldpcError(-6, "%s: len(info_bits_pos) != K" % where)
    cls = _mc_class_arg(vn_class, N, where)
    return K, N, n, pos, cls, np.zeros((max(n, 0), (max(K, 0) + 31) // 32), np.uint32), np.zeros((max(n, 0), (max(N, 0) + 31) // 32), np.uint32)


def mc_frames_host(K, N, seed, qber, first_frame, n_frames, info_bits_pos=None, vn_class=None, parity_ber=0.0):
    """Frames [first_frame, first_frame + n_frames) of the Monte-Carlo frame definition on the host, no device needed ->
    (info words [n, ceil(K/32)], flip words [n, ceil(N/32)]), uint32, MSB-first.  vn_class None: QLDPC_VN_CHANNEL at info_bits_pos
    (None = 0 .. K-1), QLDPC_VN_PINNED elsewhere."""
    K, N, n, pos, cls, info, flips = _mc_host_args(K, N, n_frames, info_bits_pos, vn_class, "mc_frames_host")
    _chk(_L.qldpc_mc_frames_host(K, N, _ptr(pos, _ip), _ptr(cls, _u8p), _u64(seed), float(qber), float(parity_ber), _u64(first_frame), n,
                                 info.ctypes.data_as(_up), flips.ctypes.data_as(_up)), "mc_frames_host")
    return info, flips


def mc_pattern_host(seed, pattern, n_cand, n_punct, key_bits=32):
    """Puncture pattern `pattern` of the Monte-Carlo pattern definition on the host, no device needed -> the n_punct chosen candidate
    indices (into an ascending candidate list of n_cand entries), ascending, int32.  key_bits below 32 coarsens the keys (tests only)."""
    idx = np.full(max(int(n_punct), 0), -1, np.int32)
    _chk(_L.qldpc_mc_pattern_host(_u64(seed), _u64(pattern), int(n_cand), int(n_punct), int(key_bits),
                                  idx.ctypes.data_as(_ip)), "mc_pattern_host")
    return idx


def mc_sweep_deal(done, frame_errors, chunk, slots, max_frames, max_frame_errors=0):
    """the deal of one round of MonteCarlo.sweep (qldpc_mc_sweep_deal_host, no device needed): done[P] and frame_errors[P] of the points ->
    give[P] (int32), the chunks of `chunk` frames each point receives out of `slots`"""
    d = np.ascontiguousarray(done, dtype=np.uint64).ravel()
    fe = np.ascontiguousarray(frame_errors, dtype=np.uint64).ravel()
    if d.size != fe.size:
        raise QldpcError(-6, "mc_sweep_deal: %d done counts, %d frame-error counts" % (d.size, fe.size))
    give = np.zeros(d.size, np.int32)
    used = _chk(_L.qldpc_mc_sweep_deal_host(d.size, int(chunk), int(slots), int(max_frames), int(max_frame_errors), d.ctypes.data_as(_u64p),
                                            fe.ctypes.data_as(_u64p), give.ctypes.data_as(_ip)), "mc_sweep_deal")
    assert used == int(give.sum())
    return give


def mc_weight_frames_host(K, N, seed, weights, first_frame, n_frames, key_bits=0, info_bits_pos=None, vn_class=None, parity_ber=0.0):
    """Frames [first_frame, first_frame + n_frames) of the fixed-weight frame definition on the host, no device needed: frame f flips the
    weights[f] channel VNs with the smallest stream-1 words (a scalar `weights` stands for every frame) -> (info words [n, ceil(K/32)],
    flip words [n, ceil(N/32)]), uint32, MSB-first.  key_bits below 32 coarsens the keys (tests only); the classes as mc_frames_host."""
    K, N, n, pos, cls, info, flips = _mc_host_args(K, N, n_frames, info_bits_pos, vn_class, "mc_weight_frames_host")
    w = np.full(max(n, 0), int(weights), np.int32) if np.ndim(weights) == 0 else _np_i32(weights).ravel()
    if w.size != max(n, 0):
        raise QldpcError(-6, "mc_weight_frames_host: %d weights for %d frames" % (w.size, n))
    _chk(_L.qldpc_mc_weight_frames_host(K, N, _ptr(pos, _ip), _ptr(cls, _u8p), _u64(seed), float(parity_ber), _u64(first_frame), n, w.ctypes.data_as(_ip),
                                        int(key_bits), info.ctypes.data_as(_up), flips.ctypes.data_as(_up)), "mc_weight_frames_host")
    return info, flips


def mc_strata_fer(n_channel, weights, frames, frame_errors, qber):
    """FER(qber) of a BSC over n_channel channel VNs from fixed-weight strata (qldpc_mc_strata_fer_host, no device needed): weights strictly
    ascending, frames and frame_errors per stratum -> float64 [4]: the binomial-weighted failure rate over [w_0, w_last] with P_f linear
    between strata, the binomial mass below w_0, the mass above w_last, the standard error of the first from the sampling of the strata"""
    w = _np_i32(weights).ravel()
    fr = np.ascontiguousarray(frames, dtype=np.uint64).ravel()
    fe = np.ascontiguousarray(frame_errors, dtype=np.uint64).ravel()
    if fr.size != w.size or fe.size != w.size:
        raise QldpcError(-6, "mc_strata_fer: %d weights, %d frame counts, %d frame-error counts" % (w.size, fr.size, fe.size))
    out = np.zeros(4, np.float64)
    _chk(_L.qldpc_mc_strata_fer_host(int(n_channel), w.size, w.ctypes.data_as(_ip), fr.ctypes.data_as(_u64p), fe.ctypes.data_as(_u64p), float(qber),
                                     out.ctypes.data_as(_dp)), "mc_strata_fer")
    return out


def mc_blind_next(pool, input_left, batch):
    """the next launch of MonteCarlo.blind (qldpc_mc_blind_next_host, no device needed): pool[max_rounds + 1] = the entries waiting per level
    (pool[0] is not read) -> (level, n), or None when nothing is left.  The deepest level with pool >= batch, else fresh input, else the
    lowest non-empty level, all of it."""
    pl = np.ascontiguousarray(pool, dtype=np.uint64).ravel()
    if pl.size < 1:
        raise QldpcError(-6, "mc_blind_next: an empty pool vector (max_rounds + 1 counts)")
    level, n = C.c_int(-1), C.c_int(0)
    got = _chk(_L.qldpc_mc_blind_next_host(pl.size - 1, int(batch), pl.ctypes.data_as(_u64p), _u64(input_left), C.byref(level), C.byref(n)), "mc_blind_next")
    return (level.value, n.value) if got else None


def mc_blind_efficiency(n_channel, n_disclosed_parity, frames, disclosed, qber):
    """f = (n_disclosed_parity + disclosed / frames) / (n_channel h2(qber)) (qldpc_mc_blind_efficiency_host, no device needed)"""
    f = C.c_double(0.0)
    _chk(_L.qldpc_mc_blind_efficiency_host(int(n_channel), int(n_disclosed_parity), _u64(frames), _u64(disclosed), float(qber), C.byref(f)), "mc_blind_efficiency")
    return f.value


def mc_guess_next(guess_bits, batch, pool, input_left):
    """the next launch of MonteCarlo.guess (qldpc_mc_guess_next_host, no device needed): pool = the failed first decodes waiting ->
    (MC_GUESS_FRESH, frames) or (MC_GUESS_TRIALS, sources), or None when nothing is left.  A trial launch of S = batch >> guess_bits sources while
    pool >= S, else fresh input, else the flush."""
    kind, n = C.c_int(0), C.c_int(0)
    got = _chk(_L.qldpc_mc_guess_next_host(int(guess_bits), int(batch), _u64(pool), _u64(input_left), C.byref(kind), C.byref(n)), "mc_guess_next")
    return (kind.value, n.value) if got else None


def _guess_row(a, N, where, name):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if int(N) >= 1 and a.shape[-1:] != ((int(N) + 31) // 32,):
        raise QldpcError(-6, "%s: %s has rows of %s words, ceil(N/32) = %d" % (where, name, a.shape[-1:], (int(N) + 31) // 32))
    return a


def guess_trial_host(N, g, t, weak, hard):
    """the known and value rows of trial t of one failed frame on the host (qldpc_guess_trial_host): weak = its guess row, hard = its
    hard-decision row, ceil(N/32) uint32 words MSB-first -> (known row, value row)"""
    weak, hard = _guess_row(weak, N, "guess_trial_host", "weak").ravel(), _guess_row(hard, N, "guess_trial_host", "hard").ravel()
    known, value = np.zeros_like(weak), np.zeros_like(weak)
    _chk(_L.qldpc_guess_trial_host(int(N), int(g), int(t), weak.ctypes.data_as(_up), hard.ctypes.data_as(_up), known.ctypes.data_as(_up),
                                   value.ctypes.data_as(_up)), "guess_trial_host")
    return known, value


def guess_pick_host(N, g, ok, trial_hard):
    """the verdict over the 2^g trials of one failed frame on the host (qldpc_guess_pick_host): ok [2^g], trial_hard [2^g, ceil(N/32)] ->
    (winner or -1, n_ok, ambiguous)"""
    ok = np.ascontiguousarray(ok, dtype=np.int32).ravel()
    rows = _guess_row(trial_hard, N, "guess_pick_host", "trial_hard")
    if 0 <= int(g) <= GUESS_MAX_BITS and (ok.size != 1 << int(g) or rows.ndim != 2 or rows.shape[0] != ok.size):
        raise QldpcError(-6, "guess_pick_host: %d flags and rows %s for %d trials" % (ok.size, rows.shape, 1 << int(g)))
    w, n, a = C.c_int(-2), C.c_int(-2), C.c_int(-2)
    _chk(_L.qldpc_guess_pick_host(int(N), int(g), ok.ctypes.data_as(_ip), rows.ctypes.data_as(_up), C.byref(w), C.byref(n), C.byref(a)), "guess_pick_host")
    return w.value, n.value, a.value


def _guess_dev(t, rows, cols, where, name):
    torch = _torch()
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == ((rows, cols) if cols else (rows,))):
        raise QldpcError(-6, "%s: %s must be a contiguous device int32 tensor of shape %s" % (where, name, (rows, cols) if cols else (rows,)))
    return _vp(t.data_ptr())


def guess_expand(N, g, weak, hard, stream=None):
    """qldpc_guess_expand_dev: weak, hard device int32 [n_src, ceil(N/32)] -> (known, value) device int32 [n_src 2^g, ceil(N/32)], trial slot
    s 2^g + t, what Decoder.load_known takes; asynchronous on `stream` (default: torch's current stream)"""
    torch = _torch()
    N, g, n, W = int(N), int(g), int(weak.shape[0]), (int(N) + 31) // 32
    _guess_dev(weak, n, W, "guess_expand", "weak"), _guess_dev(hard, n, W, "guess_expand", "hard")
    slots = n << g if 0 <= g <= GUESS_MAX_BITS and n << g <= 1 << 24 else 0      # a refused call writes nothing
    known = torch.zeros((slots, W), dtype=torch.int32, device=weak.device)
    value = torch.zeros_like(known)
    spare = torch.zeros(1, dtype=torch.int32, device=weak.device)                # an empty tensor has no address, and the call checks its pointers first
    ptr = lambda t: _vp(t.data_ptr() if t.numel() else spare.data_ptr())
    s = _stream_arg(stream, weak.device)
    with torch.cuda.device(weak.device):
        _chk(_L.qldpc_guess_expand_dev(N, g, n, ptr(weak), ptr(hard), ptr(known), ptr(value), s), "guess_expand")
    return known, value


def guess_pick(N, g, ok, trial_hard, out_hard, stream=None):
    """qldpc_guess_pick_dev: ok device int32 [n_src 2^g], trial_hard device int32 [n_src 2^g, ceil(N/32)] -> (winner, n_ok, ambiguous) device
    int32 [n_src]; the winner's row is copied into out_hard [n_src, ceil(N/32)], the row of a source without a winner is left as it is;
    asynchronous on `stream` (default: torch's current stream)"""
    torch = _torch()
    N, g, n, W = int(N), int(g), int(out_hard.shape[0]), (int(N) + 31) // 32
    slots = n << g if 0 <= g <= GUESS_MAX_BITS else int(ok.shape[0])
    op, rp = _guess_dev(ok, slots, 0, "guess_pick", "ok"), _guess_dev(trial_hard, slots, W, "guess_pick", "trial_hard")
    hp = _guess_dev(out_hard, n, W, "guess_pick", "out_hard")
    win, nok, amb = (torch.full((n,), -2, dtype=torch.int32, device=out_hard.device) for _ in range(3))
    s = _stream_arg(stream, out_hard.device)
    with torch.cuda.device(out_hard.device):
        _chk(_L.qldpc_guess_pick_dev(N, g, n, op, rp, _vp(win.data_ptr()), _vp(nok.data_ptr()), _vp(amb.data_ptr()), hp, s), "guess_pick")
    return win, nok, amb


def _mc_channel_arg(cum0, cum1, value, where):
    """-> (McChannel, the arrays it points into): levels = len(value), the rows uint64 of levels - 1 entries"""
    c0, c1 = (np.ascontiguousarray(c, dtype=np.uint64).ravel() for c in (cum0, cum1))
    val = np.ascontiguousarray(value, dtype=np.float32).ravel()
    if c0.size != c1.size or c0.size + 1 != val.size:
        raise QldpcError(-6, "%s: %d and %d thresholds for %d levels" % (where, c0.size, c1.size, val.size))
    t = McChannel()
    t.levels = val.size
    t.cum[0], t.cum[1], t.value = c0.ctypes.data_as(_u64p), c1.ctypes.data_as(_u64p), val.ctypes.data_as(_fp)
    return t, (c0, c1, val)


def mc_awgn_sigma(ebno_db, rate):
    """the noise deviation of BPSK at Eb/N0 (dB) and code rate `rate`: sqrt(1 / (2 rate 10^(ebno_db / 10)))"""
    return float(np.sqrt(1.0 / (2.0 * float(rate) * 10.0 ** (float(ebno_db) / 10.0))))


def mc_awgn_table(sigma, rmax=3.0, maxq=31):
    """The threshold table of BPSK over AWGN quantised to floor(r / rmax * maxq), clamped to [-maxq - 1, maxq] (host only) ->
    (cum0, cum1 [2 maxq + 1] uint64, value [2 maxq + 2] float32 = -maxq - 1 .. maxq): what MonteCarlo.set_channel takes"""
    q = 2 * int(maxq) + 2
    c0, c1, val = np.zeros(max(q - 1, 1), np.uint64), np.zeros(max(q - 1, 1), np.uint64), np.zeros(max(q, 1), np.float32)
    _chk(_L.qldpc_mc_awgn_table(float(sigma), float(rmax), int(maxq), c0.ctypes.data_as(_u64p), c1.ctypes.data_as(_u64p), val.ctypes.data_as(_fp)), "mc_awgn_table")
    return c0, c1, val


def mc_llr_host(K, N, seed, table, first_frame, n_frames, cw_words=None, info_bits_pos=None, vn_class=None, parity_ber=0.0):
    """Frames [first_frame, first_frame + n_frames) of the quantised-channel definition on the host, no device needed: table =
    (cum0, cum1, value), cw_words [n, ceil(N/32)] the packed codewords (None = all-zero) -> (LLRs [n, N] float32, flip words
    [n, ceil(N/32)] uint32: the VNs whose LLR sign contradicts the codeword bit)"""
    K, N, n, pos, cls, _, flips = _mc_host_args(K, N, n_frames, info_bits_pos, vn_class, "mc_llr_host")
    t, keep = _mc_channel_arg(*table, "mc_llr_host")
    cw = None
    if cw_words is not None:
        cw = np.ascontiguousarray(cw_words, dtype=np.uint32)
        if cw.shape != flips.shape:
            raise QldpcError(-6, "mc_llr_host: codeword words %s, expected (%d, %d)" % (cw.shape, n, flips.shape[1]))
    llr = np.zeros((max(n, 0), max(N, 0)), np.float32)
    _chk(_L.qldpc_mc_llr_host(K, N, _ptr(pos, _ip), _ptr(cls, _u8p), _u64(seed), float(parity_ber), C.byref(t), _ptr(cw, _up), _u64(first_frame), n,
                              llr.ctypes.data_as(_fp), flips.ctypes.data_as(_up)), "mc_llr_host")
    del keep
    return llr, flips


def _mc_sweep_tables_cfg(tables, labels, n_punct, punct_order, first_frame, max_frames, max_frame_errors, chunk, where):
    """-> (McSweepTablesCfg, everything it points into): tables = a sequence of (cum0, cum1, value), labels and n_punct one entry per table
    (None = 0.0 / 0)"""
    tables = list(tables)
    P = len(tables)
    lab = np.zeros(P, np.float64) if labels is None else np.ascontiguousarray(labels, dtype=np.float64).ravel()
    npn = np.zeros(P, np.int32) if n_punct is None else _np_i32(n_punct).ravel()
    if lab.size != P or npn.size != P:
        raise QldpcError(-6, "%s: %d tables, %d labels, %d n_punct" % (where, P, lab.size, npn.size))
    pts, keep = (McTablePoint * max(P, 1))(), []
    for i, t in enumerate(tables):
        ch, arrays = _mc_channel_arg(*t, where)
        pts[i].table, pts[i].label, pts[i].n_punct = ch, float(lab[i]), int(npn[i])
        keep.append(arrays)
    order = _np_i32(punct_order).ravel() if punct_order is not None else np.zeros(0, np.int32)
    cfg = McSweepTablesCfg()
    cfg.points, cfg.n_points = pts, P
    cfg.punct_order, cfg.n_order = (order.ctypes.data_as(_ip) if order.size else None), order.size
    cfg.chunk, cfg.first_frame = int(chunk), _u64(first_frame)
    cfg.max_frames, cfg.max_frame_errors = int(max_frames), int(max_frame_errors)
    return cfg, (pts, keep, order)


def mc_sweep_tables_check(N, batch, tables, labels=None, n_punct=None, punct_order=None, first_frame=0, max_frames=1, max_frame_errors=0, chunk=0):
    """every argument check of MonteCarlo.sweep_tables for a code of N VNs and this batch, no device needed: raises what the call would raise"""
    cfg, keep = _mc_sweep_tables_cfg(tables, labels, n_punct, punct_order, first_frame, max_frames, max_frame_errors, chunk, "mc_sweep_tables_check")
    _chk(_L.qldpc_mc_sweep_tables_check_host(int(N), int(batch), C.byref(cfg)), "mc_sweep_tables_check")
    del keep


class MonteCarlo(_Handle):
    """The harness's loop source -> encoder -> BSC -> decoder -> monitor on the device (qldpc_mc_*), around a Decoder and an Encoder of
    the same code, which it keeps alive but does not own.  Frame i is a pure function of (seed, i): run() over [first_frame, first_frame +
    max_frames) gives the same counters whatever the batch, and ranges add up."""
    _free = _L.qldpc_mc_free

    def __init__(self, decoder, encoder, vn_class=None, seed=0, batch=0, parity_ber=0.0, fail_cap=1024):
        cfg = _default(McCfg, _L.qldpc_mc_cfg_default)
        cfg.seed, cfg.batch, cfg.fail_cap, cfg.parity_ber = _u64(seed), int(batch), int(fail_cap), float(parity_ber)
        cls = _mc_class_arg(vn_class, decoder.N, "MonteCarlo")
        self._h = _create("MonteCarlo", _L.qldpc_mc_create, decoder._h, encoder._h, _ptr(cls, _u8p), C.byref(cfg))
        self.decoder, self.encoder = decoder, encoder
        self.N, self.K, self.device = decoder.N, decoder.K, decoder.device
        self.seed, self.batch, self.fail_cap, self.parity_ber = int(seed), int(batch) or decoder.max_frames, int(fail_cap), float(parity_ber)

    @property
    def device_bytes(self):
        return int(_L.qldpc_mc_device_bytes(self._h))

    def run(self, qber, first_frame=0, max_frames=None, max_frame_errors=0):
        """-> dict of the counters (frames, bit_errors, frame_errors, undetected, not_converged, iter_sum, iter_max, channel_flips,
        channel_bits, batches, next_frame, decode_ms and the other stages' source_ms .. monitor_ms by hipEvents, total_ms).  Stops at the first batch boundary with frame_errors >= max_frame_errors
        (0 = never) or after max_frames (None = one batch)."""
        res = McResult()
        n = self.batch if max_frames is None else int(max_frames)
        _chk(_L.qldpc_mc_run(self._h, float(qber), _u64(first_frame), n, int(max_frame_errors), C.byref(res)), "MonteCarlo.run")
        return _fields(res)

    def _frame_tensors(self, n):
        """-> empty device int32 tensors info [n, ceil(K/32)], cw [n, ceil(N/32)], rx [n, ceil(N/32)]"""
        torch = _torch()
        info = _dev_empty(self.device, (n, (self.K + 31) // 32), torch.int32)
        cw = _dev_empty(self.device, (n, (self.N + 31) // 32), torch.int32)
        return info, cw, torch.empty_like(cw)

    def frames(self, first_frame, n_frames, qber):
        """the source alone -> device int32 tensors (info [n, ceil(K/32)], cw [n, ceil(N/32)], rx [n, ceil(N/32)]): what
        mc_frames_host gives, the codeword by the encoder, rx = cw ^ flips"""
        n = int(n_frames)
        info, cw, rx = self._frame_tensors(n)
        _chk(_L.qldpc_mc_frames_dev(self._h, _u64(first_frame), n, float(qber), _vp(info.data_ptr()), _vp(cw.data_ptr()),
                                    _vp(rx.data_ptr())), "MonteCarlo.frames")
        self.decoder.sync()
        return info, cw, rx

    def set_channel(self, cum0=None, cum1=None, value=None):
        """A quantised soft-output channel in place of the BSC: level = #{k : u >= cum[b][k]} of the VN's stream-3 word u and codeword bit
        b, LLR = value[level] (include/qldpc.h).  run() and search() then ignore their qber (it is still validated).  None returns to the BSC."""
        if cum0 is None and cum1 is None and value is None:
            _chk(_L.qldpc_mc_set_channel(self._h, None), "MonteCarlo.set_channel")
            return
        t, keep = _mc_channel_arg(cum0, cum1, value, "MonteCarlo.set_channel")
        _chk(_L.qldpc_mc_set_channel(self._h, C.byref(t)), "MonteCarlo.set_channel")
        del keep

    def set_awgn(self, sigma=None, rmax=3.0, maxq=31, ebno_db=None, rate=None):
        """BPSK over AWGN quantised to 2 maxq + 2 levels (mc_awgn_table): sigma, or ebno_db together with rate -> sigma"""
        if (sigma is None) == (ebno_db is None) or (ebno_db is not None and rate is None):
            raise QldpcError(-1, "MonteCarlo.set_awgn: sigma, or ebno_db together with rate")
        if sigma is None:
            sigma = mc_awgn_sigma(ebno_db, rate)
        self.set_channel(*mc_awgn_table(sigma, rmax, maxq))
        return float(sigma)

    def set_source(self, mode):
        """"random" (the default) or "zero": all-zero info words, hence the all-zero codeword"""
        if mode not in MC_SOURCE:
            raise QldpcError(-1, "MonteCarlo.set_source: %r is neither 'random' nor 'zero'" % (mode,))
        _chk(_L.qldpc_mc_set_source(self._h, MC_SOURCE[mode]), "MonteCarlo.set_source")

    def llr_frames(self, first_frame, n_frames):
        """the frames of the table that is set -> device tensors (info [n, ceil(K/32)], cw [n, ceil(N/32)], rx [n, ceil(N/32)] int32 and
        llr [n, N] float32): the LLR rows and rx ^ cw are what mc_llr_host gives for the encoder's codewords"""
        n = int(n_frames)
        info, cw, rx = self._frame_tensors(n)
        llr = _dev_empty(cw.device, (n, self.N), _torch().float32)
        _chk(_L.qldpc_mc_llr_dev(self._h, _u64(first_frame), n, _vp(info.data_ptr()), _vp(cw.data_ptr()), _vp(rx.data_ptr()),
                                 _vp(llr.data_ptr())), "MonteCarlo.llr_frames")
        self.decoder.sync()
        return info, cw, rx, llr

    def iter_hist(self):
        """frames per iteration count of the last run, n_ite + 1 bins (uint64)"""
        out = np.zeros(1, np.uint64)
        bins = _chk(_L.qldpc_mc_iter_hist(self._h, out.ctypes.data_as(_u64p), 1), "MonteCarlo.iter_hist")      # the call returns n_ite + 1
        if bins > 1:
            out = np.zeros(bins, np.uint64)
            _chk(_L.qldpc_mc_iter_hist(self._h, out.ctypes.data_as(_u64p), bins), "MonteCarlo.iter_hist")
        return out

    def failed_frames(self):
        """global indices of the failed frames of the last run that were kept (the first fail_cap), ascending (uint64)"""
        out = np.zeros(self.fail_cap, np.uint64)
        n = _chk(_L.qldpc_mc_failed_frames(self._h, out.ctypes.data_as(_u64p), out.size), "MonteCarlo.failed_frames")
        return out[:n].copy()

    def set_candidates(self, vn=None):
        """the VNs a pattern may puncture: ascending, distinct, inside [0, N); None = every VN_PINNED VN of the class map"""
        if vn is None:
            _chk(_L.qldpc_mc_set_candidates(self._h, None, 0), "MonteCarlo.set_candidates")
            return
        v = _np_i32(vn).ravel()
        _chk(_L.qldpc_mc_set_candidates(self._h, v.ctypes.data_as(_ip), v.size), "MonteCarlo.set_candidates")

    def patterns(self, first_pattern, n_patterns, n_punct, key_bits=32):
        """erase rows of patterns [first_pattern, first_pattern + n_patterns) -> device int32 tensor [n, ceil(N/32)], MSB-first"""
        n = int(n_patterns)
        rows = _dev_empty(self.device, (max(n, 0), (self.N + 31) // 32), _torch().int32)
        _chk(_L.qldpc_mc_patterns_dev(self._h, _u64(first_pattern), n, int(n_punct), int(key_bits), _vp(rows.data_ptr())),
             "MonteCarlo.patterns")
        self.decoder.sync()
        return rows

    def pattern_vns(self, pattern, n_punct, key_bits=32):
        """the VNs pattern `pattern` punctures, ascending (int32)"""
        vn = np.full(max(int(n_punct), 0), -1, np.int32)
        _chk(_L.qldpc_mc_pattern_vns(self._h, _u64(pattern), int(n_punct), int(key_bits), vn.ctypes.data_as(_ip)), "MonteCarlo.pattern_vns")
        return vn

    def set_puncture(self, vn):
        """a fixed puncture set for run(): these VNs (ascending, distinct) are erased in every frame; an empty list clears it"""
        v = _np_i32(vn).ravel() if vn is not None else np.zeros(0, np.int32)
        _chk(_L.qldpc_mc_set_puncture(self._h, v.ctypes.data_as(_ip), v.size), "MonteCarlo.set_puncture")

    def search(self, qber, n_punct, frames_per_pattern, first_pattern=0, max_patterns=None, stop_at_goal=True, first_frame=0, key_bits=32):
        """Patterns [first_pattern, first_pattern + max_patterns) (None = one round), each over its own frames_per_pattern frames
        first_frame + p F + k, floor(batch / F) patterns per decoder launch -> dict of the result (patterns, frames, batches, goal, best,
        best_frame_errors, best_bit_errors, next_pattern, the stage times) plus `stats`, one MC_PATTERN_STAT row per evaluated pattern.
        goal / best are MC_NO_PATTERN where there is none.  With stop_at_goal the search ends after the first round that holds a
        pattern without frame errors."""
        cfg = McSearchCfg()
        cfg.n_punct, cfg.frames_per_pattern, cfg.key_bits, cfg.stop_at_goal = int(n_punct), int(frames_per_pattern), int(key_bits), int(bool(stop_at_goal))
        cfg.first_frame = _u64(first_frame)
        if max_patterns is None:
            max_patterns = self.batch // max(int(frames_per_pattern), 1) if 1 <= int(frames_per_pattern) <= self.batch else 1
        res = McSearchResult()
        _chk(_L.qldpc_mc_search(self._h, float(qber), C.byref(cfg), _u64(first_pattern), int(max_patterns), C.byref(res)), "MonteCarlo.search")
        out = _fields(res)
        stats = np.zeros(int(res.patterns), MC_PATTERN_STAT)
        n = _chk(_L.qldpc_mc_search_stats(self._h, _vp(stats.ctypes.data), stats.size), "MonteCarlo.search")
        assert n == stats.size
        out["stats"] = stats
        return out

    def sweep(self, qbers, n_punct=None, punct_order=None, first_frame=0, max_frames=None, max_frame_errors=0, chunk=0):
        """P operating points side by side in one batch (qldpc_mc_sweep): point q = (qbers[q], n_punct[q]) erases the first n_punct[q] VNs
        of punct_order on top of set_puncture's set; frame k of every point is frame first_frame + k; a point closes at max_frames (None = one
        batch) or at max_frame_errors (0 = never), and its lanes pass to the open points, `chunk` frames at a time (0 = min(64, batch)).
        -> dict of the result (rounds, frames, batches, the stage times) plus `points`, one MC_POINT_STAT row per point: exactly the
        counters of run(qbers[q], first_frame, frames_q) with that point's puncture set."""
        qb = np.ascontiguousarray(qbers, dtype=np.float64).ravel()
        npn = np.zeros(qb.size, np.int32) if n_punct is None else _np_i32(n_punct).ravel()
        if npn.size != qb.size:
            raise QldpcError(-6, "MonteCarlo.sweep: %d qbers, %d n_punct" % (qb.size, npn.size))
        pts = (McPoint * max(qb.size, 1))()
        for i in range(qb.size):
            pts[i].qber, pts[i].n_punct = float(qb[i]), int(npn[i])
        order = _np_i32(punct_order).ravel() if punct_order is not None else np.zeros(0, np.int32)
        cfg = McSweepCfg()
        cfg.points, cfg.n_points = pts, qb.size
        cfg.punct_order, cfg.n_order = (order.ctypes.data_as(_ip) if order.size else None), order.size
        cfg.chunk, cfg.first_frame = int(chunk), _u64(first_frame)
        cfg.max_frames, cfg.max_frame_errors = (self.batch if max_frames is None else int(max_frames)), int(max_frame_errors)
        res = McSweepResult()
        _chk(_L.qldpc_mc_sweep(self._h, C.byref(cfg), C.byref(res)), "MonteCarlo.sweep")
        out = _fields(res)
        out["points"] = self.sweep_stats()
        assert out["points"].size == qb.size
        return out

    def sweep_tables(self, tables, labels=None, n_punct=None, punct_order=None, first_frame=0, max_frames=None, max_frame_errors=0, chunk=0):
        """P operating points of table channels side by side in one batch (qldpc_mc_sweep_tables): point q draws its frames through
        tables[q] = (cum0, cum1, value), as set_channel takes them, and erases the first n_punct[q] VNs of punct_order on top of set_puncture's
        set; everything else is sweep()'s.  labels[q] (None = 0.0) is the caller's name of the point and comes back in the `qber` field of its
        row.  -> dict of the result plus `points`: exactly the counters of set_channel(*tables[q]) + run(., first_frame, frames_q) with that
        point's puncture set.  The table of set_channel, in force or not, is neither needed nor changed."""
        cfg, keep = _mc_sweep_tables_cfg(tables, labels, n_punct, punct_order, first_frame, self.batch if max_frames is None else max_frames,
                                         max_frame_errors, chunk, "MonteCarlo.sweep_tables")
        res = McSweepResult()
        _chk(_L.qldpc_mc_sweep_tables(self._h, C.byref(cfg), C.byref(res)), "MonteCarlo.sweep_tables")
        out = _fields(res)
        out["points"] = self.sweep_stats()
        assert out["points"].size == cfg.n_points
        del keep
        return out

    def sweep_awgn(self, ebno_dbs, rate, rmax=3.0, maxq=31, **kw):
        """sweep_tables over BPSK over AWGN at the Eb/N0 values ebno_dbs (dB) and code rate `rate`, each quantised to 2 maxq + 2 levels
        (mc_awgn_sigma, mc_awgn_table), labelled with its Eb/N0; kw = the other arguments of sweep_tables"""
        db = np.ascontiguousarray(ebno_dbs, dtype=np.float64).ravel()
        return self.sweep_tables([mc_awgn_table(mc_awgn_sigma(e, rate), rmax, maxq) for e in db], labels=db, **kw)

    def _last_rows(self, stats_fn, dtype, where):
        n = _chk(stats_fn(self._h, None, 0), where)
        rows = np.zeros(n, dtype)
        if n:
            _chk(stats_fn(self._h, _vp(rows.ctypes.data), n), where)
        return rows

    def _last_hists(self, stats_fn, hist_fn, where):
        P = _chk(stats_fn(self._h, None, 0), where)
        if P == 0:
            return np.zeros((0, 0), np.uint64)
        one = np.zeros(1, np.uint64)
        bins = _chk(hist_fn(self._h, 0, one.ctypes.data_as(_u64p), 1), where)      # the call returns n_ite + 1
        out = np.zeros((P, bins), np.uint64)
        for q in range(P):
            _chk(hist_fn(self._h, q, out[q].ctypes.data_as(_u64p), bins), where)
        return out

    def sweep_stats(self):
        """the point rows of the last sweep (MC_POINT_STAT), in point order"""
        return self._last_rows(_L.qldpc_mc_sweep_stats, MC_POINT_STAT, "MonteCarlo.sweep_stats")

    def sweep_hist(self):
        """frames per iteration count of every point of the last sweep -> uint64 [P, n_ite + 1]"""
        return self._last_hists(_L.qldpc_mc_sweep_stats, _L.qldpc_mc_sweep_hist, "MonteCarlo.sweep_hist")

    def weight_frames(self, first_frame, n_frames, weight, key_bits=0):
        """the source alone at one fixed error weight -> device int32 tensors (info [n, ceil(K/32)], cw [n, ceil(N/32)], rx [n, ceil(N/32)]):
        what mc_weight_frames_host gives, the codeword by the encoder, rx = cw ^ flips"""
        n = int(n_frames)
        info, cw, rx = self._frame_tensors(max(n, 0))
        _chk(_L.qldpc_mc_weight_frames_dev(self._h, _u64(first_frame), n, int(weight), int(key_bits), _vp(info.data_ptr()), _vp(cw.data_ptr()),
                                           _vp(rx.data_ptr())), "MonteCarlo.weight_frames")
        self.decoder.sync()
        return info, cw, rx

    def strata(self, weights, design_qber, first_frame=0, max_frames=None, max_frame_errors=0, chunk=0, key_bits=0):
        """Fixed error weights side by side in one batch (qldpc_mc_strata): stratum s flips exactly weights[s] channel VNs of every frame, the
        ones with the smallest channel words, and is decoded with |LLR| = bsc_llr(design_qber); frame k of every stratum is frame
        first_frame + k; a stratum closes at max_frames (None = one batch) or at max_frame_errors (0 = never), and its lanes pass to the open
        ones, `chunk` frames at a time (0 = min(64, batch)) -> dict of the result (rounds, frames, batches, the stage times) plus `strata`,
        one MC_STRATUM_STAT row per weight in the caller's order.  mc_strata_fer turns the rows into FER(q) for any q."""
        w = _np_i32(weights).ravel()
        cfg = McStrataCfg()
        cfg.weights, cfg.n_strata = (w.ctypes.data_as(_ip) if w.size else None), w.size
        cfg.design_qber, cfg.key_bits, cfg.chunk = float(design_qber), int(key_bits), int(chunk)
        cfg.first_frame = _u64(first_frame)
        cfg.max_frames, cfg.max_frame_errors = (self.batch if max_frames is None else int(max_frames)), int(max_frame_errors)
        res = McStrataResult()
        _chk(_L.qldpc_mc_strata(self._h, C.byref(cfg), C.byref(res)), "MonteCarlo.strata")
        out = _fields(res)
        out["strata"] = self.strata_stats()
        assert out["strata"].size == w.size
        return out

    def strata_stats(self):
        """the stratum rows of the last strata run (MC_STRATUM_STAT), in the caller's order"""
        return self._last_rows(_L.qldpc_mc_strata_stats, MC_STRATUM_STAT, "MonteCarlo.strata_stats")

    def strata_hist(self):
        """frames per iteration count of every stratum of the last strata run -> uint64 [n_strata, n_ite + 1]"""
        return self._last_hists(_L.qldpc_mc_strata_stats, _L.qldpc_mc_strata_hist, "MonteCarlo.strata_hist")

    def blind(self, qber, ask_bits, max_rounds, first_frame=0, max_frames=None, max_frame_errors=0):
        """Blind reconciliation rounds over the loop's frames (qldpc_mc_blind): a frame whose decode ends with a non-zero syndrome asks for its
        ask_bits weakest unknown channel VNs, gets Alice's bits there and is decoded again, up to max_rounds times; only the frames still open
        are decoded again, pooled per round across batches.  The input ends at max_frames (None = one batch) or at the first launch boundary
        with frame_errors >= max_frame_errors (0 = never); the frames in flight are finished either way.  -> dict of the result (frames,
        frame_errors, undetected, open, disclosed, decodes, launches, next_frame, the stage times) plus `rounds`, max_rounds + 2
        MC_BLIND_ROUND_STAT rows: row r = the frames that closed in round r, the last row = those still open after round max_rounds."""
        cfg = McBlindCfg()
        cfg.qber, cfg.ask_bits, cfg.max_rounds, cfg.first_frame = float(qber), int(ask_bits), int(max_rounds), _u64(first_frame)
        cfg.max_frames, cfg.max_frame_errors = (self.batch if max_frames is None else int(max_frames)), int(max_frame_errors)
        res = McBlindResult()
        _chk(_L.qldpc_mc_blind(self._h, C.byref(cfg), C.byref(res)), "MonteCarlo.blind")
        out = _fields(res)
        out["rounds"] = self.blind_stats()
        assert out["rounds"].size == int(max_rounds) + 2
        return out

    def blind_stats(self):
        """the round rows of the last blind() (MC_BLIND_ROUND_STAT)"""
        return self._last_rows(_L.qldpc_mc_blind_stats, MC_BLIND_ROUND_STAT, "MonteCarlo.blind_stats")

    def blind_open(self):
        """the frames of the last blind() that ended open (the first fail_cap of them), ascending -> (indices uint64 [n], known rows uint32
        [n, ceil(N/32)] MSB-first: everything each of them disclosed)"""
        frames = np.zeros(self.fail_cap, np.uint64)
        known = np.zeros((self.fail_cap, (self.N + 31) // 32), np.uint32)
        n = _chk(_L.qldpc_mc_blind_open(self._h, frames.ctypes.data_as(_u64p), known.ctypes.data_as(_up), self.fail_cap), "MonteCarlo.blind_open")
        return frames[:n].copy(), known[:n].copy()

    def guess(self, qber, guess_bits, first_frame=0, max_frames=None, max_frame_errors=0):
        """Guessing rounds over the loop's frames (qldpc_mc_guess): a frame whose decode ends with a non-zero syndrome is decoded again with its
        guess_bits weakest channel VNs pinned to each of the 2^guess_bits possible values, and is rescued iff a trial ends with a zero syndrome;
        nothing is disclosed.  Failed frames are pooled across batches.  The input ends at max_frames (None = one batch) or at the first launch
        boundary at which the frames closed or rescued wrong plus the open ones reach max_frame_errors (0 = never); the pool is flushed either way.
        -> dict of the result (frames, frame_errors, undetected, rescued, open, trials, trial_iter_sum, n_ok_sum, ambiguous, decodes, launches,
        next_frame, the stage times) plus `rows`, three MC_BLIND_ROUND_STAT rows (MC_GUESS_ROWS: closed at once, rescued -- the winner's decode --,
        open -- the first decode), disclosed = 0."""
        cfg = McGuessCfg()
        cfg.qber, cfg.guess_bits, cfg.first_frame = float(qber), int(guess_bits), _u64(first_frame)
        cfg.max_frames, cfg.max_frame_errors = (self.batch if max_frames is None else int(max_frames)), int(max_frame_errors)
        res = McGuessResult()
        _chk(_L.qldpc_mc_guess(self._h, C.byref(cfg), C.byref(res)), "MonteCarlo.guess")
        out = _fields(res)
        out["rows"] = self.guess_stats()
        assert out["rows"].size == 3
        return out

    def guess_stats(self):
        """the three rows of the last guess() (MC_BLIND_ROUND_STAT)"""
        return self._last_rows(_L.qldpc_mc_guess_stats, MC_BLIND_ROUND_STAT, "MonteCarlo.guess_stats")

    def guess_open(self):
        """the frames of the last guess() that ended open (the first fail_cap of them), ascending -> (indices uint64 [n], guess rows uint32
        [n, ceil(N/32)] MSB-first; all zero with guess_bits = 0)"""
        frames = np.zeros(self.fail_cap, np.uint64)
        weak = np.zeros((self.fail_cap, (self.N + 31) // 32), np.uint32)
        n = _chk(_L.qldpc_mc_guess_open(self._h, frames.ctypes.data_as(_u64p), weak.ctypes.data_as(_up), self.fail_cap), "MonteCarlo.guess_open")
        return frames[:n].copy(), weak[:n].copy()

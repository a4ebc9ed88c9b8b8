"""The batched BP decoder and decoder gangs (qldpc_decoder_*, qldpc_load_*, qldpc_fetch_*, qldpc_gang_*), with the host mirrors of their rules."""
import ctypes as C

import numpy as np

from ._lib import (_L, _Handle, _chk, _create, _default, _dev_empty, _dev_rows, _dev_vec, _fp, _ip, _np_i32, _sig, _stream_arg, _torch, _vp,
                   QldpcError)
from .codes import RULES, SCHEDULES


class DecoderCfg(C.Structure):
    _fields_ = [("schedule", C.c_int), ("rule", C.c_int), ("rule_param", C.c_float), ("n_ite", C.c_int),
                ("enable_syndrome", C.c_int), ("syndrome_depth", C.c_int), ("max_frames", C.c_int),
                ("device", C.c_int), ("frames_per_lane", C.c_int), ("engine", C.c_int), ("freeze_messages", C.c_int), ("msg_dtype", C.c_int), ("quant_scale", C.c_float), ("compact", C.c_int), ("layer_chain", C.c_int), ("giveup_patience", C.c_int)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint64), ("total_ms", C.c_double), ("alg_bytes", C.c_double), ("moved_bytes", C.c_double)]


_sig("qldpc_decoder_cfg_default", None, [C.POINTER(DecoderCfg)])
_sig("qldpc_decoder_create", C.c_int, [_vp, C.c_int, _ip, C.POINTER(DecoderCfg), C.POINTER(_vp)])
_sig("qldpc_decoder_free", None, [_vp])
_sig("qldpc_decoder_set_stream", C.c_int, [_vp, _vp])
_sig("qldpc_decoder_reset", C.c_int, [_vp])
_sig("qldpc_decoder_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_decoder_flood_post", C.c_int, [_vp])
_sig("qldpc_decoder_reserve", C.c_int, [_vp])
_sig("qldpc_decode_siho", C.c_int, [_vp, _fp, _ip, C.c_int])
_sig("qldpc_load_llr_dev", C.c_int, [_vp, _vp, C.c_int])
_sig("qldpc_load_bits_dev", C.c_int, [_vp, _vp, _vp, _vp, C.c_int])
_sig("qldpc_load_bits_short_dev", C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int])
_sig("qldpc_load_syndrome_dev", C.c_int, [_vp, _vp, C.c_int])
_sig("qldpc_load_erasures_dev", C.c_int, [_vp, _vp, C.c_int])
_sig("qldpc_syndrome_dev", C.c_int, [_vp, _vp, _vp, C.c_int])
_sig("qldpc_run", C.c_int, [_vp])
_sig("qldpc_fetch_packed_dev", C.c_int, [_vp, _vp])
_sig("qldpc_fetch_info_dev", C.c_int, [_vp, _vp])
_sig("qldpc_fetch_status_dev", C.c_int, [_vp, _vp, _vp])
_sig("qldpc_fetch_post_dev", C.c_int, [_vp, _vp])
_sig("qldpc_load_known_dev", C.c_int, [_vp, _vp, _vp, C.c_int])
_sig("qldpc_fetch_weakest_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp])
_sig("qldpc_weakest_host", C.c_int, [_fp, C.c_int, _vp, C.c_int, _vp, _ip])
_sig("qldpc_fetch_giveup_dev", C.c_int, [_vp, _vp, _vp, _vp])
_sig("qldpc_giveup_total", C.c_int, [_vp, C.POINTER(C.c_uint64)])
_sig("qldpc_giveup_host", C.c_int, [_ip, C.c_int, C.c_int, C.c_int, _ip, _ip])
_sig("qldpc_sync", C.c_int, [_vp])
_sig("qldpc_profile_enable", C.c_int, [_vp, C.c_int])
_sig("qldpc_profile_read", C.c_int, [_vp, C.POINTER(KernelStat), C.c_int])
_sig("qldpc_profile_clear", C.c_int, [_vp])
_sig("qldpc_last_run_iterations", C.c_int, [_vp])
_sig("qldpc_last_run_stats", C.c_int, [_vp, C.POINTER(C.c_longlong)])
_sig("qldpc_gang_create", C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(_vp)])
_sig("qldpc_gang_free", None, [_vp])
_sig("qldpc_gang_set_stream", C.c_int, [_vp, _vp])
_sig("qldpc_gang_run", C.c_int, [_vp, C.POINTER(C.c_ubyte)])
_sig("qldpc_gang_last_run_stats", C.c_int, [_vp, C.POINTER(C.c_longlong)])
_sig("qldpc_gang_plan", C.c_int, [C.POINTER(_vp), _ip, _ip, C.c_int, _ip, _ip, _ip])
_sig("qldpc_gang_locate_host", C.c_int, [_ip, C.c_int, C.c_int, _ip, _ip])


def _profile_rows(read_fn, h, who):
    """the kernel rows a profile_read call fills, as dicts"""
    arr = (KernelStat * 16)()
    n = _chk(read_fn(h, arr, 16), who)
    return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), total_ms=float(arr[i].total_ms),
                 alg_bytes=float(arr[i].alg_bytes), moved_bytes=float(arr[i].moved_bytes)) for i in range(n)]


class Decoder(_Handle):
    """module::Decoder_LDPC_BP_{flooding,horizontal_layered,vertical_layered}<B,Q,Rule> as a batched HIP decoder.

    Decoder(code, K, n_ite, info_bits_pos, rule=("NMS", 0.75), enable_syndrome, syndrome_depth, n_frames)
    mirrors the AFF3CT ctor (VAR/main.cpp (alist-v1.0.1):203-237).
    """
    _free = _L.qldpc_decoder_free

    def __init__(self, code, K, n_ite, info_bits_pos=None, rule="SPA", rule_param=0.0, enable_syndrome=True,
                 syndrome_depth=1, n_frames=1, schedule="flooding", device=0, frames_per_lane=0, engine="auto",
                 freeze_messages=False, msg_dtype="f32", quant_scale=0.0, compact="auto", layer_chain="auto", giveup=0):
        cfg = _default(DecoderCfg, _L.qldpc_decoder_cfg_default)
        cfg.schedule = SCHEDULES[schedule]
        cfg.rule = RULES[rule]
        cfg.rule_param = float(rule_param)
        cfg.n_ite = int(n_ite)
        cfg.enable_syndrome = int(bool(enable_syndrome))
        cfg.syndrome_depth = int(syndrome_depth)
        cfg.max_frames = int(n_frames)
        cfg.device = int(device)
        cfg.frames_per_lane = int(frames_per_lane)
        cfg.engine = {"auto": 0, "frames": 1, "edges": 2}[engine]
        cfg.freeze_messages = int(bool(freeze_messages))
        cfg.msg_dtype = {"f32": 0, "f16": 1, "i8": 2}[msg_dtype]
        cfg.quant_scale = float(quant_scale)
        cfg.compact = {"auto": 0, "on": 1, "off": 2}[compact]
        cfg.layer_chain = {"auto": 0, "on": 1, "off": 2}[layer_chain]
        cfg.giveup_patience = int(giveup)
        pos = None
        if info_bits_pos is not None:
            pos = _np_i32(info_bits_pos)
            if pos.size != K:
                raise QldpcError(-6, "Decoder: len(info_bits_pos) != K")
        self._h = _create("Decoder", _L.qldpc_decoder_create, code._h, int(K), pos.ctypes.data_as(_ip) if pos is not None else None, C.byref(cfg))
        self.code, self.K, self.N = code, int(K), code.N
        self.max_frames, self.device = int(n_frames), int(device)
        self.giveup = int(giveup)
        self.n_frames = 0

    # -- AFF3CT mirror (host vectors) --------------------------------------------------------
    def decode_siho(self, Y_N):
        """decode_siho(LLRs, dec_bits): Y_N[n_frames, N] float32 -> V_K[n_frames, K] int32 (numpy)."""
        Y = np.ascontiguousarray(Y_N, dtype=np.float32)
        if Y.ndim == 1:
            Y = Y[None, :]
        if Y.shape[1] != self.N:
            raise QldpcError(-6, "decode_siho: Y_N has %d columns, N = %d" % (Y.shape[1], self.N))
        V = np.empty((Y.shape[0], self.K), np.int32)
        _chk(_L.qldpc_decode_siho(self._h, Y.ctypes.data_as(_fp), V.ctypes.data_as(_ip), Y.shape[0]), "decode_siho")
        self.n_frames = Y.shape[0]
        return V

    def reset(self):
        _chk(_L.qldpc_decoder_reset(self._h), "reset")

    # -- staged HBM-resident path (torch tensors own the buffers) ----------------------------
    def set_stream(self, stream=None):
        _chk(_L.qldpc_decoder_set_stream(self._h, _stream_arg(stream, self.device)), "set_stream")

    def _words(self, t, name, rows=None):
        """the pointer of a device int32 tensor of packed rows of N bits"""
        return _dev_rows(t, rows, (self.N + 31) // 32, (_torch().int32,), name)

    def _empty(self, shape, dtype=None):
        """a fresh output tensor (int32 by default) on the decoder's device"""
        return _dev_empty(self.device, shape, dtype or _torch().int32)

    def load_llr(self, llr):
        p = _dev_rows(llr, None, self.N, (_torch().float32,), "llr")
        self.n_frames = llr.shape[0]
        _chk(_L.qldpc_load_llr_dev(self._h, p, llr.shape[0]), "load_llr")

    def load_bits(self, bits, llr_mag, vn_class=None, n_channel=None):
        """QKD frame formation on the device; n_channel[f] (int32, optional): channel VNs at index >= n_channel[f] are known
        (shortened) bits of frame f"""
        torch = _torch()
        pb, F = _dev_rows(bits, None, (self.N + 31) // 32, (torch.int32, torch.uint32), "bits"), bits.shape[0]
        pm, pc = _dev_vec(llr_mag, F, torch.float32, "llr_mag"), _dev_vec(vn_class, self.N, torch.uint8, "vn_class")
        self.n_frames = F
        if n_channel is not None:
            _chk(_L.qldpc_load_bits_short_dev(self._h, pb, pm, pc, _dev_vec(n_channel, F, torch.int32, "n_channel"), F), "load_bits")
            return
        _chk(_L.qldpc_load_bits_dev(self._h, pb, pm, pc, F), "load_bits")

    def load_erasures(self, erase_bits):
        """per-frame puncturing: packed masks [n_frames, ceil(N/32)], a set bit makes that VN of that frame an erasure (LLR 0)"""
        _chk(_L.qldpc_load_erasures_dev(self._h, self._words(erase_bits, "erase_bits"), erase_bits.shape[0]), "load_erasures")

    def load_known(self, known_bits, value_bits):
        """blind reconciliation: packed masks [n_frames, ceil(N/32)], a set known bit pins that VN of that frame to its value bit (+-23.03);
        known wins over erased, the next load clears it"""
        pk = self._words(known_bits, "known_bits")
        _chk(_L.qldpc_load_known_dev(self._h, pk, self._words(value_bits, "value_bits", rows=known_bits.shape[0]), known_bits.shape[0]), "load_known")

    def load_syndrome(self, synd_bits):
        """syndrome form: packed target syndromes [n_frames, ceil(M/32)] for the frames just loaded"""
        p = _dev_rows(synd_bits, None, (self.code.M + 31) // 32, (_torch().int32,), "synd_bits")
        _chk(_L.qldpc_load_syndrome_dev(self._h, p, synd_bits.shape[0]), "load_syndrome")

    def syndrome_of(self, bits):
        """s = H x for packed words [F, ceil(N/32)] -> [F, ceil(M/32)] (device)"""
        p = self._words(bits, "bits")
        out = _dev_empty(bits.device, (bits.shape[0], (self.code.M + 31) // 32), _torch().int32)
        _chk(_L.qldpc_syndrome_dev(self._h, p, _vp(out.data_ptr()), bits.shape[0]), "syndrome_of")
        return out

    def run(self):
        _chk(_L.qldpc_run(self._h), "run")

    def fetch_packed(self, out=None):
        if out is None:
            out = self._empty((self.n_frames, (self.N + 31) // 32))
        _chk(_L.qldpc_fetch_packed_dev(self._h, _vp(out.data_ptr())), "fetch_packed")
        return out

    def fetch_info(self, out=None):
        if out is None:
            out = self._empty((self.n_frames, self.K))
        _chk(_L.qldpc_fetch_info_dev(self._h, _vp(out.data_ptr())), "fetch_info")
        return out

    def fetch_status(self):
        it, ok = self._empty(self.n_frames), self._empty(self.n_frames)
        _chk(_L.qldpc_fetch_status_dev(self._h, _vp(it.data_ptr()), _vp(ok.data_ptr())), "fetch_status")
        return it, ok

    def fetch_post(self):
        out = self._empty((self.n_frames, self.N), _torch().float32)
        _chk(_L.qldpc_fetch_post_dev(self._h, _vp(out.data_ptr())), "fetch_post")
        return out

    def fetch_weakest(self, d, cand_bits=None, take=None):
        """blind reconciliation: packed rows [n_frames, ceil(N/32)] with a bit set for the min(d, candidates) smallest |posterior| of each
        frame in (key, v) order (weakest_host); cand_bits [n_frames, ceil(N/32)] int32 = the candidates (None: every VN), take [n_frames]
        int32, non-zero = wanted (None: every frame; rows of the others are zero)"""
        pc, pt = self._words(cand_bits, "cand_bits", rows=self.n_frames), _dev_vec(take, self.n_frames, _torch().int32, "take")
        out = self._empty((self.n_frames, (self.N + 31) // 32))
        _chk(_L.qldpc_fetch_weakest_dev(self._h, pc, pt, int(d), _vp(out.data_ptr())), "fetch_weakest")
        return out

    def fetch_giveup(self):
        """decoders created with giveup >= 1: (gave, last, best) int32 [n_frames] -- 1 for a frame the run gave up, its syndrome weight at its
        last test, the smallest weight it showed at a test (qldpc_fetch_giveup_dev)"""
        gave, last, best = (self._empty(self.n_frames) for _ in range(3))
        _chk(_L.qldpc_fetch_giveup_dev(self._h, _vp(gave.data_ptr()), _vp(last.data_ptr()), _vp(best.data_ptr())), "fetch_giveup")
        return gave, last, best

    def giveup_total(self):
        """frames given up by all runs of this decoder since it was created (qldpc_giveup_total; 0 with giveup = 0)"""
        n = C.c_uint64(0)
        _chk(_L.qldpc_giveup_total(self._h, C.byref(n)), "giveup_total")
        return int(n.value)

    def sync(self):
        _chk(_L.qldpc_sync(self._h), "sync")

    @property
    def device_bytes(self):
        return _L.qldpc_decoder_device_bytes(self._h)

    @property
    def flood_post(self):
        """fixed-iteration flooding runs of this decoder take the posterior form (qldpc_decoder_flood_post)"""
        return bool(_chk(_L.qldpc_decoder_flood_post(self._h), "flood_post"))

    @property
    def last_run_iterations(self):
        return _L.qldpc_last_run_iterations(self._h)

    def last_run_stats(self):
        """Early-exit bookkeeping of the last run: lane-iterations executed, compactions, groups in flight at the end, frames per group."""
        out = (C.c_longlong * 4)()
        _chk(_L.qldpc_last_run_stats(self._h, out), "last_run_stats")
        return dict(lane_iterations=int(out[0]), compactions=int(out[1]), final_groups=int(out[2]), frames_per_group=int(out[3]))

    # -- measurement ---------------------------------------------------------------------------
    def profile(self, on=True):
        _chk(_L.qldpc_profile_enable(self._h, int(on)), "profile")

    def profile_clear(self):
        _chk(_L.qldpc_profile_clear(self._h), "profile_clear")

    def profile_read(self):
        return _profile_rows(_L.qldpc_profile_read, self._h, "profile_read")


class DecoderGang(_Handle):
    """Several horizontal-layered Decoders stepped in lockstep: every colour step of a sweep is one launch per kernel class for all
    members (qldpc.h "decoder gangs").  Members are loaded and read through their own calls and give what Decoder.run() gives, bit for bit."""
    _free = _L.qldpc_gang_free

    def __init__(self, decoders):
        self.members = list(decoders)      # kept alive: the gang does not own them
        arr = (_vp * max(1, len(self.members)))(*[d._h for d in self.members])
        self._h = _create("DecoderGang", _L.qldpc_gang_create, arr, len(self.members))

    def set_stream(self, stream=None):
        _chk(_L.qldpc_gang_set_stream(self._h, _stream_arg(stream, self.members[0].device)), "DecoderGang.set_stream")

    def run(self, take=None):
        """take: one flag per member (None = every member); the others are left as they are"""
        flags = None
        if take is not None:
            if len(take) != len(self.members):
                raise QldpcError(-1, "DecoderGang.run: len(take) != number of members")
            flags = (C.c_ubyte * len(self.members))(*[1 if t else 0 for t in take])
        _chk(_L.qldpc_gang_run(self._h, flags), "DecoderGang.run")

    def last_run_stats(self):
        """sweeps issued, layer launches issued, layer launches the members would have issued alone, members dropped before the last sweep"""
        out = (C.c_longlong * 4)()
        _chk(_L.qldpc_gang_last_run_stats(self._h, out), "DecoderGang.last_run_stats")
        return dict(sweeps=int(out[0]), launches=int(out[1]), solo_launches=int(out[2]), dropped=int(out[3]))


def gang_plan(codes, rules, compressed=None):
    """The launch plan of a gang on these codes (host only): dict(steps, launches_per_sweep, solo_launches_per_sweep).
    rules[i]: rule name of member i; compressed[i]: it keeps the compressed check state (min-sum / AMS rules, check degree <= 32)."""
    n = len(codes)
    if len(rules) != n or (compressed is not None and len(compressed) != n):
        raise QldpcError(-1, "gang_plan: one rule (and one compressed flag) per code")
    arr = (_vp * max(1, n))(*[c._h for c in codes])
    r = _np_i32([RULES[x] for x in rules])
    cs = _np_i32([1 if x else 0 for x in compressed]) if compressed is not None else None
    st, la, so = C.c_int(), C.c_int(), C.c_int()
    _chk(_L.qldpc_gang_plan(arr, r.ctypes.data_as(_ip), cs.ctypes.data_as(_ip) if cs is not None else None, n, C.byref(st), C.byref(la), C.byref(so)), "gang_plan")
    return dict(steps=st.value, launches_per_sweep=la.value, solo_launches_per_sweep=so.value)


def gang_locate(prefix, block):
    """(member, block within the member's range) of a block of a gang launch whose member m owns [prefix[m], prefix[m + 1]): the host mirror
    of the kernels' mapping"""
    p = _np_i32(prefix)
    m, loc = C.c_int(), C.c_int()
    _chk(_L.qldpc_gang_locate_host(p.ctypes.data_as(_ip), p.size - 1, int(block), C.byref(m), C.byref(loc)), "gang_locate")
    return m.value, loc.value


GIVEUP_CONVERGED, GIVEUP_GAVE_UP, GIVEUP_RAN_OUT = 0, 1, 2


def giveup_host(weights, patience, syndrome_depth=1):
    """the give-up rule of the early-exit run on the host (qldpc_giveup_host): weights[n_tests] = the syndrome weights of one frame at the tests
    of a run that never stops it -> (stop_test, outcome): the 1-based test at which it converged or was given up (0: it ran out) and one of
    GIVEUP_CONVERGED / GIVEUP_GAVE_UP / GIVEUP_RAN_OUT.  patience = 0: the rule is off"""
    w = _np_i32(weights).reshape(-1)
    stop, what = C.c_int(0), C.c_int(0)
    _chk(_L.qldpc_giveup_host(w.ctypes.data_as(_ip), w.size, int(syndrome_depth), int(patience), C.byref(stop), C.byref(what)), "giveup_host")
    return stop.value, what.value


def weakest_host(post, d, cand_bits=None):
    """the select of blind reconciliation on the host (qldpc_weakest_host): post[N] float32 -> (packed row of ceil(N/32) uint32 words with a
    bit set for the min(d, candidates) smallest |post| in (bit pattern of |post|, v) order, number of bits set)"""
    x = np.ascontiguousarray(post, dtype=np.float32).ravel()
    W = (x.size + 31) // 32
    c = None
    if cand_bits is not None:
        c = np.ascontiguousarray(cand_bits, dtype=np.uint32).ravel()
        if c.size != W:
            raise QldpcError(-6, "weakest_host: cand_bits has %d words, ceil(N/32) = %d" % (c.size, W))
    out = np.zeros(max(W, 1), np.uint32)
    n = C.c_int(0)
    _chk(_L.qldpc_weakest_host(x.ctypes.data_as(_fp), x.size, c.ctypes.data_as(_vp) if c is not None else None, int(d), out.ctypes.data_as(_vp), C.byref(n)),
         "weakest_host")
    return out[:W], n.value

"""qcrypto-ldpc_amd: host-side mirror (Python, ctypes) of the LDPC reconciliation path.

The product is ``libqldpc.so`` (hand-written HIP for gfx950 behind the C ABI of ``include/qldpc.h``).
This package only binds it: names and argument meaning follow the objects the reference harness
builds from AFF3CT (``Decoder_LDPC_BP_flooding(K, N, n_ite, H, info_bits_pos, rule, enable_syndrome,
syndrome_depth, n_frames)``, ``decode_siho``, ``reset``, ``encode`` -- BS/src/main.cpp:172-195,335-393).
PyTorch appears only as the owner of device buffers / streams handed to the C ABI as raw pointers.

There is NO CPU fallback: if the shared library is missing the import fails loudly.

The directory name has a hyphen, so load it with ``_qldpc_loader.load()`` (repo root) which
registers it as module ``qcrypto_ldpc_amd``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QLDPC_LIB") or os.path.join(_HERE, "libqldpc.so")      # QLDPC_LIB: A/B builds of the same library

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libqldpc.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` or "
        "`make -C qcrypto-ldpc_amd/csrc`. There is no CPU fallback." % LIB_PATH)

def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 (soname libamdhip64.so.7, requested by file name).
    If libqldpc pulled /opt/rocm's copy in first, a later `import torch` would load a SECOND HIP runtime and
    whichever initialises last sees no GPU.  Loading torch's copy first makes both share one runtime."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    for d in spec.submodule_search_locations:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            try:
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            except OSError:
                pass
            return


_preload_torch_hip_runtime()
_L = C.CDLL(LIB_PATH)

RULES = {"MS": 0, "OMS": 1, "NMS": 2, "SPA": 3, "LSPA": 4, "AMS_MIN": 5, "AMS_MINSTAR_L2": 6, "AMS_MINSTAR": 7}
SCHEDULES = {"flooding": 0, "hlayered": 1, "vlayered": 3}      # 2 is QLDPC_RECON_SCHED_AUTO (sessions only)
VN_CHANNEL, VN_PINNED, VN_PUNCTURED = 0, 1, 2
CONFIRMED_BIT_LLR = 23.025850929840455

_ip = C.POINTER(C.c_int)
_fp = C.POINTER(C.c_float)
_vp = C.c_void_p


class DecoderCfg(C.Structure):
    _fields_ = [("schedule", C.c_int), ("rule", C.c_int), ("rule_param", C.c_float), ("n_ite", C.c_int),
                ("enable_syndrome", C.c_int), ("syndrome_depth", C.c_int), ("max_frames", C.c_int),
                ("device", C.c_int), ("frames_per_lane", C.c_int), ("engine", C.c_int), ("freeze_messages", C.c_int), ("msg_dtype", C.c_int), ("quant_scale", C.c_float), ("compact", C.c_int), ("layer_chain", C.c_int), ("giveup_patience", C.c_int)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_uint64), ("total_ms", C.c_double), ("alg_bytes", C.c_double), ("moved_bytes", C.c_double)]


def _sig(name, res, args):
    f = getattr(_L, name)
    f.restype = res
    f.argtypes = args
    return f


_sig("qldpc_version", C.c_int, [])
_sig("qldpc_strerror", C.c_char_p, [C.c_int])
_sig("qldpc_last_error", C.c_char_p, [])
_sig("qldpc_device_count", C.c_int, [])
_sig("qldpc_copy_probe", C.c_int, [C.c_int, C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_double)])
_sig("qldpc_llr_from_ber", C.c_float, [C.c_float])
_sig("qldpc_bsc_llr", C.c_float, [C.c_float])
_sig("qldpc_binary_entropy", C.c_float, [C.c_float])
_sig("qldpc_min_code_rate", C.c_float, [C.c_float, C.c_float])
_sig("qldpc_parity_bits_to_punct", C.c_int, [C.c_int, C.c_int, C.c_float])
_sig("qldpc_code_from_alist", C.c_int, [C.c_char_p, C.POINTER(_vp)])
_sig("qldpc_code_from_qc", C.c_int, [C.c_char_p, C.POINTER(_vp)])
_sig("qldpc_code_from_edges", C.c_int, [C.c_int, C.c_int, C.c_int, _ip, _ip, C.POINTER(_vp)])
_sig("qldpc_code_ira", C.c_int, [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_uint64, C.POINTER(_vp)])
_sig("qldpc_code_ira_peg", C.c_int, [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(_vp)])
_sig("qldpc_code_free", None, [_vp])
for _n in ("n", "m", "e", "max_cn_degree", "max_vn_degree", "is_ira", "layer_count", "vlayer_count"):
    _sig("qldpc_code_" + _n, C.c_int, [_vp])
_sig("qldpc_code_qc_peg", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_char_p, C.POINTER(_vp), _ip])
_sig("qldpc_code_export_edges", C.c_int, [_vp, _ip, _ip])
_sig("qldpc_code_layer_order", C.c_int, [_vp, _ip, _ip])
_sig("qldpc_code_vlayer_order", C.c_int, [_vp, _ip, _ip])
_sig("qldpc_code_syndrome_host", C.c_int, [_vp, _ip, _ip])
_sig("qldpc_code_chain_table", C.c_int, [_vp, _vp])
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
_sig("qldpc_encoder_create", C.c_int, [_vp, C.c_char_p, C.c_int, C.POINTER(_vp)])
_sig("qldpc_encoder_free", None, [_vp])
_sig("qldpc_encoder_reserve", C.c_int, [_vp, C.c_int])
_sig("qldpc_encoder_k", C.c_int, [_vp])
_sig("qldpc_encoder_info_bits_pos", C.c_int, [_vp, _ip])
_sig("qldpc_encode", C.c_int, [_vp, _ip, _ip, C.c_int])
_sig("qldpc_encode_packed_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp])


class QldpcError(RuntimeError):
    """Raised where the AFF3CT objects would throw tools::exception; carries the C status."""

    def __init__(self, status, where):
        self.status = status
        msg = _L.qldpc_last_error().decode(errors="replace")
        super().__init__("%s: %s (%d)%s" % (where, _L.qldpc_strerror(status).decode(), status, (": " + msg) if msg else ""))


def _chk(rc, where):
    if rc < 0:
        raise QldpcError(rc, where)
    return rc


def version():
    return _L.qldpc_version()


def device_count():
    return _L.qldpc_device_count()


def copy_probe(nbytes=1 << 30, reps=10, wide=False, device=0):
    """GB/s (bytes read + bytes written) this device copies at in the decoder's access shape (qldpc_copy_probe): a measured ceiling
    to read the kernels' rates against."""
    out = C.c_double(0.0)
    _chk(_L.qldpc_copy_probe(int(device), int(nbytes), int(reps), 1 if wide else 0, C.byref(out)), "copy_probe")
    return out.value


def llr_from_ber(p):
    """LLR(BER) macro, BS/src/main.cpp:20."""
    return _L.qldpc_llr_from_ber(float(p))


def bsc_llr(p):
    """|LLR| Modem_OOK_BSC gives a channel bit, BS/src/main.cpp:317,348."""
    return _L.qldpc_bsc_llr(float(p))


def binary_entropy(q):
    return _L.qldpc_binary_entropy(float(q))


def min_code_rate(qber, efficiency):
    return _L.qldpc_min_code_rate(float(qber), float(efficiency))


def parity_bits_to_punct(N, K, target_cr):
    return _L.qldpc_parity_bits_to_punct(int(N), int(K), float(target_cr))


def _np_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Code:
    """Parity-check matrix H (tools::Sparse_matrix as the harness holds it; rows = variable nodes)."""

    def __init__(self, handle):
        self._h = _vp(handle)
        self.N = _L.qldpc_code_n(self._h)
        self.M = _L.qldpc_code_m(self._h)
        self.E = _L.qldpc_code_e(self._h)
        self.max_cn_degree = _L.qldpc_code_max_cn_degree(self._h)
        self.max_vn_degree = _L.qldpc_code_max_vn_degree(self._h)
        self.is_ira = bool(_L.qldpc_code_is_ira(self._h))
        self.n_layers = _L.qldpc_code_layer_count(self._h)

    @classmethod
    def from_alist(cls, path):
        h = _vp()
        _chk(_L.qldpc_code_from_alist(os.fsencode(path), C.byref(h)), "Code.from_alist")
        return cls(h.value)

    @classmethod
    def from_qc(cls, path):
        h = _vp()
        _chk(_L.qldpc_code_from_qc(os.fsencode(path), C.byref(h)), "Code.from_qc")
        return cls(h.value)

    @classmethod
    def from_edges(cls, N, M, var, chk):
        var, chk = _np_i32(var), _np_i32(chk)
        if var.shape != chk.shape:
            raise QldpcError(-6, "Code.from_edges")
        h = _vp()
        _chk(_L.qldpc_code_from_edges(int(N), int(M), int(var.size), var.ctypes.data_as(_ip), chk.ctypes.data_as(_ip),
                                      C.byref(h)), "Code.from_edges")
        return cls(h.value)

    @classmethod
    def ira(cls, N, K, hi_frac=0.125, dv_hi=11, dv_lo=3, seed=7):
        h = _vp()
        _chk(_L.qldpc_code_ira(int(N), int(K), float(hi_frac), int(dv_hi), int(dv_lo), int(seed), C.byref(h)), "Code.ira")
        return cls(h.value)

    @classmethod
    def ira_peg(cls, N, K, hi_frac=0.125, dv_hi=11, dv_lo=3, depth=2, seed=7):
        """IRA profile with a progressive-edge-growth information part (depth 2: no 4-cycles)."""
        h = _vp()
        _chk(_L.qldpc_code_ira_peg(int(N), int(K), float(hi_frac), int(dv_hi), int(dv_lo), int(depth), int(seed), C.byref(h)), "Code.ira_peg")
        return cls(h.value)

    @classmethod
    def qc_peg(cls, n_cols, m_rows, dv, Z, seed=1, qc_path=None):
        """QC code, base graph by PEG with cycle-breaking circulant shifts (the reference's psd-peg.py), H = [lift(P) | I].
        The returned code carries .base_girth; qc_path also writes the AFF3CT .qc file."""
        h = _vp()
        g = C.c_int(0)
        _chk(_L.qldpc_code_qc_peg(int(n_cols), int(m_rows), int(dv), int(Z), int(seed), qc_path.encode() if qc_path else None, C.byref(h), C.byref(g)),
             "Code.qc_peg")
        c = cls(h.value)
        c.base_girth = g.value
        return c

    def edges(self):
        var = np.empty(self.E, np.int32)
        chk = np.empty(self.E, np.int32)
        _chk(_L.qldpc_code_export_edges(self._h, var.ctypes.data_as(_ip), chk.ctypes.data_as(_ip)), "Code.edges")
        return var, chk

    def layer_order(self):
        """(check_order[M], layer_ptr[n_layers+1], natural) of the horizontal-layered sweep."""
        order = np.empty(self.M, np.int32)
        ptr = np.empty(self.n_layers + 1, np.int32)
        nat = _chk(_L.qldpc_code_layer_order(self._h, order.ctypes.data_as(_ip), ptr.ctypes.data_as(_ip)), "Code.layer_order")
        return order, ptr, bool(nat)

    @property
    def n_vlayers(self):
        """classes of the vertical-layered sweep (the order is built on first use)"""
        return _chk(_L.qldpc_code_vlayer_count(self._h), "Code.n_vlayers")

    def vlayer_order(self):
        """(vn_order[N], vlayer_ptr[n_vlayers+1], natural) of the vertical-layered sweep: VNs of one class share no check;
        natural = the classes in order are the sequential v = 0..N-1 sweep, else the sweep runs in vn_order."""
        order = np.empty(self.N, np.int32)
        ptr = np.empty(self.n_vlayers + 1, np.int32)
        nat = _chk(_L.qldpc_code_vlayer_order(self._h, order.ctypes.data_as(_ip), ptr.ctypes.data_as(_ip)), "Code.vlayer_order")
        return order, ptr, bool(nat)

    def chain_table(self):
        """The IRA chain as the posterior form of the flooding run uses it: uint8 [M, 4] = positions of VN K + c - 1 and K + c in the row of check c,
        of VN K + c - 1 in the row of check c - 1 and of VN K + c in the row of check c + 1 (255: no such edge); None if the graph does not qualify."""
        tab = np.empty(self.M, np.uint32)
        ok = _chk(_L.qldpc_code_chain_table(self._h, _vp(tab.ctypes.data)), "Code.chain_table")
        if not ok:
            return None
        return np.stack([(tab >> s) & 0xff for s in (0, 8, 16, 24)], axis=1).astype(np.uint8)

    def syndrome(self, x):
        x = _np_i32(x)
        s = np.empty(self.M, np.int32)
        w = _chk(_L.qldpc_code_syndrome_host(self._h, x.ctypes.data_as(_ip), s.ctypes.data_as(_ip)), "Code.syndrome")
        return w, s

    def __del__(self):
        try:
            _L.qldpc_code_free(self._h)
        except Exception:
            pass


def _torch():
    import torch
    return torch


class Decoder:
    """module::Decoder_LDPC_BP_{flooding,horizontal_layered,vertical_layered}<B,Q,Rule> as a batched HIP decoder.

    Decoder(code, K, n_ite, info_bits_pos, rule=("NMS", 0.75), enable_syndrome, syndrome_depth, n_frames)
    mirrors the AFF3CT ctor (VAR/main.cpp (alist-v1.0.1):203-237).
    """

    def __init__(self, code, K, n_ite, info_bits_pos=None, rule="SPA", rule_param=0.0, enable_syndrome=True,
                 syndrome_depth=1, n_frames=1, schedule="flooding", device=0, frames_per_lane=0, engine="auto",
                 freeze_messages=False, msg_dtype="f32", quant_scale=0.0, compact="auto", layer_chain="auto", giveup=0):
        cfg = DecoderCfg()
        _L.qldpc_decoder_cfg_default(C.byref(cfg))
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
        h = _vp()
        _chk(_L.qldpc_decoder_create(code._h, int(K), pos.ctypes.data_as(_ip) if pos is not None else None,
                                     C.byref(cfg), C.byref(h)), "Decoder")
        self._h = h
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
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        _chk(_L.qldpc_decoder_set_stream(self._h, _vp(s.cuda_stream)), "set_stream")

    def load_llr(self, llr):
        torch = _torch()
        assert llr.is_cuda and llr.dtype == torch.float32 and llr.is_contiguous() and llr.dim() == 2 and llr.shape[1] == self.N
        self.n_frames = llr.shape[0]
        _chk(_L.qldpc_load_llr_dev(self._h, _vp(llr.data_ptr()), llr.shape[0]), "load_llr")

    def load_bits(self, bits, llr_mag, vn_class=None, n_channel=None):
        """QKD frame formation on the device; n_channel[f] (int32, optional): channel VNs at index >= n_channel[f] are known
        (shortened) bits of frame f"""
        torch = _torch()
        W = (self.N + 31) // 32
        assert bits.is_cuda and bits.dtype in (torch.int32, torch.uint32) and bits.is_contiguous() and bits.shape[1] == W
        assert llr_mag.is_cuda and llr_mag.dtype == torch.float32 and llr_mag.numel() == bits.shape[0]
        if vn_class is not None:
            assert vn_class.is_cuda and vn_class.dtype == torch.uint8 and vn_class.numel() == self.N
        self.n_frames = bits.shape[0]
        if n_channel is not None:
            assert n_channel.is_cuda and n_channel.dtype == torch.int32 and n_channel.numel() == bits.shape[0]
            _chk(_L.qldpc_load_bits_short_dev(self._h, _vp(bits.data_ptr()), _vp(llr_mag.data_ptr()),
                                              _vp(vn_class.data_ptr()) if vn_class is not None else None, _vp(n_channel.data_ptr()), bits.shape[0]), "load_bits")
            return
        _chk(_L.qldpc_load_bits_dev(self._h, _vp(bits.data_ptr()), _vp(llr_mag.data_ptr()),
                                    _vp(vn_class.data_ptr()) if vn_class is not None else None, bits.shape[0]), "load_bits")

    def load_erasures(self, erase_bits):
        """per-frame puncturing: packed masks [n_frames, ceil(N/32)], a set bit makes that VN of that frame an erasure (LLR 0)"""
        torch = _torch()
        assert erase_bits.is_cuda and erase_bits.dtype == torch.int32 and erase_bits.is_contiguous() and erase_bits.shape[1] == (self.N + 31) // 32
        _chk(_L.qldpc_load_erasures_dev(self._h, _vp(erase_bits.data_ptr()), erase_bits.shape[0]), "load_erasures")

    def load_known(self, known_bits, value_bits):
        """blind reconciliation: packed masks [n_frames, ceil(N/32)], a set known bit pins that VN of that frame to its value bit (+-23.03);
        known wins over erased, the next load clears it"""
        torch = _torch()
        W = (self.N + 31) // 32
        for t in (known_bits, value_bits):
            assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == W
        assert known_bits.shape[0] == value_bits.shape[0]
        _chk(_L.qldpc_load_known_dev(self._h, _vp(known_bits.data_ptr()), _vp(value_bits.data_ptr()), known_bits.shape[0]), "load_known")

    def load_syndrome(self, synd_bits):
        """syndrome form: packed target syndromes [n_frames, ceil(M/32)] for the frames just loaded"""
        torch = _torch()
        Wm = (self.code.M + 31) // 32
        assert synd_bits.is_cuda and synd_bits.dtype == torch.int32 and synd_bits.is_contiguous() and synd_bits.shape[1] == Wm
        _chk(_L.qldpc_load_syndrome_dev(self._h, _vp(synd_bits.data_ptr()), synd_bits.shape[0]), "load_syndrome")

    def syndrome_of(self, bits):
        """s = H x for packed words [F, ceil(N/32)] -> [F, ceil(M/32)] (device)"""
        torch = _torch()
        assert bits.is_cuda and bits.dtype == torch.int32 and bits.is_contiguous() and bits.shape[1] == (self.N + 31) // 32
        out = torch.empty((bits.shape[0], (self.code.M + 31) // 32), dtype=torch.int32, device=bits.device)
        _chk(_L.qldpc_syndrome_dev(self._h, _vp(bits.data_ptr()), _vp(out.data_ptr()), bits.shape[0]), "syndrome_of")
        return out

    def run(self):
        _chk(_L.qldpc_run(self._h), "run")

    def fetch_packed(self, out=None):
        torch = _torch()
        W = (self.N + 31) // 32
        if out is None:
            out = torch.empty((self.n_frames, W), dtype=torch.int32, device="cuda:%d" % self.device)
        _chk(_L.qldpc_fetch_packed_dev(self._h, _vp(out.data_ptr())), "fetch_packed")
        return out

    def fetch_info(self, out=None):
        torch = _torch()
        if out is None:
            out = torch.empty((self.n_frames, self.K), dtype=torch.int32, device="cuda:%d" % self.device)
        _chk(_L.qldpc_fetch_info_dev(self._h, _vp(out.data_ptr())), "fetch_info")
        return out

    def fetch_status(self):
        torch = _torch()
        it = torch.empty(self.n_frames, dtype=torch.int32, device="cuda:%d" % self.device)
        ok = torch.empty(self.n_frames, dtype=torch.int32, device="cuda:%d" % self.device)
        _chk(_L.qldpc_fetch_status_dev(self._h, _vp(it.data_ptr()), _vp(ok.data_ptr())), "fetch_status")
        return it, ok

    def fetch_post(self):
        torch = _torch()
        out = torch.empty((self.n_frames, self.N), dtype=torch.float32, device="cuda:%d" % self.device)
        _chk(_L.qldpc_fetch_post_dev(self._h, _vp(out.data_ptr())), "fetch_post")
        return out

    def fetch_weakest(self, d, cand_bits=None, take=None):
        """blind reconciliation: packed rows [n_frames, ceil(N/32)] with a bit set for the min(d, candidates) smallest |posterior| of each
        frame in (key, v) order (weakest_host); cand_bits [n_frames, ceil(N/32)] int32 = the candidates (None: every VN), take [n_frames]
        int32, non-zero = wanted (None: every frame; rows of the others are zero)"""
        torch = _torch()
        W = (self.N + 31) // 32
        if cand_bits is not None:
            assert cand_bits.is_cuda and cand_bits.dtype == torch.int32 and cand_bits.is_contiguous() and tuple(cand_bits.shape) == (self.n_frames, W)
        if take is not None:
            assert take.is_cuda and take.dtype == torch.int32 and take.is_contiguous() and take.numel() == self.n_frames
        out = torch.empty((self.n_frames, W), dtype=torch.int32, device="cuda:%d" % self.device)
        _chk(_L.qldpc_fetch_weakest_dev(self._h, _vp(cand_bits.data_ptr()) if cand_bits is not None else None,
                                        _vp(take.data_ptr()) if take is not None else None, int(d), _vp(out.data_ptr())), "fetch_weakest")
        return out

    def fetch_giveup(self):
        """decoders created with giveup >= 1: (gave, last, best) int32 [n_frames] -- 1 for a frame the run gave up, its syndrome weight at its
        last test, the smallest weight it showed at a test (qldpc_fetch_giveup_dev)"""
        torch = _torch()
        gave, last, best = (torch.empty(self.n_frames, dtype=torch.int32, device="cuda:%d" % self.device) for _ in range(3))
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
        arr = (KernelStat * 16)()
        n = _chk(_L.qldpc_profile_read(self._h, arr, 16), "profile_read")
        return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), total_ms=float(arr[i].total_ms),
                     alg_bytes=float(arr[i].alg_bytes), moved_bytes=float(arr[i].moved_bytes)) for i in range(n)]

    def __del__(self):
        try:
            _L.qldpc_decoder_free(self._h)
        except Exception:
            pass


class DecoderGang:
    """Several horizontal-layered Decoders stepped in lockstep: every colour step of a sweep is one launch per kernel class for all
    members (qldpc.h "decoder gangs").  Members are loaded and read through their own calls and give what Decoder.run() gives, bit for bit."""

    def __init__(self, decoders):
        self.members = list(decoders)      # kept alive: the gang does not own them
        arr = (_vp * max(1, len(self.members)))(*[d._h for d in self.members])
        h = _vp()
        _chk(_L.qldpc_gang_create(arr, len(self.members), C.byref(h)), "DecoderGang")
        self._h = h

    def set_stream(self, stream=None):
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream(self.members[0].device)
        _chk(_L.qldpc_gang_set_stream(self._h, _vp(s.cuda_stream)), "DecoderGang.set_stream")

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

    def __del__(self):
        try:
            _L.qldpc_gang_free(self._h)
        except Exception:
            pass


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


class Encoder:
    """m.encoder->encode (BS/src/main.cpp:341): method 'IRA', 'IDENTITY' / 'LU_DEC' (Encoder_LDPC_from_H's G_methods) or 'QC' (Encoder_LDPC_from_QC)."""

    def __init__(self, code, method="IDENTITY", device=0):
        h = _vp()
        _chk(_L.qldpc_encoder_create(code._h, method.encode(), int(device), C.byref(h)), "Encoder")
        self._h = h
        self.code, self.N, self.device = code, code.N, int(device)
        self.K = _L.qldpc_encoder_k(self._h)
        pos = np.empty(self.K, np.int32)
        _chk(_L.qldpc_encoder_info_bits_pos(self._h, pos.ctypes.data_as(_ip)), "Encoder.info_bits_pos")
        self.info_bits_pos = pos

    def encode(self, U_K):
        U = _np_i32(U_K)
        if U.ndim == 1:
            U = U[None, :]
        if U.shape[1] != self.K:
            raise QldpcError(-6, "encode: U_K has %d columns, K = %d" % (U.shape[1], self.K))
        X = np.empty((U.shape[0], self.N), np.int32)
        _chk(_L.qldpc_encode(self._h, U.ctypes.data_as(_ip), X.ctypes.data_as(_ip), U.shape[0]), "encode")
        return X

    def encode_packed(self, info, stream=None):
        torch = _torch()
        Wk, Wn = (self.K + 31) // 32, (self.N + 31) // 32
        assert info.is_cuda and info.dtype == torch.int32 and info.is_contiguous() and info.shape[1] == Wk
        out = torch.empty((info.shape[0], Wn), dtype=torch.int32, device=info.device)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        _chk(_L.qldpc_encode_packed_dev(self._h, _vp(info.data_ptr()), _vp(out.data_ptr()), info.shape[0], _vp(s.cuda_stream)),
             "encode_packed")
        return out

    def __del__(self):
        try:
            _L.qldpc_encoder_free(self._h)
        except Exception:
            pass


# ---- packed-bit helpers (ProcessBlock.mainBufPtr layout, helpers.h:65-70) ----------------------

def pack_bits(bits):
    """bits[..., n] of 0/1 -> uint32 words [..., ceil(n/32)], bit i <-> word[i/32] & (1 << (31 - i%32))."""
    b = np.asarray(bits).astype(np.uint8)
    n = b.shape[-1]
    pad = (-n) % 32
    if pad:
        b = np.concatenate([b, np.zeros(b.shape[:-1] + (pad,), np.uint8)], axis=-1)
    by = np.packbits(b, axis=-1, bitorder="big")
    return by.reshape(b.shape[:-1] + (-1, 4)).astype(np.uint32) @ np.array([1 << 24, 1 << 16, 1 << 8, 1], np.uint32)


def unpack_bits(words, n):
    w = np.asarray(words).astype(np.uint32)
    by = np.stack([(w >> 24) & 255, (w >> 16) & 255, (w >> 8) & 255, w & 255], axis=-1).astype(np.uint8)
    bits = np.unpackbits(by.reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="big")
    return bits[..., :n]


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


# ---- QBER from the syndrome weight (qldpc_qber_*) -----------------------------------------------

QBER_MAX_DEGREE = 63


class QberCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("max_frames", C.c_int), ("n_grid", C.c_int), ("q_lo", C.c_float), ("q_hi", C.c_float), ("checks_per_block", C.c_int)]


_sig("qldpc_qber_cfg_default", None, [C.POINTER(QberCfg)])
_sig("qldpc_qber_create", C.c_int, [_vp, C.POINTER(QberCfg), C.POINTER(_vp)])
_sig("qldpc_qber_free", None, [_vp])
_sig("qldpc_qber_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_qber_set_stream", C.c_int, [_vp, _vp])
_sig("qldpc_qber_grid", C.c_int, [_vp, _fp, _fp])
_sig("qldpc_qber_estimate_dev", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_qber_table_host", C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, _vp, _vp, _fp, _fp])
_sig("qldpc_qber_counts_host", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_qber_argmax_host", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _ip])
_sig("qldpc_qber_counts_merged_host", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_qber_set_merge", C.c_int, [_vp, C.c_int])
_sig("qldpc_qber_count_rows", C.c_int, [_vp])


def qber_table_host(max_degree, n_grid=256, q_lo=0.001, q_hi=0.25):
    """the grid and score tables of the estimator (qldpc_qber_table_host): -> (L1, L0, q, llr) with L1 / L0 int32 [max_degree + 1, n_grid]
    (row 0 zero) = round(log p_d(q_k) 2^24) / round(log(1 - p_d(q_k)) 2^24), q / llr float32 [n_grid]"""
    D, G = int(max_degree), int(n_grid)
    L1, L0 = np.zeros((max(D, 0) + 1, max(G, 1)), np.int32), np.zeros((max(D, 0) + 1, max(G, 1)), np.int32)
    q_, llr = np.zeros(max(G, 1), np.float32), np.zeros(max(G, 1), np.float32)
    _chk(_L.qldpc_qber_table_host(D, G, float(q_lo), float(q_hi), L1.ctypes.data_as(_vp), L0.ctypes.data_as(_vp), q_.ctypes.data_as(_fp), llr.ctypes.data_as(_fp)),
         "qber_table_host")
    return L1, L0, q_, llr


def qber_counts_host(code, bits, vn_class=None, n_channel=None, syndrome=None, erase=None, known=None, value=None, _merged=False):
    """the counting kernel's mirror for ONE frame (qldpc_qber_counts_host): packed uint32 rows (bits / erase / known / value: ceil(N/32) words, syndrome:
    ceil(M/32)), vn_class uint8 [N], n_channel int (None = N) -> counts uint32 [D + 1, 2]"""
    fn, what = (_L.qldpc_qber_counts_merged_host, "qber_counts_merged_host") if _merged else (_L.qldpc_qber_counts_host, "qber_counts_host")
    Wn, Wm = (code.N + 31) // 32, (code.M + 31) // 32

    def row(a, W, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.uint32).ravel()
        if a.size != W:
            raise QldpcError(-6, "%s: %s has %d words, need %d" % (what, name, a.size, W))
        return a
    b, s, e, k, v = row(bits, Wn, "bits"), row(syndrome, Wm, "syndrome"), row(erase, Wn, "erase"), row(known, Wn, "known"), row(value, Wn, "value")
    cls = None
    if vn_class is not None:
        cls = np.ascontiguousarray(vn_class, dtype=np.uint8).ravel()
        if cls.size != code.N:
            raise QldpcError(-6, "%s: vn_class has %d entries, N = %d" % (what, cls.size, code.N))
    counts = np.zeros((QBER_MAX_DEGREE + 1 if _merged else _L.qldpc_code_max_cn_degree(code._h) + 1, 2), np.uint32)
    p = lambda a: a.ctypes.data_as(_vp) if a is not None else None
    _chk(fn(code._h, p(b), p(cls), code.N if n_channel is None else int(n_channel), p(s), p(e), p(k), p(v), p(counts)), what)
    return counts


def qber_counts_merged_host(code, bits, vn_class=None, n_channel=None, syndrome=None, erase=None, known=None, value=None):
    """the merged counting kernel's mirror for ONE frame (qldpc_qber_counts_merged_host): the arguments of qber_counts_host -> counts uint32
    [QBER_MAX_DEGREE + 1, 2], runs of checks across erased accumulator VNs counted as one observation each; status -7 for a code that is no chain"""
    return qber_counts_host(code, bits, vn_class, n_channel, syndrome, erase, known, value, _merged=True)


def qber_argmax_host(counts, L1, L0):
    """the argmax kernel's mirror (qldpc_qber_argmax_host): counts [D + 1, 2] (any integer type; a frame's or a pool's) -> grid index, -1 without an
    informative check of degree >= 1"""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    a, b = np.ascontiguousarray(L1, dtype=np.int32), np.ascontiguousarray(L0, dtype=np.int32)
    if c.ndim != 2 or c.shape[1] != 2 or a.shape != b.shape or a.ndim != 2 or a.shape[0] != c.shape[0]:
        raise QldpcError(-6, "qber_argmax_host: counts [D + 1, 2] and tables [D + 1, n_grid] are required")
    k = C.c_int(0)
    _chk(_L.qldpc_qber_argmax_host(c.ctypes.data_as(_vp), c.shape[0] - 1, a.shape[1], a.ctypes.data_as(_vp), b.ctypes.data_as(_vp), C.byref(k)), "qber_argmax_host")
    return k.value


class QberEstimator:
    """QBER of every frame from the weight of its syndrome, on the device (qldpc_qber_estimate_dev): needs no decoder, reads the packed rows the
    loads take.  estimate() returns torch tensors; llr_mag can go straight into Decoder.load_bits on the same stream."""

    def __init__(self, code, n_frames, n_grid=256, q_lo=0.001, q_hi=0.25, checks_per_block=0, device=0, merge=False):
        cfg = QberCfg()
        _L.qldpc_qber_cfg_default(C.byref(cfg))
        cfg.device, cfg.max_frames, cfg.n_grid, cfg.q_lo, cfg.q_hi, cfg.checks_per_block = int(device), int(n_frames), int(n_grid), float(q_lo), float(q_hi), int(checks_per_block)
        h = _vp()
        _chk(_L.qldpc_qber_create(code._h, C.byref(cfg), C.byref(h)), "QberEstimator")
        self._h = h
        self.code, self.N, self.M, self.D = code, code.N, code.M, _L.qldpc_code_max_cn_degree(code._h)
        self.max_frames, self.n_grid, self.device = int(n_frames), int(n_grid), int(device)
        self.q, self.llr = np.zeros(self.n_grid, np.float32), np.zeros(self.n_grid, np.float32)
        _chk(_L.qldpc_qber_grid(h, self.q.ctypes.data_as(_fp), self.llr.ctypes.data_as(_fp)), "QberEstimator.grid")
        self.rows = self.D + 1
        if merge:
            self.set_merge(True)

    def set_merge(self, on=True):
        """merging on or off (qldpc_qber_set_merge): runs of checks across erased accumulator VNs become one observation each, and the counts get
        QBER_MAX_DEGREE + 1 rows (self.rows); status -7 for a code whose parity part is no accumulator chain"""
        _chk(_L.qldpc_qber_set_merge(self._h, int(bool(on))), "QberEstimator.set_merge")
        self.rows = int(_L.qldpc_qber_count_rows(self._h))

    def set_stream(self, stream=None):
        torch = _torch()
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        _chk(_L.qldpc_qber_set_stream(self._h, _vp(s.cuda_stream)), "QberEstimator.set_stream")

    def device_bytes(self):
        return int(_L.qldpc_qber_device_bytes(self._h))

    def estimate(self, bits, vn_class=None, n_channel=None, syndrome=None, erase=None, known=None, value=None, out=None, index=True, pool=True):
        """bits / erase / known / value int32 [F, ceil(N/32)], syndrome int32 [F, ceil(M/32)], vn_class uint8 [N], n_channel int32 [F] (device tensors)
        -> dict(index int32 [F], qber float32 [F], llr_mag float32 [F], counts int32 [F, rows, 2], pool_counts int64 [rows, 2], pool_index int32 [1]), rows = D + 1,
        merged QBER_MAX_DEGREE + 1;
        asynchronous on the estimator's stream.  out = the dict of an earlier call of the same size: its tensors are written again (nothing is
        allocated); index / pool = False: the per-frame estimates / the pool are not asked for (their tensors are left alone)"""
        torch = _torch()
        Wn, Wm = (self.N + 31) // 32, (self.M + 31) // 32
        F = bits.shape[0]

        def chk(t, W, name):
            if t is None:
                return None
            assert t.is_cuda and t.dtype in (torch.int32, torch.uint32) and t.is_contiguous() and t.dim() == 2 and tuple(t.shape) == (F, W), name
            return _vp(t.data_ptr())
        pb, ps, pe, pk, pv = chk(bits, Wn, "bits"), chk(syndrome, Wm, "syndrome"), chk(erase, Wn, "erase"), chk(known, Wn, "known"), chk(value, Wn, "value")
        pc = pn = None
        if vn_class is not None:
            assert vn_class.is_cuda and vn_class.dtype == torch.uint8 and vn_class.is_contiguous() and vn_class.numel() == self.N
            pc = _vp(vn_class.data_ptr())
        if n_channel is not None:
            assert n_channel.is_cuda and n_channel.dtype == torch.int32 and n_channel.is_contiguous() and n_channel.numel() == F
            pn = _vp(n_channel.data_ptr())
        dev = bits.device
        if out is None:
            out = dict(index=torch.empty(F, dtype=torch.int32, device=dev), qber=torch.empty(F, dtype=torch.float32, device=dev),
                       llr_mag=torch.empty(F, dtype=torch.float32, device=dev), counts=torch.empty((F, self.rows, 2), dtype=torch.int32, device=dev),
                       pool_counts=torch.empty((self.rows, 2), dtype=torch.int64, device=dev), pool_index=torch.empty(1, dtype=torch.int32, device=dev))
        assert out["counts"].shape[0] == F and out["counts"].shape[1] == self.rows
        ptr = lambda name, on: _vp(out[name].data_ptr()) if on else None
        _chk(_L.qldpc_qber_estimate_dev(self._h, pb, pc, pn, ps, pe, pk, pv, F, ptr("counts", True), ptr("index", index), ptr("qber", index),
                                        ptr("llr_mag", index), ptr("pool_counts", pool), ptr("pool_index", pool)), "QberEstimator.estimate")
        return out

    def __del__(self):
        try:
            _L.qldpc_qber_free(self._h)
        except Exception:
            pass


# ---- reconciliation sessions (engine of the ecd2 LDPC handler) ---------------------------------

class ReconCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("efficiency", C.c_float), ("n_rates", C.c_int), ("rates", C.c_float * 8),
                ("n_ite", C.c_int), ("rule", C.c_int), ("rule_param", C.c_float), ("key_quantum", C.c_int),
                ("max_blocks", C.c_int), ("seed", C.c_uint64), ("schedule", C.c_int), ("mother_step", C.c_int), ("mother_max", C.c_int),
                ("rate_gap", C.c_float), ("puncture", C.c_int), ("preload", C.c_int), ("peg_depth", C.c_int), ("gap_profile", C.c_int)]


class ReconMsg(C.Structure):
    _fields_ = [("rate_index", C.c_uint32), ("key_bits", C.c_uint32), ("code_k", C.c_uint32), ("code_m", C.c_uint32),
                ("crc32", C.c_uint32), ("n_punct", C.c_uint32)]


_up = C.POINTER(C.c_uint32)
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
class ReconBlind(C.Structure):
    _fields_ = [("n_known", C.c_int), ("cap", C.c_int), ("pos", _ip), ("bit", C.POINTER(C.c_uint8)), ("n_ask", C.c_int), ("ask", _ip)]


_sig("qldpc_recon_decode_blind", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), C.POINTER(ReconBlind), C.c_int, _ip, _ip, _ip, _ip])
_sig("qldpc_recon_disclose_host", C.c_int, [_up, C.c_int, _ip, C.c_int, C.POINTER(C.c_uint8)])
# a qldpc_recon_guess per block, as a structured array
RECON_GUESS_DTYPE = np.dtype([(f, np.int32) for f in ("tried", "winner", "n_ok", "n_pass", "ambiguous", "trial_iterations")])
_sig("qldpc_recon_decode_guess", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _fp, C.POINTER(ReconMsg), C.POINTER(_up), C.c_int, _vp, _ip, _ip, _ip])
_sig("qldpc_recon_guess_settle_dev", C.c_int, [C.c_int] * 4 + [_vp] * 12 + [_vp])
_sig("qldpc_recon_guess_settle_host", C.c_int, [C.c_int] * 4 + [_up, _ip, _ip, _up, _ip, _up, _ip, _ip, _up, _up, _ip, _ip])
_sig("qldpc_crc32_words_chunked", C.c_uint32, [_up, C.c_int, C.c_int])
_sig("qldpc_recon_parity_words", C.c_int, [C.POINTER(ReconMsg)])
_sig("qldpc_recon_leaked_bits", C.c_int, [C.POINTER(ReconMsg)])
_sig("qldpc_recon_entries_created", C.c_long, [_vp])
_sig("qldpc_recon_check_header", C.c_int, [_vp, C.POINTER(ReconMsg), C.c_int])
_sig("qldpc_recon_profile_enable", C.c_int, [_vp, C.c_int])
_sig("qldpc_recon_profile_read", C.c_int, [_vp, C.POINTER(KernelStat), C.c_int])


_sig("qldpc_privamp", C.c_int, [C.c_int, _up, C.c_int, C.c_uint32, C.c_int, _up])
_sig("qldpc_privamp_dev", C.c_int, [_vp, C.c_int, C.c_uint32, C.c_int, _vp, _vp])


def privamp(key_words, workbits, seed, final_bits, device=0):
    """privAmp_doPrivAmp's hash (priv_amp.c:213-218) on the GPU: -> ceil(final_bits/32) words, MSB-first."""
    kw = np.ascontiguousarray(key_words, dtype=np.uint32)
    out = np.zeros((int(final_bits) + 31) // 32, np.uint32)
    _chk(_L.qldpc_privamp(int(device), kw.ctypes.data_as(_up), int(workbits), int(seed) & 0xFFFFFFFF, int(final_bits),
                          out.ctypes.data_as(_up)), "privamp")
    return out


_sig("qldpc_privamp_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_privamp_free", None, [_vp])
_sig("qldpc_privamp_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_privamp_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, _up, _ip, C.POINTER(_up)])
_sig("qldpc_privamp_blocks_dev", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _ip, _up, _ip, _vp, C.c_size_t, _vp])
_sig("qldpc_privamp_key_functional", C.c_uint32, [_up, C.c_int, C.c_int])
_sig("qldpc_privamp_expand_host", C.c_int, [C.c_uint32, C.c_int, C.c_uint32, C.c_int, _up])


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


class PrivAmp:
    """privAmp_doPrivAmp's hash for batches of blocks of any mix of lengths, one launch per call (qldpc_privamp_blocks*).
    Everything is allocated here; blocks() / blocks_dev() allocate nothing on the device."""

    def __init__(self, device=0, max_blocks=64, max_key_bits=1 << 16, max_final_bits=1 << 16):
        h = _vp()
        _chk(_L.qldpc_privamp_create(int(device), int(max_blocks), int(max_key_bits), int(max_final_bits), C.byref(h)), "PrivAmp")
        self._h = h
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

    def __del__(self):
        try:
            _L.qldpc_privamp_free(self._h)
        except Exception:
            pass


# ---- Toeplitz-hash privacy amplification (qldpc_toeplitz_*): y_i = XOR_j x_j t_(i+j), the caller's seed of n + m - 1 bits ----------

_sig("qldpc_toeplitz_seed_words", C.c_size_t, [C.c_int, C.c_int])
_sig("qldpc_toeplitz_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_toeplitz_free", None, [_vp])
_sig("qldpc_toeplitz_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_toeplitz_blocks", C.c_int, [_vp, C.c_int, C.POINTER(_up), _ip, C.POINTER(_up), _ip, C.POINTER(_up)])
_sig("qldpc_toeplitz_blocks_dev", C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _ip, _vp, C.c_size_t, _ip, _vp, C.c_size_t, _vp])
_sig("qldpc_toeplitz_host", C.c_int, [_up, C.c_int, _up, C.c_int, C.c_int, _up])


class _ToeplitzCfg(C.Structure):
    _fields_ = [("device", C.c_int), ("max_blocks", C.c_int), ("max_key_bits", C.c_int), ("max_out_bits", C.c_int),
                ("method", C.c_int), ("pass_log2", C.c_int), ("work_bytes", C.c_size_t)]


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


class Toeplitz:
    """Toeplitz hashing for batches of blocks of any mix of lengths, one launch per call (qldpc_toeplitz_blocks*).  The seeds are the
    caller's: key_bits + out_bits - 1 uniformly random bits per block, which may be public and shared by the blocks of a call.
    Everything is allocated here; blocks() / blocks_dev() allocate nothing on the device.  method "direct" is the n x m product;
    "ntt" gives the same words by three number-theoretic transforms per block, for long keys (pass_log2: 0 = the production pass kernels,
    TOEPLITZ_PASS_LOG2_SMALL = the small instance; work_bytes: the work area, 0 = the library's default).  Nothing picks the method for
    the caller."""

    def __init__(self, max_blocks=64, max_key_bits=1 << 16, max_out_bits=1 << 16, device=0, method="direct", pass_log2=0, work_bytes=0):
        if method not in TOEPLITZ_METHODS:
            raise QldpcError(-1, "Toeplitz: method %r (one of %s)" % (method, sorted(TOEPLITZ_METHODS)))
        if int(work_bytes) < 0:
            raise QldpcError(-6, "Toeplitz: work_bytes = %d" % work_bytes)
        cfg = _ToeplitzCfg()
        _L.qldpc_toeplitz_cfg_default(C.byref(cfg))
        cfg.device, cfg.max_blocks, cfg.max_key_bits, cfg.max_out_bits = int(device), int(max_blocks), int(max_key_bits), int(max_out_bits)
        cfg.method, cfg.pass_log2, cfg.work_bytes = TOEPLITZ_METHODS[method], int(pass_log2), int(work_bytes)
        h = _vp()
        _chk(_L.qldpc_toeplitz_create_cfg(C.byref(cfg), C.byref(h)), "Toeplitz")
        self._h = h
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

    def __del__(self):
        try:
            _L.qldpc_toeplitz_free(self._h)
        except Exception:
            pass


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


class PolyHash:
    """Error verification for batches of blocks of any mix of lengths, one launch per call (qldpc_polyhash_blocks*): polynomial evaluation
    over 2^61 - 1 with the length as a coefficient, n_keys independent keys per block.  The keys are the caller's: two uniformly random words
    (hi, lo) per key, chosen after the blocks are fixed; the blocks of a call may share them.  A tag is 2 n_keys words.  Everything is
    allocated here; blocks() / blocks_dev() allocate nothing on the device.  tile_words: 0 = the production tile,
    POLYHASH_TILE_WORDS_SMALL = the small instance; the tags do not depend on it."""

    def __init__(self, max_blocks=64, max_key_bits=1 << 16, n_keys=1, device=0, tile_words=0):
        cfg = _PolyHashCfg()
        _L.qldpc_polyhash_cfg_default(C.byref(cfg))
        cfg.device, cfg.max_blocks, cfg.max_key_bits, cfg.n_keys, cfg.tile_words = int(device), int(max_blocks), int(max_key_bits), int(n_keys), int(tile_words)
        h = _vp()
        _chk(_L.qldpc_polyhash_create_cfg(C.byref(cfg), C.byref(h)), "PolyHash")
        self._h = h
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

    def __del__(self):
        try:
            _L.qldpc_polyhash_free(self._h)
        except Exception:
            pass


# ---- Monte-Carlo FER loop (qldpc_mc_*): frame i is a pure function of (seed, i); source, channel and monitor run on the device -------

class McCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("batch", C.c_int), ("fail_cap", C.c_int), ("parity_ber", C.c_double), ("reserved", C.c_int * 2)]


class McResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("frames", "bit_errors", "frame_errors", "undetected", "not_converged", "iter_sum", "iter_max",
                                          "channel_flips", "channel_bits", "batches", "next_frame")] + [(n, C.c_double) for n in ("decode_ms", "source_ms", "encode_ms", "channel_ms", "load_ms", "monitor_ms", "total_ms")]


_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
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

_dp = C.POINTER(C.c_double)
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
_fp = C.POINTER(C.c_float)
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


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


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
    s = stream if stream is not None else torch.cuda.current_stream(weak.device)
    with torch.cuda.device(weak.device):
        _chk(_L.qldpc_guess_expand_dev(N, g, n, ptr(weak), ptr(hard), ptr(known), ptr(value), _vp(s.cuda_stream)), "guess_expand")
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
    s = stream if stream is not None else torch.cuda.current_stream(out_hard.device)
    with torch.cuda.device(out_hard.device):
        _chk(_L.qldpc_guess_pick_dev(N, g, n, op, rp, _vp(win.data_ptr()), _vp(nok.data_ptr()), _vp(amb.data_ptr()), hp, _vp(s.cuda_stream)), "guess_pick")
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


class MonteCarlo:
    """The harness's loop source -> encoder -> BSC -> decoder -> monitor on the device (qldpc_mc_*), around a Decoder and an Encoder of
    the same code, which it keeps alive but does not own.  Frame i is a pure function of (seed, i): run() over [first_frame, first_frame +
    max_frames) gives the same counters whatever the batch, and ranges add up."""

    def __init__(self, decoder, encoder, vn_class=None, seed=0, batch=0, parity_ber=0.0, fail_cap=1024):
        cfg = McCfg()
        _L.qldpc_mc_cfg_default(C.byref(cfg))
        cfg.seed, cfg.batch, cfg.fail_cap, cfg.parity_ber = _u64(seed), int(batch), int(fail_cap), float(parity_ber)
        cls = _mc_class_arg(vn_class, decoder.N, "MonteCarlo")
        h = _vp()
        _chk(_L.qldpc_mc_create(decoder._h, encoder._h, _ptr(cls, _u8p), C.byref(cfg), C.byref(h)), "MonteCarlo")
        self._h = h
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
        dev = "cuda:%d" % self.device
        info = torch.empty((n, (self.K + 31) // 32), dtype=torch.int32, device=dev)
        cw = torch.empty((n, (self.N + 31) // 32), dtype=torch.int32, device=dev)
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
        llr = _torch().empty((n, self.N), dtype=_torch().float32, device=cw.device)
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
        torch = _torch()
        n = int(n_patterns)
        rows = torch.empty((max(n, 0), (self.N + 31) // 32), dtype=torch.int32, device="cuda:%d" % self.device)
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

    def __del__(self):
        try:
            _L.qldpc_mc_free(self._h)
        except Exception:
            pass


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
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(s):
        _chk(_L.qldpc_recon_guess_settle_dev(g, n, Wk, Wn, *ptrs, _vp(passed.data_ptr()), _vp(crc.data_ptr()), _vp(res_keys.data_ptr()), _vp(res.data_ptr()),
                                             _vp(guess.data_ptr()), _vp(s.cuda_stream)), "recon_guess_settle")
        host = [t.cpu().numpy() for t in (res_keys, res, guess, passed, crc)]
    return _settle_result(n, host[0].view(np.uint32), host[1][:, :n], np.ascontiguousarray(host[2][:n]), host[3][:slots], host[4][:slots].view(np.uint32))


class Recon:
    """One side's reconciliation engine: what an ecd2 LDPC handler calls (qber_estim.c:337-340,420-423)."""

    def __init__(self, device=0, efficiency=1.4, rates=(0.5, 0.7, 0.8, 0.9), n_ite=None, rule=None, rule_param=None,
                 key_quantum=1024, max_blocks=1, seed=7, schedule="auto", mother_step=None, mother_max=None, rate_gap=None,
                 puncture=True, preload=False, peg_depth=None, gap_profile=0):
        cfg = ReconCfg()
        _L.qldpc_recon_cfg_default(C.byref(cfg))
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
        h = _vp()
        _chk(_L.qldpc_recon_create(C.byref(cfg), C.byref(h)), "Recon")
        self._h = h
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
        arr = (KernelStat * 16)()
        n = _L.qldpc_recon_profile_read(self._h, arr, 16)
        _chk(n, "Recon.profile_read")
        return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), total_ms=float(arr[i].total_ms),
                     alg_bytes=float(arr[i].alg_bytes), moved_bytes=float(arr[i].moved_bytes)) for i in range(n)]

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
        st, co, it = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        _chk(_L.qldpc_recon_decode_batch(self._h, n, kw.ctypes.data_as(_up), int(key_bits), qb.ctypes.data_as(_fp), arr,
                                         par.ctypes.data_as(_up), st.ctypes.data_as(_ip), co.ctypes.data_as(_ip),
                                         it.ctypes.data_as(_ip)), "Recon.decode_batch")
        return st, kw, co, it

    def encode_blocks(self, keys, key_bits, qber):
        """Alice's side for a list of blocks: returns (msgs, parities), one ReconMsg / uint32 array per block"""
        n = len(keys)
        kws = [np.ascontiguousarray(k, dtype=np.uint32) for k in keys]
        kb = np.ascontiguousarray(key_bits, dtype=np.int32)
        qb = np.ascontiguousarray(qber, dtype=np.float32)
        plans = [self.plan(int(b), float(p)) for b, p in zip(kb, qb)]
        pars = [np.zeros(self.parity_words(m), np.uint32) for m in plans]
        caps = np.array([p.size for p in pars], np.int32)
        kp = (_up * n)(*[k.ctypes.data_as(_up) for k in kws])
        pp = (_up * n)(*[p.ctypes.data_as(_up) for p in pars])
        arr = (ReconMsg * n)()
        _chk(_L.qldpc_recon_encode_blocks(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, caps.ctypes.data_as(_ip)),
             "Recon.encode_blocks")
        return [arr[i] for i in range(n)], pars

    def decode_blocks(self, keys, key_bits, qber, msgs, parities):
        """blocks of any mix of lengths / plans: lists of per-block uint32 arrays; returns (status[], corrected keys, corrected[], iterations[])"""
        n = len(keys)
        kws = [np.array(k, dtype=np.uint32, copy=True) for k in keys]
        pars = [np.ascontiguousarray(p, dtype=np.uint32) for p in parities]
        kp = (_up * n)(*[k.ctypes.data_as(_up) for k in kws])
        pp = (_up * n)(*[p.ctypes.data_as(_up) for p in pars])
        kb = np.ascontiguousarray(key_bits, dtype=np.int32)
        qb = np.ascontiguousarray(qber, dtype=np.float32)
        arr = (ReconMsg * n)(*msgs)
        st, co, it = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        _chk(_L.qldpc_recon_decode_blocks(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, st.ctypes.data_as(_ip),
                                          co.ctypes.data_as(_ip), it.ctypes.data_as(_ip)), "Recon.decode_blocks")
        return st, kws, co, it

    def estimate_blocks(self, keys, key_bits, msgs, parities, merge=False):
        """Bob's QBER estimate of every block out of its parity message (qldpc_recon_estimate_blocks), before any decode: returns (qber float32 [n],
        counts uint32 [n, QBER_MAX_DEGREE + 1, 2], pooled qber over the call); keys are not touched.  merge=True (qldpc_recon_estimate_blocks_merged):
        runs of checks across punctured parity bits count as one observation each, so a block with half of its parity punctured or more has an estimate"""
        n = len(keys)
        kws = [np.ascontiguousarray(k, dtype=np.uint32) for k in keys]
        pars = [np.ascontiguousarray(p, dtype=np.uint32) for p in parities]
        kp = (_up * n)(*[k.ctypes.data_as(_up) for k in kws])
        pp = (_up * n)(*[p.ctypes.data_as(_up) for p in pars])
        kb = np.ascontiguousarray(key_bits, dtype=np.int32)
        arr = (ReconMsg * n)(*msgs)
        qb, counts, pool = np.zeros(n, np.float32), np.zeros((n, QBER_MAX_DEGREE + 1, 2), np.uint32), C.c_float(0.0)
        fn = _L.qldpc_recon_estimate_blocks_merged if merge else _L.qldpc_recon_estimate_blocks
        _chk(fn(self._h, n, kp, kb.ctypes.data_as(_ip), arr, pp, qb.ctypes.data_as(_fp), counts.ctypes.data_as(_up), C.byref(pool)), "Recon.estimate_blocks")
        return qb, counts, float(pool.value)

    def decode_blind(self, keys, key_bits, qber, msgs, parities, known, ask_bits):
        """one round of blind reconciliation (qldpc_recon_decode_blind): decode_blocks with known[i] = (positions, Alice's bits there) pinned;
        returns (status[], corrected keys, corrected[], iterations[], leaked[], asks) where asks[i] = the ascending positions block i asks for
        next (empty unless its status is QLDPC_EDECODE)"""
        n = len(keys)
        kws = [np.array(k, dtype=np.uint32, copy=True) for k in keys]
        pars = [np.ascontiguousarray(p, dtype=np.uint32) for p in parities]
        kp = (_up * n)(*[k.ctypes.data_as(_up) for k in kws])
        pp = (_up * n)(*[p.ctypes.data_as(_up) for p in pars])
        kb = np.ascontiguousarray(key_bits, dtype=np.int32)
        qb = np.ascontiguousarray(qber, dtype=np.float32)
        arr = (ReconMsg * n)(*msgs)
        pos = [_np_i32(k[0]).ravel() for k in known]
        bit = [np.ascontiguousarray(k[1], dtype=np.uint8).ravel() for k in known]
        ask = [np.zeros(max(1, int(ask_bits)), np.int32) for _ in range(n)]
        bl = (ReconBlind * n)()
        for i in range(n):
            if pos[i].size != bit[i].size:
                raise QldpcError(-1, "Recon.decode_blind: block %d has %d positions and %d bits" % (i, pos[i].size, bit[i].size))
            bl[i].n_known = bl[i].cap = pos[i].size
            bl[i].pos, bl[i].bit, bl[i].ask = pos[i].ctypes.data_as(_ip), bit[i].ctypes.data_as(C.POINTER(C.c_uint8)), ask[i].ctypes.data_as(_ip)
        st, co, it, lk = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        _chk(_L.qldpc_recon_decode_blind(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, bl, int(ask_bits), st.ctypes.data_as(_ip),
                                         co.ctypes.data_as(_ip), it.ctypes.data_as(_ip), lk.ctypes.data_as(_ip)), "Recon.decode_blind")
        return st, kws, co, it, lk, [ask[i][:bl[i].n_ask].copy() for i in range(n)]

    def decode_guess(self, keys, key_bits, qber, msgs, parities, guess_bits):
        """decode_blocks with guessing rounds (qldpc_recon_decode_guess): a block whose first decode fails is decoded again with its guess_bits weakest key
        positions pinned to each of the 2^guess_bits values, and the lowest trial with a zero syndrome and Alice's CRC is kept; nothing is disclosed.
        Returns (status[], corrected keys, corrected[], iterations[], guess) with guess a RECON_GUESS_DTYPE array, one row per block"""
        n = len(keys)
        kws = [np.array(k, dtype=np.uint32, copy=True) for k in keys]
        pars = [np.ascontiguousarray(p, dtype=np.uint32) for p in parities]
        kp = (_up * n)(*[k.ctypes.data_as(_up) for k in kws])
        pp = (_up * n)(*[p.ctypes.data_as(_up) for p in pars])
        kb = np.ascontiguousarray(key_bits, dtype=np.int32)
        qb = np.ascontiguousarray(qber, dtype=np.float32)
        arr = (ReconMsg * n)(*msgs)
        st, co, it = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        guess = np.zeros(n, RECON_GUESS_DTYPE)
        guess["winner"] = -1
        _chk(_L.qldpc_recon_decode_guess(self._h, n, kp, kb.ctypes.data_as(_ip), qb.ctypes.data_as(_fp), arr, pp, int(guess_bits), _vp(guess.ctypes.data),
                                         st.ctypes.data_as(_ip), co.ctypes.data_as(_ip), it.ctypes.data_as(_ip)), "Recon.decode_guess")
        return st, kws, co, it, guess

    def prepare_decode(self, keys, key_bits, qber, msgs, parities):
        """decode_blocks with the argument marshalling done once: returns an object whose run() is the one C call
        (qldpc_recon_decode_blocks) and nothing else -- what a C caller's timed region contains"""
        return _PreparedDecode(self, keys, key_bits, qber, msgs, parities)

    def __del__(self):
        try:
            _L.qldpc_recon_free(self._h)
        except Exception:
            pass


class _PreparedDecode:
    def __init__(self, recon, keys, key_bits, qber, msgs, parities):
        self._r = recon
        self.n = n = len(keys)
        self._orig = [np.ascontiguousarray(k, dtype=np.uint32) for k in keys]
        self.keys = [k.copy() for k in self._orig]
        self._pars = [np.ascontiguousarray(p_, dtype=np.uint32) for p_ in parities]
        self._kp = (_up * n)(*[k.ctypes.data_as(_up) for k in self.keys])
        self._pp = (_up * n)(*[p_.ctypes.data_as(_up) for p_ in self._pars])
        self._kb = np.ascontiguousarray(key_bits, dtype=np.int32)
        self._qb = np.ascontiguousarray(qber, dtype=np.float32)
        self._msgs = (ReconMsg * n)(*msgs)
        self.status, self.corrected, self.iterations = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)

    def reset(self):
        """Bob's uncorrected keys again (the decode works in place)"""
        for k, o in zip(self.keys, self._orig):
            k[:] = o

    def run(self):
        _chk(_L.qldpc_recon_decode_blocks(self._r._h, self.n, self._kp, self._kb.ctypes.data_as(_ip), self._qb.ctypes.data_as(_fp), self._msgs, self._pp,
                                          self.status.ctypes.data_as(_ip), self.corrected.ctypes.data_as(_ip), self.iterations.ctypes.data_as(_ip)),
             "Recon.decode_blocks")

"""The parity-check matrix and its encoder (qldpc_code_*, qldpc_encoder_*), the scalar helpers and the packed-bit layout.

(Not `code.py`: bench.py puts this directory on sys.path to import `shard`, where that name would hide the standard library's.)"""
import ctypes as C
import os

import numpy as np

from ._lib import _L, _Handle, _chk, _create, _dev_empty, _dev_rows, _ip, _np_i32, _sig, _stream_arg, _torch, _vp, QldpcError

RULES = {"MS": 0, "OMS": 1, "NMS": 2, "SPA": 3, "LSPA": 4, "AMS_MIN": 5, "AMS_MINSTAR_L2": 6, "AMS_MINSTAR": 7}
SCHEDULES = {"flooding": 0, "hlayered": 1, "vlayered": 3}      # 2 is QLDPC_RECON_SCHED_AUTO (sessions only)
VN_CHANNEL, VN_PINNED, VN_PUNCTURED = 0, 1, 2
CONFIRMED_BIT_LLR = 23.025850929840455

_sig("qldpc_version", C.c_int, [])
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
_sig("qldpc_encoder_create", C.c_int, [_vp, C.c_char_p, C.c_int, C.POINTER(_vp)])
_sig("qldpc_encoder_free", None, [_vp])
_sig("qldpc_encoder_reserve", C.c_int, [_vp, C.c_int])
_sig("qldpc_encoder_k", C.c_int, [_vp])
_sig("qldpc_encoder_info_bits_pos", C.c_int, [_vp, _ip])
_sig("qldpc_encode", C.c_int, [_vp, _ip, _ip, C.c_int])
_sig("qldpc_encode_packed_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp])


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


class Code(_Handle):
    """Parity-check matrix H (tools::Sparse_matrix as the harness holds it; rows = variable nodes)."""
    _free = _L.qldpc_code_free

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
        return cls(_create("Code.from_alist", _L.qldpc_code_from_alist, os.fsencode(path)).value)

    @classmethod
    def from_qc(cls, path):
        return cls(_create("Code.from_qc", _L.qldpc_code_from_qc, os.fsencode(path)).value)

    @classmethod
    def from_edges(cls, N, M, var, chk):
        var, chk = _np_i32(var), _np_i32(chk)
        if var.shape != chk.shape:
            raise QldpcError(-6, "Code.from_edges")
        return cls(_create("Code.from_edges", _L.qldpc_code_from_edges, int(N), int(M), int(var.size), var.ctypes.data_as(_ip), chk.ctypes.data_as(_ip)).value)

    @classmethod
    def ira(cls, N, K, hi_frac=0.125, dv_hi=11, dv_lo=3, seed=7):
        return cls(_create("Code.ira", _L.qldpc_code_ira, int(N), int(K), float(hi_frac), int(dv_hi), int(dv_lo), int(seed)).value)

    @classmethod
    def ira_peg(cls, N, K, hi_frac=0.125, dv_hi=11, dv_lo=3, depth=2, seed=7):
        """IRA profile with a progressive-edge-growth information part (depth 2: no 4-cycles)."""
        return cls(_create("Code.ira_peg", _L.qldpc_code_ira_peg, int(N), int(K), float(hi_frac), int(dv_hi), int(dv_lo), int(depth), int(seed)).value)

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


class Encoder(_Handle):
    """m.encoder->encode (BS/src/main.cpp:341): method 'IRA', 'IDENTITY' / 'LU_DEC' (Encoder_LDPC_from_H's G_methods) or 'QC' (Encoder_LDPC_from_QC)."""
    _free = _L.qldpc_encoder_free

    def __init__(self, code, method="IDENTITY", device=0):
        self._h = _create("Encoder", _L.qldpc_encoder_create, code._h, method.encode(), int(device))
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
        p = _dev_rows(info, None, (self.K + 31) // 32, (torch.int32,), "info")
        out = _dev_empty(info.device, (info.shape[0], (self.N + 31) // 32), torch.int32)
        _chk(_L.qldpc_encode_packed_dev(self._h, p, _vp(out.data_ptr()), info.shape[0], _stream_arg(stream, self.device)), "encode_packed")
        return out


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

"""QBER from the syndrome weight (qldpc_qber_*): the estimator on the device and the host mirrors of its tables and kernels."""
import ctypes as C

import numpy as np

from ._lib import _L, _Handle, _chk, _create, _default, _dev_empty, _dev_rows, _dev_vec, _fp, _ip, _sig, _stream_arg, _torch, _vp, QldpcError

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


class QberEstimator(_Handle):
    """QBER of every frame from the weight of its syndrome, on the device (qldpc_qber_estimate_dev): needs no decoder, reads the packed rows the
    loads take.  estimate() returns torch tensors; llr_mag can go straight into Decoder.load_bits on the same stream."""
    _free = _L.qldpc_qber_free

    def __init__(self, code, n_frames, n_grid=256, q_lo=0.001, q_hi=0.25, checks_per_block=0, device=0, merge=False):
        cfg = _default(QberCfg, _L.qldpc_qber_cfg_default)
        cfg.device, cfg.max_frames, cfg.n_grid, cfg.q_lo, cfg.q_hi, cfg.checks_per_block = int(device), int(n_frames), int(n_grid), float(q_lo), float(q_hi), int(checks_per_block)
        self._h = h = _create("QberEstimator", _L.qldpc_qber_create, code._h, C.byref(cfg))
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
        _chk(_L.qldpc_qber_set_stream(self._h, _stream_arg(stream, self.device)), "QberEstimator.set_stream")

    def device_bytes(self):
        return int(_L.qldpc_qber_device_bytes(self._h))

    def estimate(self, bits, vn_class=None, n_channel=None, syndrome=None, erase=None, known=None, value=None, out=None, index=True, pool=True):
        """bits / erase / known / value int32 [F, ceil(N/32)], syndrome int32 [F, ceil(M/32)], vn_class uint8 [N], n_channel int32 [F] (device tensors)
        -> dict(index int32 [F], qber float32 [F], llr_mag float32 [F], counts int32 [F, rows, 2], pool_counts int64 [rows, 2], pool_index int32 [1]), rows = D + 1,
        merged QBER_MAX_DEGREE + 1;
        asynchronous on the estimator's stream.  out = the dict of an earlier call of the same size: its tensors are written again (nothing is
        allocated); index / pool = False: the per-frame estimates / the pool are not asked for (their tensors are left alone)"""
        torch = _torch()
        Wn, Wm, words = (self.N + 31) // 32, (self.M + 31) // 32, (torch.int32, torch.uint32)
        F = bits.shape[0]
        pb, ps, pe, pk, pv = (_dev_rows(t, F, W, words, name) for t, W, name in ((bits, Wn, "bits"), (syndrome, Wm, "syndrome"), (erase, Wn, "erase"),
                                                                                 (known, Wn, "known"), (value, Wn, "value")))
        pc, pn = _dev_vec(vn_class, self.N, torch.uint8, "vn_class"), _dev_vec(n_channel, F, torch.int32, "n_channel")
        if out is None:
            new = lambda shape, dtype: _dev_empty(bits.device, shape, dtype)
            out = dict(index=new(F, torch.int32), qber=new(F, torch.float32), llr_mag=new(F, torch.float32), counts=new((F, self.rows, 2), torch.int32),
                       pool_counts=new((self.rows, 2), torch.int64), pool_index=new(1, torch.int32))
        assert out["counts"].shape[0] == F and out["counts"].shape[1] == self.rows
        ptr = lambda name, on: _vp(out[name].data_ptr()) if on else None
        _chk(_L.qldpc_qber_estimate_dev(self._h, pb, pc, pn, ps, pe, pk, pv, F, ptr("counts", True), ptr("index", index), ptr("qber", index),
                                        ptr("llr_mag", index), ptr("pool_counts", pool), ptr("pool_index", pool)), "QberEstimator.estimate")
        return out

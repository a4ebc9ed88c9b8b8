"""Polar codes (qldpc_polar_*): the batched encoder, the successive-cancellation decoder and the CRC-aided list decoder on the device, their
host mirrors, a polarization-weight order for callers without a standard's reliability table, and the genie-aided construction that fits an
information set to a channel (the tally on the device and on the host, the order and the K of a tally)."""
import ctypes as C

import numpy as np

from ._lib import _L, _Handle, _chk, _create, _dev_empty, _dev_rows, _ip, _ptr, _sig, _stream_arg, _torch, _u64p, _up, _vp, QldpcError

POLAR_I8, POLAR_F32 = 0, 1
POLAR_FORMS = {"lanes": 0, "wide": 1}
POLAR_RULES = {"sc": 0, "ssc": 1}
POLAR_SSC_KINDS = ("rate0", "rate1", "mixed")      # the kinds of a plan's steps, by their number
POLAR_MAX_LOG2N = 20
POLAR_LIST_MAX_LOG2N = 16
POLAR_CRC11 = (11, 0x621)          # the CRC of the reference's list decoder: crc_len, crc_poly

_sig("qldpc_polar_create", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_polar_create_form", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_polar_create_rule", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_polar_free", None, [_vp])
_sig("qldpc_polar_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_polar_set_stream", C.c_int, [_vp, _vp])
_sig("qldpc_polar_encode_dev", C.c_int, [_vp, C.c_int, _vp, _vp])
_sig("qldpc_polar_decode_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_decode_rows_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_encode_host", C.c_int, [C.c_int, C.c_int, _up, _up])
_sig("qldpc_polar_decode_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, _vp, _up, _up, _up, _up, _vp])
_sig("qldpc_polar_decode_rows_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, _vp, _up, _up, _up, _up, _up, _vp])
_sig("qldpc_polar_decode_wide_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, _vp, _up, _up, _up, _up, _vp])
_sig("qldpc_polar_decode_ssc_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, _vp, _up, _up, _up, _up])
_sig("qldpc_polar_ssc_plan_host", C.c_int, [C.c_int, C.c_int, _ip, _ip, _ip])
_sig("qldpc_polar_list_create", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_polar_list_free", None, [_vp])
_sig("qldpc_polar_list_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_polar_list_set_stream", C.c_int, [_vp, _vp])
_sig("qldpc_polar_list_decode_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_list_decode_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, _vp, _up, _up, _up, _up, _up,
                                               _ip, _vp, _up])
_sig("qldpc_polar_crc_host", C.c_int, [C.c_int, C.c_uint32, C.c_int, C.c_int, _up, _up])
_sig("qldpc_polar_tally_dev", C.c_int, [_vp, C.c_int, _vp, _vp, _vp])
_sig("qldpc_polar_tally_host", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _vp, _up, _u64p])
_sig("qldpc_polar_construct_order_host", C.c_int, [C.c_int, _u64p, _ip, _ip])
_sig("qldpc_polar_construct_k_host", C.c_int, [C.c_int, _u64p, _ip, C.c_uint64, _ip])


def _messages(messages):
    if messages in ("i8", POLAR_I8):
        return POLAR_I8, np.int8
    if messages in ("f32", POLAR_F32):
        return POLAR_F32, np.float32
    raise QldpcError(-1, "polar: messages=%r ('i8' or 'f32')" % (messages,))


def _form(form):
    """'lanes' or 'wide'; a number goes to the library as it is, which refuses what is neither"""
    if isinstance(form, str):
        if form not in POLAR_FORMS:
            raise QldpcError(-1, "polar: form=%r ('lanes' or 'wide')" % (form,))
        return POLAR_FORMS[form]
    return int(form)


def _rule(rule):
    """'sc' or 'ssc'; a number goes to the library as it is, which refuses what is neither"""
    if isinstance(rule, str):
        if rule not in POLAR_RULES:
            raise QldpcError(-1, "polar: rule=%r ('sc' or 'ssc')" % (rule,))
        return POLAR_RULES[rule]
    return int(rule)


def _words(log2_n):
    return max(1, (1 << max(int(log2_n), 0)) // 32) if int(log2_n) <= POLAR_MAX_LOG2N else 1


def polar_pw_order(n):
    """the positions 0 .. 2^n - 1 in ascending polarization weight sum_j b_j 2^(j/4) (b_j = bit j of the position), ties by index: the least
    reliable first, so a code of K information bits takes the last K.  Pure numpy; not part of the C ABI."""
    n = int(n)
    i = np.arange(1 << n, dtype=np.int64)
    w = np.zeros(1 << n, np.float64)
    for j in range(n):
        w += ((i >> j) & 1) * 2.0 ** (j / 4.0)
    return np.argsort(w, kind="stable").astype(np.int32)


def polar_encode_host(log2_n, u):
    """the encoder's mirror (qldpc_polar_encode_host): packed rows uint32 [F, ceil(N/32)] (or one row) -> x of the same shape"""
    u = np.ascontiguousarray(u, dtype=np.uint32)
    rows = u.reshape(-1, u.shape[-1]) if u.ndim else u.reshape(1, 1)
    if rows.shape[1] != _words(log2_n):
        raise QldpcError(-6, "polar_encode_host: rows have %d words, need %d" % (rows.shape[1], _words(log2_n)))
    x = np.zeros_like(rows)
    _chk(_L.qldpc_polar_encode_host(int(log2_n), rows.shape[0], rows.ctypes.data_as(_up), x.ctypes.data_as(_up)), "polar_encode_host")
    return x.reshape(u.shape)


def _host_rows(who, log2_n, max_log2_n, info_pos, llr, frozen, messages):
    """the marshalling of (info_pos, llr, frozen) of the host decodes, which take them the same way
    -> kind, dt (the messages), pos int32 [K], llr [F, N] of dt, fz uint32 [F, W] or None, n, N (0: a size the library will refuse), W, F"""
    kind, dt = _messages(messages)
    pos = np.ascontiguousarray(info_pos, dtype=np.int32).ravel()
    llr = np.ascontiguousarray(llr, dtype=dt)
    n = int(log2_n)
    N, W = (1 << n) if 0 <= n <= max_log2_n else 0, _words(n)
    if N and (llr.ndim != 2 or llr.shape[1] != N):
        raise QldpcError(-6, "%s: llr must be [frames, N = %d]" % (who, N))
    F = llr.shape[0] if llr.ndim == 2 else 0
    fz = None
    if frozen is not None:
        fz = np.ascontiguousarray(frozen, dtype=np.uint32)
        if fz.shape != (F, W):
            raise QldpcError(-6, "%s: frozen must be [frames, %d] words" % (who, W))
    return kind, dt, pos, llr, fz, n, N, W, F


def _decode_host(fn, who, log2_n, info_pos, llr, frozen, messages, maxq, leaf):
    """the two host SC decodes, which take the same arguments"""
    kind, dt, pos, llr, fz, n, N, W, F = _host_rows(who, log2_n, POLAR_MAX_LOG2N, info_pos, llr, frozen, messages)
    out = dict(u=np.zeros((F, W), np.uint32), info=np.zeros((F, (pos.size + 31) // 32), np.uint32), x=np.zeros((F, W), np.uint32))
    if leaf:
        out["leaf"] = np.zeros((F, N), dt)
    _chk(fn(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), F, llr.ctypes.data_as(_vp), _ptr(fz, _up), _ptr(out["u"], _up), _ptr(out["info"], _up),
            _ptr(out["x"], _up), _ptr(out.get("leaf"), _vp)), who)
    return out


def polar_decode_host(log2_n, info_pos, llr, frozen=None, messages="i8", maxq=31, leaf=False):
    """the SC decoder's mirror (qldpc_polar_decode_host): llr [F, N] int8 or float32 by `messages`, frozen uint32 [F, ceil(N/32)] or None
    -> dict(u uint32 [F, W], info uint32 [F, ceil(K/32)], x uint32 [F, W]) and, with leaf=True, leaf [F, N] of the messages' type"""
    return _decode_host(_L.qldpc_polar_decode_host, "polar_decode_host", log2_n, info_pos, llr, frozen, messages, maxq, leaf)


def polar_decode_wide_host(log2_n, info_pos, llr, frozen=None, messages="i8", maxq=31, leaf=False):
    """the host walk of the wide form's memory plan (qldpc_polar_decode_wide_host): the arguments and the results of polar_decode_host, bit for bit"""
    return _decode_host(_L.qldpc_polar_decode_wide_host, "polar_decode_wide_host", log2_n, info_pos, llr, frozen, messages, maxq, leaf)


def polar_decode_rows_host(log2_n, info_pos, llr, rows, frozen=None, messages="i8", maxq=31, leaf=False):
    """the rows decode's mirror (qldpc_polar_decode_rows_host): polar_decode_host with a frozen set per frame, rows uint32 [F, ceil(N/32)]: a set
    bit freezes that position of that frame on top of the code's frozen set (to its bit of `frozen`, 0 without one) -> the dict of
    polar_decode_host"""
    who = "polar_decode_rows_host"
    kind, dt, pos, llr, fz, n, N, W, F = _host_rows(who, log2_n, POLAR_MAX_LOG2N, info_pos, llr, frozen, messages)
    rw = None
    if rows is not None:
        rw = np.ascontiguousarray(rows, dtype=np.uint32)
        if rw.shape != (F, W):
            raise QldpcError(-6, "%s: rows must be [frames, %d] words" % (who, W))
    out = dict(u=np.zeros((F, W), np.uint32), info=np.zeros((F, (pos.size + 31) // 32), np.uint32), x=np.zeros((F, W), np.uint32))
    if leaf:
        out["leaf"] = np.zeros((F, N), dt)
    _chk(_L.qldpc_polar_decode_rows_host(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), F, llr.ctypes.data_as(_vp), _ptr(fz, _up), _ptr(rw, _up),
                                         _ptr(out["u"], _up), _ptr(out["info"], _up), _ptr(out["x"], _up), _ptr(out.get("leaf"), _vp)), who)
    return out


def polar_decode_ssc_host(log2_n, info_pos, llr, frozen=None, messages="i8", maxq=31):
    """the simplified SC decoder's mirror (qldpc_polar_decode_ssc_host): the arguments of polar_decode_host without leaf -> dict(u, info, x).
    Rate-0 and rate-1 subtrees are pruned: SC bit for bit on every frame in which no belief of a rate-1 node is 0"""
    who = "polar_decode_ssc_host"
    kind, dt, pos, llr, fz, n, N, W, F = _host_rows(who, log2_n, POLAR_MAX_LOG2N, info_pos, llr, frozen, messages)
    out = dict(u=np.zeros((F, W), np.uint32), info=np.zeros((F, (pos.size + 31) // 32), np.uint32), x=np.zeros((F, W), np.uint32))
    _chk(_L.qldpc_polar_decode_ssc_host(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), F, llr.ctypes.data_as(_vp), _ptr(fz, _up), _ptr(out["u"], _up),
                                        _ptr(out["info"], _up), _ptr(out["x"], _up)), who)
    return out


def polar_ssc_plan(log2_n, info_pos):
    """the plan of a code under the SSC rule (qldpc_polar_ssc_plan_host) -> int32 [steps, 3]: first 32-leaf block, log2 of the leaves, kind (by
    POLAR_SSC_KINDS) in leaf order; one mixed step of the whole frame for N < 32"""
    pos = np.ascontiguousarray(info_pos, dtype=np.int32).ravel()
    steps = np.zeros((_words(log2_n), 3), np.int32)
    count = C.c_int(0)
    _chk(_L.qldpc_polar_ssc_plan_host(int(log2_n), pos.size, pos.ctypes.data_as(_ip), steps.ctypes.data_as(_ip), C.byref(count)), "polar_ssc_plan")
    return steps[:count.value].copy()


# ---- the genie-aided construction --------------------------------------------------------------------------------------------------------

def polar_tally_host(log2_n, llr, u_true, messages="i8", maxq=31, out=None):
    """the tally's mirror (qldpc_polar_tally_host): llr [F, N] int8 or float32 by `messages`, u_true uint32 [F, W] the frames' true rows
    -> uint64 [2, N]: the wrong frames and the ties of every position under the SC decoder that is told all earlier bits, ADDED to `out` where
    one is given"""
    who = "polar_tally_host"
    kind, dt, _, llr, tr, n, N, W, F = _host_rows(who, log2_n, POLAR_MAX_LOG2N, [], llr, u_true, messages)
    if tr is None:
        raise QldpcError(-1, "polar_tally_host: u_true is required")
    if out is None:
        out = np.zeros((2, max(N, 1)), np.uint64)
    if out.dtype != np.uint64 or out.shape != (2, max(N, 1)) or not out.flags.c_contiguous:
        raise QldpcError(-6, "polar_tally_host: out must be a contiguous uint64 [2, N]")
    _chk(_L.qldpc_polar_tally_host(n, kind, int(maxq), F, llr.ctypes.data_as(_vp), tr.ctypes.data_as(_up), out.ctypes.data_as(_u64p)), who)
    return out


def _tally_rows(wrong, ties):
    """(wrong, ties) of N = 2^n positions each -> n (0: no such size, the library's to refuse) and the [2, N] row the library takes"""
    t = np.ascontiguousarray(np.stack([np.asarray(wrong).ravel(), np.asarray(ties).ravel()]), dtype=np.uint64)
    N = t.shape[1]
    return (N.bit_length() - 1 if N >= 2 and N & (N - 1) == 0 else 0), t


def polar_construct_order(wrong, ties, prior=None):
    """the positions in ascending reliability (qldpc_polar_construct_order_host), so a code of K bits takes the last K: by the score
    2 wrong + ties descending and, among equal scores, by the rank in `prior` (an order of ascending reliability such as polar_pw_order's; None:
    by index) -> int32 [N]"""
    who = "polar_construct_order"
    n, t = _tally_rows(wrong, ties)
    pr = None
    if prior is not None:
        pr = np.ascontiguousarray(prior, dtype=np.int32).ravel()
        if pr.size != t.shape[1]:
            raise QldpcError(-6, "polar_construct_order: prior must hold N = %d positions" % t.shape[1])
    order = np.zeros(t.shape[1], np.int32)
    _chk(_L.qldpc_polar_construct_order_host(n, t.ctypes.data_as(_u64p), _ptr(pr, _ip), order.ctypes.data_as(_ip)), who)
    return order


def polar_construct_k(wrong, ties, order, frames, bound):
    """the largest K whose last K positions of `order` have estimated error probabilities that sum to at most `bound` (a union bound on the frame
    error rate of SC decoding), from a tally over `frames` frames (qldpc_polar_construct_k_host with floor(2 frames bound))"""
    who = "polar_construct_k"
    n, t = _tally_rows(wrong, ties)
    od = np.ascontiguousarray(order, dtype=np.int32).ravel()
    if od.size != t.shape[1]:
        raise QldpcError(-6, "polar_construct_k: order must hold N = %d positions" % t.shape[1])
    if not (float(bound) >= 0.0 and int(frames) >= 0):
        raise QldpcError(-1, "polar_construct_k: frames and bound must not be negative")
    k = C.c_int(0)
    _chk(_L.qldpc_polar_construct_k_host(n, t.ctypes.data_as(_u64p), od.ctypes.data_as(_ip), min(int(np.floor(2.0 * int(frames) * float(bound))), (1 << 64) - 1),
                                         C.byref(k)), who)
    return int(k.value)


class _PolarCode(_Handle):
    """what Polar and PolarList share: the code's attributes, the input checks of decode, its output dict and the stream"""

    def _create_code(self, create, log2_n, info_pos, messages, maxq, before, max_frames, after, device):
        """create(log2_n, K, info_pos, messages, maxq, *before, max_frames, *after, device) -> the handle, and the attributes both classes have"""
        self.messages, self._np_dtype = _messages(messages)
        pos = np.ascontiguousarray(info_pos, dtype=np.int32).ravel()
        self._h = _create(type(self).__name__, create, int(log2_n), pos.size, pos.ctypes.data_as(_ip), self.messages, int(maxq), *before, int(max_frames), *after,
                          int(device))
        self.log2_n, self.N, self.K, self.W, self.Wi = int(log2_n), 1 << int(log2_n), pos.size, _words(log2_n), (pos.size + 31) // 32
        self.info_pos, self.maxq, self.max_frames, self.device = pos, int(maxq), int(max_frames), int(device)

    def device_bytes(self):
        return int(self._device_bytes(self._h))

    def _on_current_stream(self):
        _chk(self._set_stream(self._h, _stream_arg(None, self.device)), "polar.set_stream")

    def _decode_inputs(self, llr, frozen):
        """llr [F, N] of the context's messages and frozen [F, W] words or None, checked -> torch, F and their pointers"""
        torch = _torch()
        pl = _dev_rows(llr, None, self.N, (torch.int8 if self.messages == POLAR_I8 else torch.float32,), "llr")
        return torch, llr.shape[0], pl, _dev_rows(frozen, llr.shape[0], self.W, (torch.int32, torch.uint32), "frozen")

    @staticmethod
    def _outputs(device, shapes, want):
        """a fresh device tensor for every name of `shapes` (name -> (shape, dtype)) that `want` names -> the dict, and ptr(name): the pointer the
        library gets for it, None where it was not asked for or is empty"""
        out = {k: _dev_empty(device, *v) for k, v in shapes.items() if k in want}
        return out, lambda name: _vp(out[name].data_ptr()) if name in out and out[name].numel() else None


class Polar(_PolarCode):
    """A polar code of N = 2^log2_n bits with information at `info_pos` (every other position frozen) on the device: encode() and the
    successive-cancellation decode() of up to max_frames frames a call.  form="lanes": 64 frames to a wave, for batches; form="wide": a workgroup
    to a frame, for few long frames.  The same function bit for bit, and the choice is the caller's.  rule="sc": every node of the tree is
    visited; rule="ssc": rate-0 and rate-1 subtrees are pruned (lanes form; no leaf output), which is SC bit for bit on every frame in which no
    belief of a rate-1 node is 0, and again the choice is the caller's.  Device tensors in, device tensors out, asynchronous on torch's current
    stream."""
    _free, _device_bytes, _set_stream = _L.qldpc_polar_free, _L.qldpc_polar_device_bytes, _L.qldpc_polar_set_stream

    def __init__(self, log2_n, info_pos, messages="i8", maxq=31, max_frames=4096, device=0, form="lanes", rule="sc"):
        self.form, self.rule = _form(form), _rule(rule)
        self._create_code(_L.qldpc_polar_create_rule, log2_n, info_pos, messages, maxq, (), max_frames, (self.form, self.rule), device)

    def encode(self, u, out=None):
        """u int32 / uint32 [F, W] packed rows on the device -> x of the same shape; out=u encodes in place"""
        torch = _torch()
        words = (torch.int32, torch.uint32)
        pu = _dev_rows(u, None, self.W, words, "u")
        x = _dev_empty(u.device, tuple(u.shape), u.dtype) if out is None else out
        px = _dev_rows(x, u.shape[0], self.W, words, "out")
        self._on_current_stream()
        _chk(_L.qldpc_polar_encode_dev(self._h, u.shape[0], pu, px), "Polar.encode")
        return x

    def decode(self, llr, frozen=None, leaf=False, want=("u", "info", "x")):
        """llr [F, N] int8 or float32 (the context's messages), frozen int32 / uint32 [F, W] frozen values or None (zeros)
        -> dict of device tensors: u int32 [F, W], info int32 [F, ceil(K/32)], x int32 [F, W] (those named in `want`) and, with leaf=True,
        leaf [F, N] of the messages' type"""
        torch, F, pl, pf = self._decode_inputs(llr, frozen)
        out, ptr = self._outputs(llr.device, dict(u=((F, self.W), torch.int32), info=((F, self.Wi), torch.int32), x=((F, self.W), torch.int32)), want)
        if leaf:
            out["leaf"] = _dev_empty(llr.device, (F, self.N), llr.dtype)
        self._on_current_stream()
        _chk(_L.qldpc_polar_decode_dev(self._h, F, pl, pf, ptr("u"), ptr("info"), ptr("x"), ptr("leaf")), "Polar.decode")
        return out

    def decode_rows(self, llr, rows, frozen=None, leaf=False, want=("u", "info", "x")):
        """decode() with a frozen set per frame (qldpc_polar_decode_rows_dev): rows int32 / uint32 [F, W], a set bit freezes that position of
        that frame on top of the code's frozen set, to its bit of `frozen` (0 without one) -> the dict of decode().  Lanes form, SC rule"""
        torch, F, pl, pf = self._decode_inputs(llr, frozen)
        pr = _dev_rows(rows, F, self.W, (torch.int32, torch.uint32), "rows")
        out, ptr = self._outputs(llr.device, dict(u=((F, self.W), torch.int32), info=((F, self.Wi), torch.int32), x=((F, self.W), torch.int32)), want)
        if leaf:
            out["leaf"] = _dev_empty(llr.device, (F, self.N), llr.dtype)
        self._on_current_stream()
        _chk(_L.qldpc_polar_decode_rows_dev(self._h, F, pl, pf, pr, ptr("u"), ptr("info"), ptr("x"), ptr("leaf")), "Polar.decode_rows")
        return out

    def tally(self, llr, u_true, out=None):
        """the genie-aided tally (qldpc_polar_tally_dev): llr [F, N] of the context's messages, u_true int32 / uint32 [F, W] the frames' true rows
        -> int64 [2, N] on the device, row 0 the wrong frames and row 1 the ties of every position, ADDED to `out` where one is given (a fresh
        row of zeros otherwise).  The context's own information set plays no part; lanes form only"""
        torch, F, pl, pu = self._decode_inputs(llr, u_true)
        if out is None:
            out = torch.zeros((2, self.N), dtype=torch.int64, device=llr.device)
        po = _dev_rows(out, 2, self.N, (torch.int64, torch.uint64), "out")
        self._on_current_stream()
        _chk(_L.qldpc_polar_tally_dev(self._h, F, pl, pu, po), "Polar.tally")
        return out


# ---- the CRC-aided list decoder ------------------------------------------------------------------------------------------------------------

LIST_OUTPUTS = ("u", "info", "x", "pick", "metric", "list_x")


def polar_crc_host(crc_len, crc_poly, bits_rows, n_bits):
    """Alice's CRC (qldpc_polar_crc_host): packed rows uint32 [F, ceil(n_bits/32)] -> the remainders uint32 [F] of the first n_bits bits of each"""
    rows = np.ascontiguousarray(bits_rows, dtype=np.uint32)
    if rows.ndim != 2 or rows.shape[1] != (max(int(n_bits), 0) + 31) // 32:
        raise QldpcError(-6, "polar_crc_host: rows must be [frames, ceil(n_bits / 32)] words")
    crc = np.zeros(rows.shape[0], np.uint32)
    _chk(_L.qldpc_polar_crc_host(int(crc_len), int(crc_poly) & 0xffffffff, int(n_bits), rows.shape[0], rows.ctypes.data_as(_up), crc.ctypes.data_as(_up)),
         "polar_crc_host")
    return crc


def polar_list_decode_host(log2_n, info_pos, llr, frozen=None, crc=None, messages="i8", maxq=31, list_size=4, crc_len=0, crc_poly=0, want=LIST_OUTPUTS):
    """the list decoder's mirror (qldpc_polar_list_decode_host): llr [F, N] int8 or float32 by `messages`, frozen uint32 [F, W] or None, crc uint32
    [F] the expected remainders or None (zeros) -> dict of those of u, info, x uint32 rows of the picked path, pick int32 [F] (-1: no path
    matched), metric [F, L] uint32 or float32, list_x uint32 [F, L, W] that `want` names"""
    who = "polar_list_decode_host"
    kind, dt, pos, llr, fz, n, N, W, F = _host_rows(who, log2_n, POLAR_LIST_MAX_LOG2N, info_pos, llr, frozen, messages)
    L, cr = int(list_size), None
    if crc is not None:
        cr = np.ascontiguousarray(crc, dtype=np.uint32)
        if cr.shape != (F,):
            raise QldpcError(-6, "polar_list_decode_host: crc must be [frames]")
    Ls = L if 1 <= L <= 8 else 1
    shapes = dict(u=((F, W), np.uint32), info=((F, (pos.size + 31) // 32), np.uint32), x=((F, W), np.uint32), pick=((F,), np.int32),
                  metric=((F, Ls), np.uint32 if kind == POLAR_I8 else np.float32), list_x=((F, Ls, W), np.uint32))
    out = {k: np.zeros(*shapes[k]) for k in LIST_OUTPUTS if k in want}
    _chk(_L.qldpc_polar_list_decode_host(n, pos.size, pos.ctypes.data_as(_ip), kind, int(maxq), L, int(crc_len), int(crc_poly) & 0xffffffff, F,
                                         llr.ctypes.data_as(_vp), _ptr(fz, _up), _ptr(cr, _up), _ptr(out.get("u"), _up), _ptr(out.get("info"), _up),
                                         _ptr(out.get("x"), _up), _ptr(out.get("pick"), _ip), _ptr(out.get("metric"), _vp), _ptr(out.get("list_x"), _up)), who)
    return out


class PolarList(_PolarCode):
    """The CRC-aided successive-cancellation list decoder of a polar code on the device: up to `list_size` (1, 2, 4, 8) paths a frame, a lane of a
    wave holding all paths of its frame, and the pick of the first path in list order whose CRC over the information bits is the expected one.
    Device tensors in, device tensors out, asynchronous on torch's current stream."""
    _free, _device_bytes, _set_stream = _L.qldpc_polar_list_free, _L.qldpc_polar_list_device_bytes, _L.qldpc_polar_list_set_stream

    def __init__(self, log2_n, info_pos, messages="i8", maxq=31, list_size=4, crc_len=0, crc_poly=0, max_frames=4096, device=0):
        self._create_code(_L.qldpc_polar_list_create, log2_n, info_pos, messages, maxq, (int(list_size), int(crc_len), int(crc_poly) & 0xffffffff), max_frames, (), device)
        self.list_size, self.crc_len, self.crc_poly = int(list_size), int(crc_len), int(crc_poly)

    def decode(self, llr, frozen=None, crc=None, want=LIST_OUTPUTS):
        """llr [F, N] int8 or float32 (the context's messages), frozen int32 / uint32 [F, W] or None (zeros), crc int32 / uint32 [F] the expected
        remainders or None (zeros) -> dict of device tensors, those `want` names: u, info, x int32 rows of the picked path as Polar.decode gives
        them, pick int32 [F], metric [F, L] int32 (the uint32's bits) or float32, list_x int32 [F, L, W]"""
        torch, F, pl, pf = self._decode_inputs(llr, frozen)
        L, pc = self.list_size, None
        if crc is not None:
            assert crc.is_cuda and crc.dtype in (torch.int32, torch.uint32) and crc.is_contiguous() and tuple(crc.shape) == (F,), "crc"
            pc = _vp(crc.data_ptr())
        out, ptr = self._outputs(llr.device, dict(u=((F, self.W), torch.int32), info=((F, self.Wi), torch.int32), x=((F, self.W), torch.int32),
                                                  pick=((F,), torch.int32), metric=((F, L), torch.int32 if self.messages == POLAR_I8 else torch.float32),
                                                  list_x=((F, L, self.W), torch.int32)), want)
        self._on_current_stream()
        _chk(_L.qldpc_polar_list_decode_dev(self._h, F, pl, pf, pc, ptr("u"), ptr("info"), ptr("x"), ptr("pick"), ptr("metric"), ptr("list_x")),
             "PolarList.decode")
        return out

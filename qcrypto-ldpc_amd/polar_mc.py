"""The Monte-Carlo FER loop around the polar decoders (qldpc_polar_mc_*): frames generated, sent through a threshold-table channel, decoded and
judged on the device around an existing Polar or PolarList, the host mirror of its frames, and the AWGN table builder in the two roundings of the
reference's scripts."""
import ctypes as C

import numpy as np

from ._lib import _L, _Handle, _chk, _create, _dp, _fp, _ip, _ptr, _sig, _torch, _u64p, _up, _vp, QldpcError
from .polar import POLAR_I8, PolarList, _messages, _words

POLAR_MC_FROZEN = {"zero": 0, "random": 1}
POLAR_MC_SOURCE = {"random": 0, "zero": 1}
POLAR_MC_ROUNDING = {"floor": 0, "round": 1}
POLAR_MC_COUNTERS = ("frames", "bit_errors", "frame_errors", "undetected", "crc_fails", "channel_flips", "channel_bits", "batches", "next_frame")
POLAR_MC_MS = ("source_ms", "encode_ms", "channel_ms", "decode_ms", "monitor_ms", "total_ms")
POLAR_MC_OUTPUTS = ("info", "u", "x", "llr", "flips")

_sig("qldpc_polar_mc_create", C.c_int, [_vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)])
_sig("qldpc_polar_mc_free", None, [_vp])
_sig("qldpc_polar_mc_device_bytes", C.c_size_t, [_vp])
_sig("qldpc_polar_mc_set_source", C.c_int, [_vp, C.c_int])
_sig("qldpc_polar_mc_set_channel", C.c_int, [_vp, C.c_int, _u64p, _u64p, _fp])
_sig("qldpc_polar_mc_frames_dev", C.c_int, [_vp, C.c_uint64, C.c_int, _vp, _vp, _vp, _vp, _vp])
_sig("qldpc_polar_mc_run", C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, _u64p, _dp])
_sig("qldpc_polar_mc_failed_frames", C.c_int, [_vp, _u64p, C.c_int])
_sig("qldpc_polar_mc_construct", C.c_int, [_vp, C.c_uint64, C.c_uint64, _u64p, _dp])
_sig("qldpc_polar_mc_awgn_table", C.c_int, [C.c_double, C.c_double, C.c_int, C.c_int, _u64p, _u64p, _fp])
_sig("qldpc_polar_mc_frames_host", C.c_int, [C.c_int, C.c_int, _ip, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_int, _u64p, _u64p, _fp,
                                            C.c_uint64, C.c_int, _up, _up, _up, _vp, _up])


def _mode(table, value, what):
    """a mode by its name; a number goes to the library as it is, which refuses what is none"""
    if isinstance(value, str):
        if value not in table:
            raise QldpcError(-1, "polar_mc: %s=%r (%s)" % (what, value, " or ".join(repr(k) for k in table)))
        return table[value]
    return int(value)


def _table(cum0, cum1, value):
    """(cum0, cum1, value) as the library takes them -> levels (what `value` holds) and the three arrays"""
    c0, c1 = (np.ascontiguousarray(a, dtype=np.uint64).ravel() for a in (cum0, cum1))
    v = np.ascontiguousarray(value, dtype=np.float32).ravel()
    if c0.size != max(v.size - 1, 0) or c1.size != c0.size:
        raise QldpcError(-6, "polar_mc: cum0 and cum1 hold levels - 1 entries, value levels")
    return v.size, c0, c1, v


def polar_mc_awgn_table(sigma, rmax=4.0, maxq=31, rounding="floor"):
    """the threshold table of BPSK over AWGN of deviation sigma, received values quantised as the reference's scripts do (qldpc_polar_mc_awgn_table):
    rounding="floor": floor(r / rmax maxq) clamped to [-maxq - 1, maxq], 2 maxq + 2 levels (the SC scripts, mc_awgn_table bit for bit);
    rounding="round": round(clip(r, -rmax, rmax) / rmax maxq), 2 maxq + 1 levels (the list script) -> (cum0, cum1, value)"""
    cap = 2 * max(int(maxq), 0) + 2
    c0, c1, v = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.float32)
    q = _chk(_L.qldpc_polar_mc_awgn_table(float(sigma), float(rmax), int(maxq), _mode(POLAR_MC_ROUNDING, rounding, "rounding"), c0.ctypes.data_as(_u64p),
                                          c1.ctypes.data_as(_u64p), v.ctypes.data_as(_fp)), "polar_mc_awgn_table")
    return c0[:q - 1].copy(), c1[:q - 1].copy(), v[:q].copy()


def polar_mc_frames_host(log2_n, info_pos, first, n, seed=0, table=None, messages="i8", crc_len=0, crc_poly=0, frozen="zero", source="random",
                         want=POLAR_MC_OUTPUTS):
    """the mirror of the loop's frames (qldpc_polar_mc_frames_host), no device: frames first .. first + n - 1 of the code (log2_n, info_pos) with the
    CRC (crc_len, crc_poly) through `table` = (cum0, cum1, value) or None (then neither llr nor flips)
    -> dict of those of info uint32 [n, ceil(K/32)], u, x uint32 [n, W], llr [n, N] int8 or float32, flips uint32 [n] that `want` names"""
    kind, dt = _messages(messages)
    pos = np.ascontiguousarray(info_pos, dtype=np.int32).ravel()
    nl, n, W = int(log2_n), int(n), _words(log2_n)
    N = (1 << nl) if 0 <= nl <= 20 else 1
    levels, c0, c1, v = _table(*table) if table is not None else (0, None, None, None)
    shapes = dict(info=((max(n, 0), (pos.size + 31) // 32), np.uint32), u=((max(n, 0), W), np.uint32), x=((max(n, 0), W), np.uint32),
                  llr=((max(n, 0), N), dt), flips=((max(n, 0),), np.uint32))
    out = {k: np.zeros(*shapes[k]) for k in POLAR_MC_OUTPUTS if k in want}
    _chk(_L.qldpc_polar_mc_frames_host(nl, pos.size, pos.ctypes.data_as(_ip), kind, int(crc_len), int(crc_poly) & 0xffffffff, _mode(POLAR_MC_FROZEN, frozen, "frozen"),
                                       _mode(POLAR_MC_SOURCE, source, "source"), int(seed) & 0xffffffffffffffff, levels, _ptr(c0, _u64p), _ptr(c1, _u64p),
                                       _ptr(v, _fp), int(first) & 0xffffffffffffffff, n, _ptr(out.get("info"), _up), _ptr(out.get("u"), _up),
                                       _ptr(out.get("x"), _up), _ptr(out.get("llr"), _vp), _ptr(out.get("flips"), _up)), "polar_mc_frames_host")
    return out


class PolarMonteCarlo(_Handle):
    """The device-resident Monte-Carlo loop around `decoder`, a Polar (either form) or a PolarList, which it does not own: frame i is a pure function
    of (seed, i, the code, the CRC, the frozen mode, the table).  frozen="zero": frozen positions are 0; "random": random frozen values that the
    decoder is told, the reconciliation form.  batch = 0: the decoder's max_frames.  Runs on torch's current stream."""
    _free = _L.qldpc_polar_mc_free

    def __init__(self, decoder, seed=0, batch=0, fail_cap=1024, frozen="zero", source="random"):
        is_list = isinstance(decoder, PolarList)
        self.decoder, self.seed, self.fail_cap = decoder, int(seed), int(fail_cap)
        self.frozen = _mode(POLAR_MC_FROZEN, frozen, "frozen")
        self._h = _create("PolarMonteCarlo", _L.qldpc_polar_mc_create, None if is_list else decoder._h, decoder._h if is_list else None,
                          self.seed & 0xffffffffffffffff, int(batch), self.fail_cap, self.frozen)
        self.batch = int(batch) or decoder.max_frames
        self.crc_len, self.crc_poly = (decoder.crc_len, decoder.crc_poly) if is_list else (0, 0)
        self.table = None
        if _mode(POLAR_MC_SOURCE, source, "source"):
            self.set_source(source)

    def device_bytes(self):
        return int(_L.qldpc_polar_mc_device_bytes(self._h))

    def set_source(self, source):
        _chk(_L.qldpc_polar_mc_set_source(self._h, _mode(POLAR_MC_SOURCE, source, "source")), "PolarMonteCarlo.set_source")

    def set_channel(self, cum0, cum1, value):
        """the threshold table every frame goes through from now on: cum0, cum1 uint64 [levels - 1], value float32 [levels]"""
        levels, c0, c1, v = _table(cum0, cum1, value)
        _chk(_L.qldpc_polar_mc_set_channel(self._h, levels, c0.ctypes.data_as(_u64p), c1.ctypes.data_as(_u64p), v.ctypes.data_as(_fp)), "PolarMonteCarlo.set_channel")
        self.table = (c0, c1, v)

    def set_awgn(self, ebno_db, rate, rmax=4.0, maxq=31, rounding="floor"):
        """BPSK over AWGN at Eb/N0 = ebno_db for a code of rate `rate`: sigma = sqrt(1 / (2 rate 10^(ebno_db / 10))), quantised as polar_mc_awgn_table does"""
        sigma = float(np.sqrt(1.0 / (2.0 * float(rate) * 10.0 ** (float(ebno_db) / 10.0))))
        self.set_channel(*polar_mc_awgn_table(sigma, rmax, maxq, rounding))
        return sigma

    def set_bsc(self, qber, mag):
        """a BSC of crossover qber: the 2-level table {+mag, -mag}"""
        t = int(np.floor(float(qber) * 4294967296.0))
        self.set_channel([(1 << 32) - t], [t], [float(mag), -float(mag)])

    def frames(self, first, n, want=POLAR_MC_OUTPUTS):
        """frames first .. first + n - 1 -> dict of device tensors, those `want` names: info int32 [n, ceil(K/32)], u, x int32 [n, W], llr [n, N] of the
        decoder's messages, flips int32 [n]"""
        torch, d, F = _torch(), self.decoder, max(int(n), 0)      # a negative n is the library's to refuse
        shapes = dict(info=((F, d.Wi), torch.int32), u=((F, d.W), torch.int32), x=((F, d.W), torch.int32),
                      llr=((F, d.N), torch.int8 if d.messages == POLAR_I8 else torch.float32), flips=((F,), torch.int32))
        out, ptr = d._outputs(d.device, shapes, want)
        d._on_current_stream()
        _chk(_L.qldpc_polar_mc_frames_dev(self._h, int(first) & 0xffffffffffffffff, int(n), ptr("info"), ptr("u"), ptr("x"), ptr("llr"), ptr("flips")),
             "PolarMonteCarlo.frames")
        return out

    def run(self, first_frame, max_frames, max_frame_errors=0):
        """batches from first_frame until max_frames are done or, at a batch boundary, max_frame_errors (0: never) are reached
        -> dict of the counters (POLAR_MC_COUNTERS) and the times in ms (POLAR_MC_MS)"""
        ctr, ms = np.zeros(16, np.uint64), np.zeros(8, np.float64)
        self.decoder._on_current_stream()
        _chk(_L.qldpc_polar_mc_run(self._h, int(first_frame) & 0xffffffffffffffff, int(max_frames), int(max_frame_errors), ctr.ctypes.data_as(_u64p),
                                   ms.ctypes.data_as(_dp)), "PolarMonteCarlo.run")
        out = {k: int(ctr[i]) for i, k in enumerate(POLAR_MC_COUNTERS)}
        out.update({k: float(ms[i]) for i, k in enumerate(POLAR_MC_MS)})
        return out

    def construct(self, first_frame, n_frames):
        """the genie-aided tally (qldpc_polar_mc_construct) of the object's own frames first_frame .. first_frame + n_frames - 1, batch by batch on
        the device with one read-back at the end: for polar_construct_order and polar_construct_k.  It needs a Polar of the lanes' form,
        frozen="random", the random source and a channel -> dict(wrong, ties uint64 [N], frames, and the times in ms (POLAR_MC_MS): the tally's
        in decode_ms, monitor_ms 0)"""
        tally, ms = np.zeros((2, self.decoder.N), np.uint64), np.zeros(8, np.float64)
        self.decoder._on_current_stream()
        _chk(_L.qldpc_polar_mc_construct(self._h, int(first_frame) & 0xffffffffffffffff, int(n_frames), tally.ctypes.data_as(_u64p), ms.ctypes.data_as(_dp)),
             "PolarMonteCarlo.construct")
        out = dict(wrong=tally[0].copy(), ties=tally[1].copy(), frames=int(n_frames))
        out.update({k: float(ms[i]) for i, k in enumerate(POLAR_MC_MS)})
        return out

    def failed_frames(self):
        """the first fail_cap failed global frame indices of the last run, ascending, uint64"""
        buf = np.zeros(max(self.fail_cap, 1), np.uint64)
        n = _chk(_L.qldpc_polar_mc_failed_frames(self._h, buf.ctypes.data_as(_u64p), self.fail_cap), "PolarMonteCarlo.failed_frames")
        return buf[:n].copy()

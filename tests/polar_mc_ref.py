"""numpy restatement of the frames of the Monte-Carlo loop around the polar decoders (include/qldpc.h, "a device-resident Monte-Carlo FER loop
(qldpc_polar_mc_*)"), shared by tests/test_polar_mc.py and tests/test_polar_mc_gpu.py, on unpacked bits.  frames() calls nothing of the library;
counters() is the yardstick of the loop's counters: the MIRROR's frames through the host decoders, judged in numpy.

    message    A = K - crc_len bits, word j = Philox output word j % 4 at counter (j / 4, 0, i_lo, i_hi), MSB first, or zeros
    info row   the message, then its CRC remainder MSB first
    u          u[info_pos[m]] = info bit m; frozen positions 0, or the bits of stream 4 (word w % 4 at counter (w / 4, 4, i_lo, i_hi))
    x          encode(u)
    channel    position v draws word v % 4 at counter (v / 4, 3, i_lo, i_hi); level = #{k : u >= cum[x_v][k]}; LLR = value[level]
    flips      positions with x_v = 0 and LLR < 0, or x_v = 1 and LLR > 0
"""
import numpy as np

import mc_ref
import mc_soft_ref
import polar_list_ref as LR
import polar_ref as R

COUNTERS = ("frames", "bit_errors", "frame_errors", "undetected", "crc_fails", "channel_flips", "channel_bits")
MC_SEED = 20261         # the seed of the published-curve tests, CPU and GPU


def _bits(seed, first, F, stream, count):
    """the first `count` bits of a stream of frames first .. first + F - 1, MSB first -> uint8 [F, count]"""
    if count == 0:
        return np.zeros((F, 0), np.uint8)
    return mc_ref.unpack(mc_ref._stream(seed, first, F, stream, (count + 31) // 32), count)


def frames(n, pos, seed, first, F, table=None, messages="i8", crc=(0, 0), frozen="zero", source="random"):
    """-> dict(info uint8 [F, K], u, x uint8 [F, N], and with a table llr [F, N] int8 or float32 and flips int64 [F])"""
    N, pos = 1 << n, np.asarray(pos, np.int64)
    K, (crc_len, crc_poly) = len(pos), crc
    A = K - crc_len
    msg = _bits(seed, first, F, 0, A) if source == "random" else np.zeros((F, A), np.uint8)
    info = np.concatenate([msg, LR.crc_word(LR.crc_bits(msg, crc_len, crc_poly), crc_len)], axis=1) if crc_len else msg
    u = np.zeros((F, N), np.uint8)
    if frozen == "random":
        mask = np.ones(N, bool)
        mask[pos] = False
        u[:, mask] = _bits(seed, first, F, 4, N)[:, mask]
    u[:, pos] = info
    x = R.encode(u)
    out = dict(info=info, u=u, x=x)
    if table is not None:
        llr, flip_words = mc_soft_ref.llr_frames(N, N, seed, table, first, F, cw_bits=x, vn_class=np.zeros(N, np.uint8))
        out["llr"] = llr.astype(np.int8) if messages == "i8" else llr
        out["flips"] = mc_ref.unpack(flip_words, N).sum(axis=1).astype(np.int64)
    return out


def check_frames(got, ref, what=""):
    """a frames dict of the library (host arrays, packed rows) against frames(): bit for bit, floats by their bit patterns; only the keys `got` has"""
    words = lambda a: np.asarray(a).view(np.uint32)
    for k in ("info", "u", "x"):
        if k in got:
            bits = ref[k]
            want = R.pack(bits) if bits.shape[1] else np.zeros((bits.shape[0], 0), np.uint32)
            assert np.array_equal(words(got[k]), want), what + ": " + k
    if "llr" in got:
        g = np.asarray(got["llr"])
        assert g.dtype == ref["llr"].dtype and g.shape == ref["llr"].shape, what + ": llr"
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, ref["llr"].view(np.uint32) if g.dtype == np.float32 else ref["llr"]), what + ": llr"
    if "flips" in got:
        assert np.array_equal(np.asarray(got["flips"]).astype(np.int64), ref["flips"]), what + ": flips"


def counters(q, n, pos, seed, first, F, table, messages="i8", maxq=31, L=None, crc=(0, 0), frozen="zero", source="random"):
    """the counters of a run of F frames from `first`, restated: the mirror's frames -> polar_decode_host (L None) or polar_list_decode_host ->
    the verdict in numpy -> (dict of COUNTERS, the failed global indices uint64, ascending)"""
    N, K = 1 << n, len(pos)
    A = K - crc[0]
    fr = q.polar_mc_frames_host(n, pos, first, F, seed, table, messages, crc[0], crc[1], frozen, source)
    fz = fr["u"] if frozen == "random" else None
    if L is None:
        info = q.polar_decode_host(n, pos, fr["llr"], fz, messages, maxq)["info"]
        pick = np.zeros(F, np.int32)
    else:
        got = q.polar_list_decode_host(n, pos, fr["llr"], fz, None, messages, maxq, L, crc[0], crc[1], want=("info", "pick"))
        info, pick = got["info"], got["pick"]
    be = (R.unpack(info, K)[:, :A] != R.unpack(fr["info"], K)[:, :A]).sum(axis=1)
    fe, crcf = be > 0, pick < 0
    c = dict(frames=F, bit_errors=int(be.sum()), frame_errors=int(fe.sum()), undetected=int((fe & ~crcf).sum()), crc_fails=int(crcf.sum()),
             channel_flips=int(fr["flips"].astype(np.int64).sum()), channel_bits=F * N)
    return c, (np.uint64(first) + np.nonzero(fe)[0].astype(np.uint64))


def add(a, b):
    return {k: a[k] + b[k] for k in COUNTERS}


# ---- the published curves through the loop: the table and the code of every point ---------------------------------------------------------

def sc_point(q, k):
    """point k of the published SC curve -> (row, info_pos, table, frames): K = 512 in the 5G order, 6-bit values by floor"""
    pub = R.published()
    N, K = pub["N"], pub["K"]
    row = pub["res2"][k]
    sigma = np.sqrt(1.0 / (2.0 * (K / N) * 10.0 ** (row[0] / 10.0)))
    return row, R.nr_order(N)[N - K:], q.polar_mc_awgn_table(sigma, pub["rmax"], pub["maxqr"], "floor"), R.FER_FRAMES[k]


def list_point(q, k):
    """point k of the published list-4 curve -> (row, info_pos, table, frames): A = 500 and CRC 11 at the 511 best positions, 6-bit values by round"""
    pub = R.published()
    N, res3 = pub["N"], pub["res3"]
    A, row = res3["A"], res3["rows"][k]
    sigma = np.sqrt(1.0 / (2.0 * (A / N) * 10.0 ** (row[0] / 10.0)))
    return row, R.nr_order(N)[N - (A + res3["crcL"]):], q.polar_mc_awgn_table(sigma, res3["rmax"], pub["maxqr"], "round"), LR.LIST_FRAMES[k]

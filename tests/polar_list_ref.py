"""The restatement the list-decoder tests hold the library to: the CRC-aided successive-cancellation list decoder written from its definition
(qldpc_polar_list_core.h's header) in numpy, vectorised over frames, with WHOLE-STATE copies on a fork and a stable argsort on
(metric, candidate index); int64 beliefs and metrics for the int8 messages, np.float32 for the float ones.  Also the CRC by its bitwise
definition and the frames of the published list-4 curve."""
import numpy as np

import polar_ref as R

CRC11 = (11, 0x621)


# ---- the CRC: register form, zero start, MSB first, no reflection, no final XOR ------------------------------------------------------------

def crc_bits(bits, crc_len, crc_poly):
    """bits uint8 [F, n] -> the remainders uint32 [F]"""
    bits = np.asarray(bits, np.uint8)
    r = np.zeros(bits.shape[0], np.uint64)
    if crc_len == 0:
        return r.astype(np.uint32)
    mask = np.uint64((1 << crc_len) - 1)
    for m in range(bits.shape[1]):
        top = ((r >> np.uint64(crc_len - 1)) & np.uint64(1)) ^ bits[:, m].astype(np.uint64)
        r = ((r << np.uint64(1)) & mask) ^ (top * np.uint64(crc_poly))
    return r.astype(np.uint32)


def crc_word(r, crc_len):
    """the remainders as crc_len bits, MSB first: what is appended to a message"""
    r = np.asarray(r, np.uint64)
    return np.stack([((r >> np.uint64(crc_len - 1 - b)) & np.uint64(1)).astype(np.uint8) for b in range(crc_len)], axis=1).reshape(len(r), crc_len)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------

def decode(llr, frozen_mask, frozen_values=None, messages="i8", maxq=31, L=4, info_pos=(), crc_len=0, crc_poly=0, crc=None):
    """llr [F, N]; frozen_mask bool [N]; frozen_values uint8 [F, N] or None; crc uint32 [F] or None -> dict(list_x uint8 [F, L, N], metric [F, L]
    (uint32 / float32, all ones / inf past the live paths), pick int32 [F], u, x uint8 [F, N] and info uint8 [F, K] of the picked path, P)"""
    i8 = messages == "i8"
    if i8:
        L0 = np.clip(np.asarray(llr).astype(np.int64), -(maxq + 1), maxq)
        sat = lambda v: np.clip(v, -(maxq + 1), maxq)
        metric = np.zeros((L0.shape[0], 1), np.int64)
    else:
        L0 = np.asarray(llr, np.float32)
        sat = lambda v: v
        metric = np.zeros((L0.shape[0], 1), np.float32)
    F, N = L0.shape
    n = N.bit_length() - 1
    one = L0.dtype.type(1)
    rows = np.arange(F)[:, None]
    # a path's whole state: beliefs B[l] [F, P, 2^l] of the node at work on every level, re-encoded bits x [F, P, N] of every finished node in place
    B = [np.zeros((F, 1, 1 << l), L0.dtype) for l in range(n)] + [L0[:, None, :].copy()]
    x = np.zeros((F, 1, N), np.uint8)

    def sgn(v):
        return np.where(v < 0, -one, one)

    for i in range(N):
        top = n - 1 if i == 0 else (i & -i).bit_length() - 1
        for l in range(top, -1, -1):
            h = 1 << l
            a, b = B[l + 1][:, :, :h], B[l + 1][:, :, h:]
            if i != 0 and l == top:
                c = x[:, :, i - h:i].astype(L0.dtype)
                B[l] = sat(b + (one - 2 * c) * a).astype(L0.dtype)
            else:
                B[l] = (sgn(a) * sgn(b) * np.minimum(np.abs(a), np.abs(b))).astype(L0.dtype)
        D = B[0][:, :, 0]
        P = D.shape[1]
        neg = (D < 0).astype(np.uint8)
        if frozen_mask[i]:
            bit = frozen_values[:, i:i + 1] if frozen_values is not None else np.zeros((F, 1), np.uint8)
            metric = metric + np.where(neg != bit, np.abs(D), 0).astype(metric.dtype)
            x[:, :, i] = bit
        else:
            cand = np.concatenate([metric, (metric + np.abs(D)).astype(metric.dtype)], axis=1)         # [F, 2P]: KEEP 0 .. P - 1, FLIP 0 .. P - 1
            keep = np.argsort(cand, axis=1, kind="stable")[:, :min(L, 2 * P)]
            parent = keep % P
            metric = cand[rows, keep]
            B = [v[rows, parent] for v in B]
            x = x[rows, parent]
            x[:, :, i] = neg[rows, parent] ^ (keep >= P).astype(np.uint8)
        h = 1
        while i & h:                                                   # every node that ends with leaf i, smallest first
            x[:, :, i + 1 - 2 * h:i + 1 - h] ^= x[:, :, i + 1 - h:i + 1]
            h *= 2
    P = x.shape[1]
    pos = np.asarray(info_pos, np.int64)
    u_all = np.stack([R.encode(x[:, k]) for k in range(P)], axis=1)    # the involution: u = encode(x)
    want = np.zeros(F, np.uint32) if crc is None else np.asarray(crc, np.uint32)
    match = np.stack([crc_bits(u_all[:, k][:, pos], crc_len, crc_poly) == want for k in range(P)], axis=1)
    pick = np.where(match.any(axis=1), match.argmax(axis=1), -1).astype(np.int32)
    chosen = np.maximum(pick, 0)
    list_x = np.zeros((F, L, N), np.uint8)
    list_x[:, :P] = x
    if i8:
        m_out = np.full((F, L), 0xffffffff, np.uint32)
        m_out[:, :P] = metric.astype(np.uint32)
    else:
        m_out = np.full((F, L), np.inf, np.float32)
        m_out[:, :P] = metric
    u = u_all[np.arange(F), chosen]
    return dict(list_x=list_x, metric=m_out, pick=pick, u=u, x=x[np.arange(F), chosen], info=u[:, pos], P=P)


def check_outputs(out, ref, what=""):
    """a list decode's dict (host arrays) against the restatement's, bit for bit (floats by their bit patterns); only the keys `out` has"""
    F, L, N = ref["list_x"].shape
    bits = lambda a: np.asarray(a).view(np.uint32)
    if "list_x" in out:
        assert np.array_equal(bits(out["list_x"]), R.pack(ref["list_x"].reshape(F * L, N)).reshape(F, L, -1)), what + ": list_x"
    if "metric" in out:
        assert np.array_equal(bits(out["metric"]), ref["metric"].view(np.uint32)), what + ": metric"
    if "pick" in out:
        assert np.array_equal(np.asarray(out["pick"]), ref["pick"]), what + ": pick"
    if "u" in out:
        assert np.array_equal(bits(out["u"]), R.pack(ref["u"])), what + ": u"
    if "x" in out:
        assert np.array_equal(bits(out["x"]), R.pack(ref["x"])), what + ": x"
    if "info" in out:
        K = ref["info"].shape[1]
        assert np.array_equal(bits(out["info"]), R.pack(ref["info"]) if K else np.zeros((F, 0), np.uint32)), what + ": info"


# ---- the frames of the published list-4 curve ----------------------------------------------------------------------------------------------

LIST_FRAMES = (1000, 1000, 3000, 20000)      # frames here at the four res3 points
LIST_SEED = 4711


def list_point(k, F=None):
    """point k of the published list-4 curve as the script forms it: A = 500 random message bits, their CRC 11 appended MSB first, the 511 bits
    at the 511 most reliable positions of the 5G order, BPSK over AWGN with sigma from rate 500 / 1024, received values rounded to 6 bits
    -> (published row, info_pos, msg uint8 [F, 500], rq int8 [F, N])"""
    pub = R.published()
    N, res3 = pub["N"], pub["res3"]
    A, crc_len, rmax, maxqr = res3["A"], res3["crcL"], res3["rmax"], pub["maxqr"]
    row = res3["rows"][k]
    pos = R.nr_order(N)[N - (A + crc_len):]
    rng = np.random.default_rng([LIST_SEED, k])
    F = LIST_FRAMES[k] if F is None else F
    msg = rng.integers(0, 2, (F, A)).astype(np.uint8)
    word = np.concatenate([msg, crc_word(crc_bits(msg, *CRC11), crc_len)], axis=1)
    u = np.zeros((F, N), np.uint8)
    u[:, pos] = word
    sigma = np.sqrt(1.0 / (2.0 * (A / N) * 10.0 ** (row[0] / 10.0)))
    r = (1.0 - 2.0 * R.encode(u)) + sigma * rng.standard_normal((F, N))
    rq = np.round(np.clip(r, -rmax, rmax) / rmax * maxqr).astype(np.int8)
    return row, pos, msg, rq


def recon_frames(F=2000, qber=0.06):
    """the reconciliation form as R.recon_frames builds it (N = 1024, K = 512 in the 5G order, Alice's key x, her frozen values encode(x), Bob's
    float LLRs of x through a BSC), at the QBER where SC starts to fail -> (info_pos, x uint8 [F, N], frozen uint32 [F, 32], llr float32 [F, N])"""
    N, K = 1024, 512
    pos = R.nr_order(N)[N - K:]
    rng = np.random.default_rng([77, 60])
    x = rng.integers(0, 2, (F, N), dtype=np.uint8)
    y = x ^ (rng.random((F, N)) < qber).astype(np.uint8)
    mag = np.float32(np.log((1.0 - qber) / qber))
    llr = ((1.0 - 2.0 * y) * mag).astype(np.float32)
    return pos, x, R.pack(R.encode(x)), llr

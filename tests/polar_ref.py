"""The restatement the polar tests hold the library to: the encoder and the successive-cancellation decoder written from their definition (DESIGN
section 3.3, qldpc_polar_core.h's header) in numpy, vectorised over frames, int64 for the int8 messages and np.float32 for the float ones, on
unpacked bits.  Also what the tests share: packing, the 5G reliability order, the frames of the published curve and of the reconciliation form."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- packed rows (MSB-first uint32 words) <-> bits [F, N] ---------------------------------------------------------------------------------

def pack(bits):
    bits = np.asarray(bits, np.uint8)
    F, N = bits.shape
    pad = (-N) % 32
    if pad:
        bits = np.concatenate([bits, np.zeros((F, pad), np.uint8)], axis=1)
    return np.ascontiguousarray(np.packbits(np.ascontiguousarray(bits), axis=1, bitorder="big")).view(">u4").astype(np.uint32)


def unpack(words, N):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    return np.unpackbits(words.astype(">u4").view(np.uint8), axis=1, bitorder="big")[:, :N]


# ---- the definition ----------------------------------------------------------------------------------------------------------------------

def encode(u):
    """u uint8 [F, N] -> x: for m = 1, 2, .., N/2, in every block of 2m bits the first half becomes first ^ second"""
    x = np.array(u, np.uint8)
    F, N = x.shape
    m = 1
    while m < N:
        v = x.reshape(F, N // (2 * m), 2, m)
        v[:, :, 0, :] ^= v[:, :, 1, :]
        m *= 2
    return x


def kron_matrix(n):
    """F^{(x) n}, F = [[1, 0], [1, 1]]: x = u G over GF(2)"""
    G = np.array([[1]], np.uint8)
    for _ in range(n):
        G = np.kron(G, np.array([[1, 0], [1, 1]], np.uint8))
    return G


def decode(llr, frozen_mask, frozen_values=None, messages="i8", maxq=31):
    """llr [F, N]; frozen_mask bool [N]; frozen_values uint8 [F, N] or None -> (u, x, leaf): decisions uint8 [F, N], the root's re-encoded word
    uint8 [F, N], leaf beliefs [F, N] (int64 or float32)"""
    i8 = messages == "i8"
    if i8:
        L0 = np.clip(np.asarray(llr).astype(np.int64), -(maxq + 1), maxq)
        sat = lambda v: np.clip(v, -(maxq + 1), maxq)
    else:
        L0 = np.asarray(llr, np.float32)
        sat = lambda v: v
    F, N = L0.shape
    u = np.zeros((F, N), np.uint8)
    leaf = np.zeros((F, N), L0.dtype)
    one = L0.dtype.type(1)

    def sgn(v):
        return np.where(v < 0, -one, one)

    def node(L, lo):
        s = L.shape[1]
        if s == 1:
            leaf[:, lo] = L[:, 0]
            if frozen_mask[lo]:
                bit = frozen_values[:, lo] if frozen_values is not None else np.zeros(F, np.uint8)
            else:
                bit = (L[:, 0] < 0).astype(np.uint8)
            u[:, lo] = bit
            return bit.reshape(F, 1).astype(np.uint8)
        a, b = L[:, :s // 2], L[:, s // 2:]
        cl = node(sgn(a) * sgn(b) * np.minimum(np.abs(a), np.abs(b)), lo)
        cr = node(sat(b + (one - 2 * cl.astype(L.dtype)) * a), lo + s // 2)
        return np.concatenate([cl ^ cr, cr], axis=1)

    x = node(L0, 0)
    return u, x, leaf


# ---- what the tests share ----------------------------------------------------------------------------------------------------------------

def nr_order(N):
    """the 5G reliability order for N <= 1024 (tests/golden/nr_polar_reliability.json): ascending reliability, entries below N"""
    q = np.array(json.load(open(os.path.join(GOLD, "nr_polar_reliability.json")))["sequence"], np.int32)
    return q[q < N]


def published():
    return json.load(open(os.path.join(GOLD, "matlab_polar_fer.json")))


FER_FRAMES = (2000, 4000, 10000, 10000, 20000)      # frames here at the five res2 points
FER_SEED = 38212


def fer_point(k):
    """point k of the published SC curve as the script forms it: random messages, BPSK over AWGN with sigma from rate K/N, 6-bit received values
    -> (published row, info_pos, msg uint8 [F, K], rq int8 [F, N])"""
    pub = published()
    N, K, rmax, maxqr = pub["N"], pub["K"], pub["rmax"], pub["maxqr"]
    row = pub["res2"][k]
    pos = nr_order(N)[N - K:]
    rng = np.random.default_rng([FER_SEED, k])
    F = FER_FRAMES[k]
    msg = rng.integers(0, 2, (F, K), dtype=np.uint8)
    u = np.zeros((F, N), np.uint8)
    u[:, pos] = msg
    sigma = np.sqrt(1.0 / (2.0 * (K / N) * 10.0 ** (row[0] / 10.0)))
    r = (1.0 - 2.0 * encode(u)) + sigma * rng.standard_normal((F, N))
    rq = np.clip(np.floor(r / rmax * maxqr), -(maxqr + 1), maxqr).astype(np.int8)
    return row, pos, msg, rq


def fer_band(row, F):
    """the half width of the band around the published FER f: 4 sqrt(f (1 - f) / F + f (1 - f) / F_pub)"""
    f, F_pub = row[1], row[5]
    return 4.0 * np.sqrt(f * (1.0 - f) / F + f * (1.0 - f) / F_pub)


def info_bits(info_words, K):
    return unpack(info_words, K)


def recon_frames(seed, F=2000, qber=0.02):
    """the reconciliation form at N = 1024, K = 512 in the 5G order: Alice's key x, her frozen values encode(x) (packed rows), Bob's float LLRs of
    x through a BSC -> (info_pos, x uint8 [F, N], frozen uint32 [F, 32], llr float32 [F, N])"""
    N, K = 1024, 512
    pos = nr_order(N)[N - K:]
    rng = np.random.default_rng([seed, 7])
    x = rng.integers(0, 2, (F, N), dtype=np.uint8)
    y = x ^ (rng.random((F, N)) < qber).astype(np.uint8)
    mag = np.float32(np.log((1.0 - qber) / qber))
    llr = ((1.0 - 2.0 * y) * mag).astype(np.float32)
    return pos, x, pack(encode(x)), llr


def i8_inputs(rng, F, N, maxq):
    """int8 levels over the full range (the load clamps them); frame 0 all -(maxq + 1), so that f yields maxq + 1, and frame 1 all 0"""
    llr = rng.integers(-128, 128, (F, N)).astype(np.int8)
    llr[0] = -(maxq + 1)
    if F > 1:
        llr[1] = 0
    return llr


def f32_inputs(rng, F, N):
    """float LLRs, the kind by frame index mod 5: normal; BSC +-|LLR| (massive ties, exact cancellations); +-0.0; denormals; magnitudes up to 1e30"""
    sign = np.where(rng.random((F, N)) < 0.5, -1.0, 1.0)
    kinds = [rng.standard_normal((F, N)) * 4.0,
             np.where(rng.random((F, N)) < 0.05, -1.0, 1.0) * np.log(0.95 / 0.05),
             sign * 0.0,
             sign * rng.integers(1, 1 << 20, (F, N)) * 1.401298464324817e-45,
             sign * 10.0 ** rng.uniform(-30.0, 30.0, (F, N))]
    llr = np.empty((F, N), np.float32)
    for f in range(F):
        llr[f] = kinds[f % 5][f].astype(np.float32)
    return llr


def random_code(rng, N, K=None):
    """info_pos (K of them, in a random order) and the frozen mask bool [N]"""
    K = int(rng.integers(0, N + 1)) if K is None else K
    pos = rng.permutation(N)[:K].astype(np.int32)
    mask = np.ones(N, bool)
    mask[pos] = False
    return pos, mask


def check_outputs(out, ref, pos, N, frozen_mask, what=""):
    """a decode's dict against the restatement's (u, x, leaf), bit for bit (floats by their bit patterns); only the keys `out` has"""
    u, x, leaf = ref
    if "u" in out:
        assert np.array_equal(np.asarray(out["u"]).view(np.uint32), pack(u)), what + ": u"
    if "x" in out:
        assert np.array_equal(np.asarray(out["x"]).view(np.uint32), pack(x)), what + ": x"
    if "info" in out:
        assert np.array_equal(np.asarray(out["info"]).view(np.uint32), pack(u[:, pos]) if len(pos) else np.zeros((u.shape[0], 0), np.uint32)), what + ": info"
    if "leaf" in out:
        got = np.asarray(out["leaf"])
        if got.dtype == np.float32:
            assert np.array_equal(got.view(np.uint32), leaf.astype(np.float32).view(np.uint32)), what + ": leaf"
        else:
            assert np.array_equal(got.astype(np.int64), leaf), what + ": leaf"

"""Blind reconciliation restated in numpy (test infrastructure): the weakest-VN select as a lexsort over (key, v), and the round loop
over the CPU oracle.  Nothing here calls the library under test."""
import numpy as np

PIN = np.float32(23.025850929840455)      # QLDPC_CONFIRMED_BIT_LLR


def pack_row(bits):
    """0/1 per VN -> uint32 words, MSB-first"""
    b = np.asarray(bits, np.uint8)
    pad = (-b.size) % 32
    by = np.packbits(np.concatenate([b, np.zeros(pad, np.uint8)]), bitorder="big")
    return by.reshape(-1, 4).astype(np.uint32) @ np.array([1 << 24, 1 << 16, 1 << 8, 1], np.uint32)


def unpack_row(words, n):
    w = np.asarray(words).astype(np.uint32).ravel()
    by = np.stack([(w >> 24) & 255, (w >> 16) & 255, (w >> 8) & 255, w & 255], axis=-1).astype(np.uint8)
    return np.unpackbits(by.ravel(), bitorder="big")[:n]


def weakest_vns(post, d, cand=None):
    """the min(d, candidates) candidates that come first in ascending (key, v) order, key = bits(|post|) as uint32; ascending VN indices"""
    post = np.ascontiguousarray(post, np.float32)
    key = post.view(np.uint32) & np.uint32(0x7fffffff)
    v = np.arange(post.size) if cand is None else np.flatnonzero(np.asarray(cand))
    order = np.lexsort((v, key[v]))               # last key is the primary one
    return np.sort(v[order[:max(0, min(int(d), v.size))]])


def weakest(post, d, cand=None):
    """the same as a packed row"""
    bits = np.zeros(np.asarray(post).size, np.uint8)
    bits[weakest_vns(post, d, cand)] = 1
    return pack_row(bits)


def weakest_rows(post, d, cand=None, take=None):
    """rows of a batch post[F, N]; cand[F, N] 0/1 or None; take[F] or None: rows of frames not taken are zero"""
    F, N = post.shape
    out = np.zeros((F, (N + 31) // 32), np.uint32)
    for f in range(F):
        if take is None or take[f]:
            out[f] = weakest(post[f], d, None if cand is None else cand[f])
    return out


def layered_graph(O, code, og):
    """the oracle's graph with the checks in the code's layer order (what the horizontal-layered decoder visits), and that order"""
    order, _, _ = code.layer_order()
    var, chk = og.edges()
    inv = np.empty(code.M, np.int32)
    inv[order] = np.arange(code.M, dtype=np.int32)
    newc = inv[chk]
    idx = np.argsort(newc, kind="stable")
    return O.Graph.from_edges(code.N, code.M, var[idx], newc[idx]), order


def pinned(llr, known, value):
    """llr[F, N] with +-PIN written where known[F, N] is set, by value[F, N]"""
    out = np.array(llr, np.float32, copy=True)
    k = np.asarray(known).astype(bool)
    out[k] = np.where(np.asarray(value)[k] != 0, -PIN, PIN)
    return out


def loop(decode, llr, alice, d, max_rounds, key_bits=None):
    """The round loop: decode(llr[F', N], live[F']) -> dict(post, hard, synd_ok) runs the oracle on the frames still open (live = their indices).  Per round: the frames that fail
    ask for their d weakest positions below key_bits that are not known yet, and get Alice's bits there.
    Returns (asks, done_round, hard): asks[r][F, N] 0/1 = what every frame asked for after round r (zero rows for frames that were not decoded
    or succeeded), done_round[F] = the round (0-based) in which the frame succeeded or -1, hard[F, N] = its decision then."""
    F, N = llr.shape
    key_bits = N if key_bits is None else key_bits
    known = np.zeros((F, N), np.uint8)
    done = np.full(F, -1, np.int32)
    hard = np.zeros((F, N), np.int32)
    asks = []
    for r in range(max_rounds):
        live = np.flatnonzero(done < 0)
        if live.size == 0:
            break
        res = decode(pinned(llr[live], known[live], alice[live]), live)
        ask = np.zeros((F, N), np.uint8)
        for i, f in enumerate(live):
            if res["synd_ok"][i]:
                done[f] = r
                hard[f] = res["hard"][i]
                continue
            cand = np.zeros(N, np.uint8)
            cand[:key_bits] = 1
            cand[known[f] != 0] = 0
            ask[f, weakest_vns(res["post"][i], d, cand)] = 1
        known |= ask
        asks.append(ask)
    return asks, done, hard

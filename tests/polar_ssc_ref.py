"""The restatement the SSC tests hold the library to: the simplified successive-cancellation decoder written from its definition (DESIGN section
3.3, qldpc_polar_ssc_core.h's header) in numpy -- recursive, vectorised over frames, int64 for the int8 messages and np.float32 for the float
ones, on unpacked bits, as polar_ref.decode -- the plan restated from the frozen mask, and the two families of codes the SSC tests draw."""
import numpy as np

import polar_ref as R

RATE0, RATE1, MIXED = 0, 1, 2


def decode(llr, frozen_mask, frozen_values=None, messages="i8", maxq=31):
    """llr [F, N]; frozen_mask bool [N]; frozen_values uint8 [F, N] or None -> (u, x, flag): decisions uint8 [F, N], the root's returned word
    uint8 [F, N], flag bool [F]: a belief of a rate-1 node of the frame is 0 (where SSC and SC may part)"""
    i8 = messages == "i8"
    if i8:
        L0 = np.clip(np.asarray(llr).astype(np.int64), -(maxq + 1), maxq)
        sat = lambda v: np.clip(v, -(maxq + 1), maxq)
    else:
        L0 = np.asarray(llr, np.float32)
        sat = lambda v: v
    frozen_mask = np.asarray(frozen_mask, bool)
    F, N = L0.shape
    u = np.zeros((F, N), np.uint8)
    flag = np.zeros(F, bool)
    one = L0.dtype.type(1)

    def sgn(v):
        return np.where(v < 0, -one, one)

    def node(L, lo):
        s = L.shape[1]
        fm = frozen_mask[lo:lo + s]
        if fm.all():                                               # rate 0: the beliefs are not looked at
            v = frozen_values[:, lo:lo + s] if frozen_values is not None else np.zeros((F, s), np.uint8)
            u[:, lo:lo + s] = v
            return R.encode(v)
        if not fm.any():                                           # rate 1: the signs, and their encoding as the decisions
            c = (L < 0).astype(np.uint8)
            flag[:] |= (L == 0).any(axis=1)
            u[:, lo:lo + s] = R.encode(c)
            return c
        a, b = L[:, :s // 2], L[:, s // 2:]
        cl = node(sgn(a) * sgn(b) * np.minimum(np.abs(a), np.abs(b)), lo)
        cr = node(sat(b + (one - 2 * cl.astype(L.dtype)) * a), lo + s // 2)
        return np.concatenate([cl ^ cr, cr], axis=1)

    x = node(L0, 0)
    return u, x, flag


def plan(frozen_mask):
    """the steps of a code in leaf order, int32 [steps, 3] = (first 32-leaf block, log2 of the leaves, kind): the maximal rate-0 / rate-1 nodes
    of 32 leaves or more, and every other 32-leaf block as MIXED; N < 32: one MIXED step of the whole frame"""
    frozen_mask = np.asarray(frozen_mask, bool)
    N = len(frozen_mask)
    if N < 32:
        return np.array([[0, N.bit_length() - 1, MIXED]], np.int32)
    steps = []

    def node(lo, s):
        fm = frozen_mask[lo:lo + s]
        if fm.all() or not fm.any():
            steps.append((lo // 32, s.bit_length() - 1, RATE0 if fm.all() else RATE1))
        elif s == 32:
            steps.append((lo // 32, 5, MIXED))
        else:
            node(lo, s // 2)
            node(lo + s // 2, s // 2)

    node(0, N)
    return np.array(steps, np.int32)


def plan_stats(n, steps):
    """what a plan keeps of the SC traversal: the steps by kind, the f/g element steps it issues and the leaf blocks it decodes as MIXED, beside
    SC's N log2 N element steps and N / 32 blocks (n > 5).  A step at block j whose node sits at level lam descends from top(j) to lam (rate 1,
    mixed: the last 5 levels of a mixed block are the in-block recursion, counted in full) or to lam + 1 (rate 0)"""
    N, kinds, fg = 1 << n, [0, 0, 0], 0
    for j, lam, kind in np.asarray(steps).tolist():
        kinds[kind] += 1
        top = n - 1 if j == 0 else ((j & -j).bit_length() - 1) + 5
        for l in range(top, (lam + 1 if kind == RATE0 else lam) - 1, -1):
            fg += 1 << l
        if kind == MIXED:
            fg += 5 * 32
    return dict(rate0=kinds[0], rate1=kinds[1], mixed=kinds[2], fg_steps=fg, fg_steps_sc=N * n, fg_share=fg / (N * n),
                blocks=kinds[2], blocks_sc=max(N // 32, 1), block_share=kinds[2] / max(N // 32, 1))


def mask_of(pos, N):
    mask = np.ones(N, bool)
    mask[np.asarray(pos, np.int64)] = False
    return mask


def no_pair_code(rng, n):
    """information only on even positions, so no rate-1 node has two leaves or more and SSC is SC on every input; one aligned quarter of the
    frame (a half at N = 2) is wholly frozen -> (info_pos in a random order, frozen mask)"""
    N = 1 << n
    info = np.zeros(N, bool)
    info[0::2] = rng.random(N // 2) < 0.6
    q = max(N // 4, 1)
    lo = int(rng.integers(0, N // q)) * q
    info[lo:lo + q] = False
    pos = rng.permutation(np.flatnonzero(info)).astype(np.int32)
    return pos, ~info


def clustered_code(rng, n):
    """a random dyadic partition of the frame: the root always splits, a node splits again with probability 0.75, and an unsplit node is all
    frozen, all information or random: rate-0 and rate-1 nodes of many sizes, as left and as right children -> (info_pos, frozen mask)"""
    N = 1 << n
    info = np.zeros(N, bool)

    def node(lo, s, root):
        if s > 1 and (root or rng.random() < 0.75):
            node(lo, s // 2, False)
            node(lo + s // 2, s // 2, False)
            return
        kind = int(rng.integers(0, 3))
        info[lo:lo + s] = False if kind == 0 else (True if kind == 1 else rng.random(s) < 0.5)

    node(0, N, True)
    pos = rng.permutation(np.flatnonzero(info)).astype(np.int32)
    return pos, ~info


def check_outputs(out, ref, pos, what=""):
    """a decode's dict against the restatement's (u, x, flag), bit for bit; only the keys `out` has"""
    u, x, _ = ref
    if "u" in out:
        assert np.array_equal(np.asarray(out["u"]).view(np.uint32), R.pack(u)), what + ": u"
    if "x" in out:
        assert np.array_equal(np.asarray(out["x"]).view(np.uint32), R.pack(x)), what + ": x"
    if "info" in out:
        assert np.array_equal(np.asarray(out["info"]).view(np.uint32), R.pack(u[:, pos]) if len(pos) else np.zeros((u.shape[0], 0), np.uint32)), what + ": info"

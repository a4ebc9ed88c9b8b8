"""Exact restatement of the variable-node update, the graphs that isolate one VN update, and their input families.

Plain numpy, float32 operation for operation, no device.  TEST INFRASTRUCTURE ONLY.

The contract (Decoder_LDPC_BP_flooding::_initialize_var_to_chk / _compute_post, restated by oracle/qldpc_oracle.c):

    sum = 0; sum += m[slot] in slot order;  tmp = Y + sum;  v2c[slot] = tmp - m[slot]

stars(degrees, counts): disjoint stars, each one centre VN of degree d, d checks of degree 2 and d leaf VNs of degree 1.  A degree-2 check of
the min-sum family hands each edge the other edge's input: unchanged under MS and AMS_MIN, through through() under OMS and NMS.  So with
m_k = (Y_leaf_k + 0) - 0 and T = through:

    flooding, n_ite = 1   post[centre] = fl(Y_c + (((0 + T(m_0)) + T(m_1)) + ...))            the POST body, degree d
                          post[leaf_k] = fl(Y_leaf_k + (0 + T((Y_c + 0) - 0)))
    flooding, n_ite = 2   post[leaf_k] = fl(Y_leaf_k + (0 + T(fl(tmp_c - T(m_k)))))           every extrinsic output of the NORMAL body, slot by slot
                          post[centre] = fl(Y_c + sum_k T(fl(fl(Y_leaf_k + (0 + L)) - L)))     L = T((Y_c + 0) - 0)
    hlayered, 1 sweep     per check of the star in sweep order, p the centre's running posterior:
                          new p = fl(fl(p - 0) + T(fl(Y_leaf - 0))),  post[leaf] = fl(fl(Y_leaf - 0) + T(fl(p - 0)))

Slot order is the code's own: the inverse of the exported `transpose` (CN-major edge -> VN-major slot).  Checks and VNs carry shuffled ids, so
slot order (ascending check id) is not construction order.

fan(info_degrees, M): an IRA code -- information VNs of the given degrees on the least-loaded checks, accumulator VN K + c on checks c and c + 1 --
for the posterior form of the flooding run.  Its reference is flood(), a plain flooding min-sum decoder over any exported graph with the check
update of tests/vlayered_ref.py; flood(order=...) also states the mutants the inputs are held sensitive to (tests/test_vn_rules_host.py):
"rev" (slots summed last to first), "yfirst" (Y first, then the slots), "drop_last" (the last slot left out), "pad" (the message of slot
vn_ptr[v + 1], the next VN's first, folded in).
"""
import numpy as np

import vlayered_ref

F32 = np.float32
MS_RULES = [("MS", 0.0), ("OMS", 0.35), ("NMS", 0.75), ("AMS_MIN", 0.0)]
F_FRAMES = 130      # two full 64-frame groups and a ragged one
PINNED = 23.02585
BSC_MAG = 2.6
I8_SCALE = 8.0
I8_SAT = 127.0 / I8_SCALE

# degree -> stars.  Set A: both bucket edges of VN_CAPS = {4, 12} (4 | 5, 12 | 13), the generic body, 64 | 65.  The counts leave a tail in every VN
# list (tests/test_vn_rules_host.py asserts it against UN and QK_WAVES of qldpc_launch.hip).
SET_A = {1: 3, 2: 3, 3: 3, 4: 3, 5: 3, 8: 3, 11: 3, 12: 2, 13: 3, 16: 2, 33: 2, 64: 2, 65: 2}
# The edge engine stages 512 VNs x max_dv messages in 64 KiB of LDS: VN degree <= 32 (its refusal said 64 until these tests ran a degree of 33 and
# of 64).  Its set: the degrees of set A up to that limit, the limit itself, and 33 alone as the first excess
EDGE_MAX_DV = 32
SET_EDGE = dict([(d, n) for d, n in SET_A.items() if d <= EDGE_MAX_DV] + [(EDGE_MAX_DV, 2)])
SET_33 = {EDGE_MAX_DV + 1: 1}
SET_256 = {256: 1}
SET_257 = {257: 1}
# the fan: information-VN degree -> count: degrees 0 .. 12 are 13 classes of qk_vn_fpost (four launches), every class with a tail; degrees 13 and 16 go to the cap-0 bucket
FAN_PROFILE = {0: 5, 1: 17, 2: 6, 3: 5, 4: 7, 5: 9, 6: 3, 7: 5, 8: 3, 9: 3, 10: 3, 11: 5, 12: 9, 13: 3, 16: 2}
FAN_M = 48


def through(rule, param, x):
    """what a degree-2 check of the min-sum family hands one edge when the other edge's input is x"""
    x = np.asarray(x, F32)
    if rule == "OMS":
        return np.copysign(np.maximum(F32(0), (np.abs(x) - F32(param)).astype(F32)), x).astype(F32)
    if rule == "NMS":
        return np.copysign((np.abs(x) * F32(param)).astype(F32), x).astype(F32)
    assert rule in ("MS", "AMS_MIN")
    return x


# ---------------------------------------------------------------- stars ----------

class Stars:
    """N, M, var, chk (edges for from_edges), and once bind(ex) has seen the built graph's export: per degree d the centres[n] and their
    leaves[n, d] and checks[n, d] in the centres' slot order"""

    def __init__(self, degrees, counts, seed=1):
        rng = np.random.default_rng(seed)
        self.deg = np.repeat(np.asarray(degrees, np.int64), np.asarray(counts, np.int64))      # per star
        self.N = int(self.deg.sum() + len(self.deg))
        self.M = int(self.deg.sum())
        vid = rng.permutation(self.N)
        cid = rng.permutation(self.M)
        self.centre = vid[:len(self.deg)].astype(np.int64)
        var, chk, at_v, at_c = [], [], len(self.deg), 0
        self.star_of_vn = np.empty(self.N, np.int64)
        for s, d in enumerate(self.deg):
            self.star_of_vn[self.centre[s]] = s
            for k in range(int(d)):
                leaf, c = vid[at_v + k], cid[at_c + k]
                self.star_of_vn[leaf] = s
                pair = [(self.centre[s], c), (leaf, c)]
                if rng.random() < 0.5:
                    pair.reverse()
                var += [p[0] for p in pair]
                chk += [p[1] for p in pair]
            at_v += int(d)
            at_c += int(d)
        e = rng.permutation(len(var))
        self.var, self.chk = np.asarray(var, np.int32)[e], np.asarray(chk, np.int32)[e]
        self.is_centre = np.zeros(self.N, bool)
        self.is_centre[self.centre] = True
        self.groups = None

    def bind(self, ex):
        """read the slot order off an exported graph (O.Graph.export())"""
        vn_ptr, cn_ptr, cn_var, tr = (ex[k].astype(np.int64) for k in ("vn_ptr", "cn_ptr", "cn_var", "transpose"))
        E = len(tr)
        slot_to_edge = np.empty(E, np.int64)
        slot_to_edge[tr] = np.arange(E)
        chk_of_edge = np.repeat(np.arange(len(cn_ptr) - 1), np.diff(cn_ptr))
        assert (np.diff(cn_ptr) == 2).all()
        self.groups = {}
        for d in np.unique(self.deg):
            cen = self.centre[self.deg == d]
            assert (vn_ptr[cen + 1] - vn_ptr[cen] == d).all()
            k = slot_to_edge[vn_ptr[cen][:, None] + np.arange(d)[None, :]]          # [n, d] CN-major edges of the centres' slots
            c = chk_of_edge[k]
            other = cn_ptr[c] + (1 - (k - cn_ptr[c]))                               # the other edge of the degree-2 check
            leaves = cn_var[other]
            assert (self.star_of_vn[leaves] == self.star_of_vn[cen][:, None]).all() and not self.is_centre[leaves].any()
            assert (np.diff(c, axis=1) > 0).all()                                   # a VN's slots ascend in check id
            self.groups[int(d)] = (cen, leaves, c)
        return self

    def members(self, v):
        """(degree, centre, leaves in slot order) of the star VN v belongs to"""
        s = self.star_of_vn[v]
        cen, leaves, _ = self.groups[int(self.deg[s])]
        i = int(np.nonzero(cen == self.centre[s])[0][0])
        return int(self.deg[s]), int(cen[i]), leaves[i]


def stars(degrees, counts, seed=1):
    return Stars(degrees, counts, seed)


def _seq_sum(m):
    """(((0 + m[..., 0]) + m[..., 1]) + ...) in float32"""
    s = np.zeros(m.shape[:-1], F32)
    for k in range(m.shape[-1]):
        s = (s + m[..., k]).astype(F32)
    return s


def star_flooding(st, y, rule, param, n_ite):
    """post[F, N] of the flooding schedule after n_ite = 1 or 2 iterations without a syndrome test"""
    assert n_ite in (1, 2) and st.groups is not None
    y = np.asarray(y, F32)
    Z = F32(0)
    post = np.empty_like(y)
    with np.errstate(over="ignore", invalid="ignore"):
        for d, (cen, leaves, _) in st.groups.items():
            yc, yl = y[:, cen], y[:, leaves]                                         # [F, n], [F, n, d]
            m = ((yl + Z) - Z).astype(F32)                                           # what the leaves send first
            Mk = through(rule, param, m)                                             # ... as the centre receives it
            L = through(rule, param, ((yc + Z) - Z).astype(F32))[..., None]          # what every leaf receives first
            if n_ite == 1:
                post[:, cen] = yc + _seq_sum(Mk)
                post[:, leaves] = yl + (Z + L)
            else:
                tmp_c = (yc + _seq_sum(Mk)).astype(F32)
                ext = (tmp_c[..., None] - Mk).astype(F32)                            # the NORMAL body's outputs, slot by slot
                post[:, leaves] = yl + (Z + through(rule, param, ext))
                tmp_l = (yl + (Z + L)).astype(F32)
                back = through(rule, param, (tmp_l - L).astype(F32))
                post[:, cen] = yc + _seq_sum(back)
    return post


def star_hlayered(st, y, rule, param, order=None):
    """post[F, N] after one horizontal-layered sweep over the checks in `order` (default 0 .. M - 1, the oracle's)"""
    y = np.asarray(y, F32)
    Z = F32(0)
    post = y.copy()
    rank = np.empty(st.M, np.int64)
    rank[np.arange(st.M) if order is None else np.asarray(order, np.int64)] = np.arange(st.M)
    for d, (cen, leaves, chk) in st.groups.items():
        seq = np.argsort(rank[chk], axis=1)                                         # each centre's checks in sweep order
        p = y[:, cen].copy()
        for t in range(d):
            lf = np.take_along_axis(leaves, seq[:, t:t + 1], axis=1)[:, 0]
            inc, inl = (p - Z).astype(F32), (y[:, lf] - Z).astype(F32)
            post[:, lf] = inl + through(rule, param, inc)
            p = (inc + through(rule, param, inl)).astype(F32)
        post[:, cen] = p
    return post


# ---------------------------------------------------------------- the fan ----------

def fan(info_degrees=None, M=FAN_M, seed=3):
    """(N, M, var, chk, deg[K]): information VN i (ids shuffled over the degrees) on the deg[i] least-loaded checks, VN K + c on checks c and c + 1"""
    rng = np.random.default_rng(seed)
    prof = FAN_PROFILE if info_degrees is None else info_degrees
    deg = rng.permutation(np.repeat(np.fromiter(prof.keys(), np.int64), np.fromiter(prof.values(), np.int64)))
    K = len(deg)
    load = np.zeros(M, np.int64)
    var, chk = [], []
    for v, d in enumerate(deg):
        pick = np.lexsort((rng.random(M), load))[:int(d)]
        load[pick] += 1
        var += [v] * int(d)
        chk += pick.tolist()
    for c in range(M):
        var.append(K + c)
        chk.append(c)
        if c + 1 < M:
            var.append(K + c)
            chk.append(c + 1)
    e = rng.permutation(len(var))
    return K + M, M, np.asarray(var, np.int32)[e], np.asarray(chk, np.int32)[e], deg


# ---------------------------------------------------------------- plain flooding min-sum ----------

ORDERS = ("slot", "rev", "yfirst", "drop_last", "pad")


def _vn_sum(y, c2v, vn_ptr, by_deg, order):
    """tmp[F, N] = Y + (the VN's messages in slot order), or one of the mutants"""
    E = c2v.shape[1]
    padded = np.concatenate([c2v, np.zeros((c2v.shape[0], 1), F32)], axis=1)        # slot E: nothing behind the last VN
    tmp = np.empty_like(y)
    for d, vs in by_deg.items():
        slots = vn_ptr[vs][:, None] + np.arange(d)[None, :]
        m = c2v[:, slots]                                                            # [F, n, d]
        if order == "rev":
            m = m[..., ::-1]
        elif order == "drop_last":
            m = m[..., :max(d - 1, 0)]
        elif order == "pad":
            m = np.concatenate([m, padded[:, np.minimum(vn_ptr[vs + 1], E)][..., None]], axis=2)
        if order == "yfirst":
            s = y[:, vs]
            for k in range(m.shape[-1]):
                s = (s + m[..., k]).astype(F32)
            tmp[:, vs] = s
        else:
            tmp[:, vs] = y[:, vs] + _seq_sum(m)
    return tmp


def flood(ex, y, rule, param, n_ite, order="slot"):
    """Flooding min-sum over an exported graph, no syndrome test: dict(post, hard, iters, synd_ok) as O.decode returns them"""
    assert order in ORDERS
    y = np.ascontiguousarray(y, F32)
    Fn, N = y.shape
    vn_ptr, cn_ptr, tr = ex["vn_ptr"].astype(np.int64), ex["cn_ptr"].astype(np.int64), ex["transpose"].astype(np.int64)
    dv, dc = np.diff(vn_ptr), np.diff(cn_ptr)
    by_deg = {int(d): np.nonzero(dv == d)[0] for d in np.unique(dv)}
    by_cdeg = {int(d): np.nonzero(dc == d)[0] for d in np.unique(dc)}
    c2v = np.zeros((Fn, len(tr)), F32)                                               # VN-major slots
    with np.errstate(over="ignore", invalid="ignore"):
        for _ in range(n_ite):
            tmp = _vn_sum(y, c2v, vn_ptr, by_deg, order)
            v2c = (np.repeat(tmp, dv, axis=1) - c2v).astype(F32)
            for d, cs in by_cdeg.items():
                slots = tr[cn_ptr[cs][:, None] + np.arange(d)[None, :]]              # [n, d]
                c2v[:, slots] = vlayered_ref.fold(v2c[:, slots], rule, param)
        post = _vn_sum(y, c2v, vn_ptr, by_deg, order)
    hard = (~(post >= 0)).astype(np.int32)
    return dict(post=post, hard=hard, iters=np.full(Fn, n_ite, np.int32), synd_ok=vlayered_syndrome(ex, hard))


def vlayered_syndrome(ex, hard):
    """1 where every check of the frame has even parity of hard[F, N]"""
    par = np.logical_xor.reduceat(np.asarray(hard).astype(bool)[:, ex["cn_var"]], ex["cn_ptr"][:-1], axis=1)
    return (~par.any(axis=1)).astype(np.int32)


# ---------------------------------------------------------------- input families ----------

GENERAL = ("u8", "logu", "qkd", "dyadic")
FLOOD_FAMILIES = GENERAL + ("cancel",)
LAYER_FAMILIES = GENERAL + ("cancel", "negzero")


def _sign(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def _draw(rng, family, shape):
    if family == "u8":
        x = rng.uniform(-8.0, 8.0, shape)
    elif family == "logu":
        x = np.exp(rng.uniform(np.log(1e-5), np.log(40.0), shape)) * _sign(rng, shape)
    elif family == "qkd":
        x = rng.choice(np.array([BSC_MAG, -BSC_MAG, PINNED, -PINNED, 0.0]), shape, p=[0.3, 0.3, 0.125, 0.125, 0.15])
    elif family == "dyadic":      # +-2^e (1 + j / 8), e in [-20, 23]: sums of these round differently in every order
        x = np.ldexp(1.0 + rng.integers(0, 8, shape) / 8.0, rng.integers(-20, 24, shape)) * _sign(rng, shape)
    elif family == "cancel":      # leaves: small integers (every partial sum exact); the centres are set by frames()
        x = rng.integers(1, 9, shape) * _sign(rng, shape)
    elif family == "negzero":     # -0.0 among ordinary values
        x = rng.uniform(-8.0, 8.0, shape)
        x = np.where(rng.random(shape) < 0.5, -0.0, x)
    else:
        raise ValueError(family)
    return np.asarray(x, F32)


def general_frames(N, seed, F=F_FRAMES):
    """y[F, N]: the four general families, each (frame, VN) its own draw, the family rotating over frame + VN"""
    rng = np.random.default_rng(seed)
    fam = (np.arange(F)[:, None] + np.arange(N)[None, :]) % len(GENERAL)
    y = np.empty((F, N), F32)
    for i, name in enumerate(GENERAL):
        y = np.where(fam == i, _draw(rng, name, (F, N)), y) if i else _draw(rng, name, (F, N))
    return y.astype(F32)


def frames(st, families, seed, rule="MS", param=0.0, F=F_FRAMES):
    """(y[F, N] float32, fam[F, stars]): each (frame, star) takes one family, rotating over frame + star; a star of the *cancel* family has
    integer leaves and Y_c = -(the sequential sum of what the centre receives under `rule`), so its flooding posterior after one iteration is
    exactly +0.0 (and so is the layered one where the partial sums are exact: MS, NMS, AMS_MIN); every other *negzero* star (all_negzero) is -0.0
    throughout, so the layered schedules keep a -0.0 posterior"""
    rng = np.random.default_rng(seed)
    fam = (np.arange(F)[:, None] + np.arange(len(st.deg))[None, :]) % len(families)
    fam_vn = fam[:, st.star_of_vn]
    y = np.empty((F, st.N), F32)
    for i, name in enumerate(families):
        d = _draw(rng, name, (F, st.N))
        y = np.where(fam_vn == i, d, y) if i else d
    y = y.astype(F32)
    if "negzero" in families:
        y[all_negzero(fam, families)[:, st.star_of_vn]] = F32(-0.0)
    if "cancel" in families:
        ci = families.index("cancel")
        for d, (cen, leaves, _) in st.groups.items():
            m = ((y[:, leaves] + F32(0)) - F32(0)).astype(F32)
            want = -_seq_sum(through(rule, param, m))
            sel = fam[:, st.star_of_vn[cen]] == ci
            y[:, cen] = np.where(sel, want, y[:, cen])
    return y, fam


def all_negzero(fam, families):
    """mask[F, stars]: the *negzero* stars that are -0.0 throughout (every other turn of the family)"""
    turn = np.arange(fam.shape[0])[:, None] // len(families)
    return (fam == families.index("negzero")) & (turn % 2 == 1)


def saturated_frames(st):
    """the 8-bit form at its limit, 6 frames: every input +sat, every input -sat, signs alternating over the VN index (both phases), centre
    against its leaves (both signs); sat = 127 / scale"""
    s = F32(I8_SAT)
    alt = np.where(np.arange(st.N) % 2 == 0, s, -s).astype(F32)
    anti = np.where(st.is_centre, s, -s).astype(F32)
    return np.stack([np.full(st.N, s, F32), np.full(st.N, -s, F32), alt, -alt, anti, -anti]).astype(F32)


def qkd_frames(N, seed, F=F_FRAMES):
    """The QKD mix in its coded form (as check_rules_ref.qkd_frames): (y, bits, mag, cls, erase) with y the LLRs that load_bits(bits, mag, cls) +
    load_erasures(erase) stand for"""
    rng = np.random.default_rng(seed)
    cls = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), N)
    cls[0] = 0
    bits = rng.integers(0, 2, (F, N)).astype(np.uint8)
    mag = rng.uniform(1.5, 6.0, F).astype(F32)
    mag[::3] = F32(BSC_MAG)
    erase = (rng.random((F, N)) < 0.1).astype(np.uint8)
    m = np.where(cls[None, :] == 0, mag[:, None], np.where(cls[None, :] == 1, F32(23.025850929840455), F32(0.0))).astype(F32)
    m[erase == 1] = 0.0
    y = np.where((bits == 1) & (m != 0), -m, m).astype(F32)
    return y, bits, mag, cls, erase


def tails(n, un, waves):
    """a list of n entries fills neither its last wave (un entries; one entry per wave has no such tail) nor its last workgroup (un x waves)"""
    return (un == 1 or n % un != 0) and n % (un * waves) != 0

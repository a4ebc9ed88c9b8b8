"""CPU reference of the layered BP recursions for the tests of the vertical-layered schedule (numpy, float32 throughout,
vectorised over frames).  TEST INFRASTRUCTURE ONLY.

Parity status: AFF3CT's source is not in the reference tree and no vector of Decoder_LDPC_BP_vertical_layered exists in it, so the
vertical recursion below is a restatement in the terms of the oracle's horizontal decoder (oracle/qldpc_oracle.c: decode_hlayered,
cn_update) -- parity UNPINNED against AFF3CT.  What pins it: fold() restates cn_update operation for operation, and the `hlayered`
branch, which shares fold(), the state, the syndrome test and the iteration / depth bookkeeping with the `vlayered` branch, equals
O.decode(..., "hlayered") bit for bit for MS / OMS / NMS / AMS_MIN (tests/test_vlayered_host.py).

State as in the horizontal decoder: var_nodes[N] = Y, messages[E] = 0 (CN-major, a check's edges in col_to_rows order).  One
vertical iteration:

    for v in VN order:
        for each check c of v, in the VN's slot order (vn_ptr order):
            in[i]  = var_nodes[v_i] - messages[c, i]      for ALL i of check c (v's own position p included)
            out[.] = cn_update(rule, in)                   (sign0 from the coset target)
            messages[c, p] = out[p]                        ONLY v's own edge is written
            var_nodes[v]   = in[p] + out[p]                ONLY v's posterior is written
    then check_syndrome_soft(var_nodes) after EVERY iteration, the last included

`class_ptr` (optional, with `order`): consecutive runs of `order` whose VNs share no check.  The VNs of such a run touch disjoint
messages and read only each other's untouched posteriors, so the run is worked through slot by slot for all its VNs at once (one
fold per check degree); without it every VN is a run of its own -- the plain sequential sweep.  Both give the same floats.
"""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FLT_MIN = np.finfo(F32).tiny
ONE_MINUS_EPS = F32(1) - np.finfo(F32).eps
EXACT_RULES = ("MS", "OMS", "NMS", "AMS_MIN")


def _fmin(a, b):          # std::min(a, b) = (b < a) ? b : a
    return np.where(b < a, b, a)


def _fmax(a, b):          # std::max(a, b) = (a < b) ? b : a
    return np.where(a < b, b, a)


def _corr_l2(x):
    t = (F32(0.6) - F32(0.24) * np.abs(x)).astype(F32)
    return np.where(t > 0, t, F32(0)).astype(F32)


def _ams_min(rule, a, b):
    m = np.where(a < b, a, b)
    if rule == "AMS_MIN":
        return _fmin(a, b)
    if rule == "AMS_MINSTAR":
        return (m + np.log(F32(1) + np.exp(-(a + b))) - np.log(F32(1) + np.exp(-np.abs(a - b)))).astype(F32)
    r = (m + _corr_l2(a + b) - _corr_l2(a - b)).astype(F32)
    return np.where(r > 0, r, F32(0)).astype(F32)


def fold(inn, rule, param=0.0, sign0=None):
    """cn_update of the oracle on inn[..., deg] (float32): the outgoing messages out[..., deg].  sign0[...] (bool): initial sign of the fold."""
    inn = np.asarray(inn, F32)
    deg = inn.shape[-1]
    a = np.abs(inn)
    sg = np.signbit(inn)
    sign = np.logical_xor.reduce(sg, axis=-1)
    if sign0 is not None:
        sign = np.logical_xor(sign, sign0)
    param = F32(param)
    with np.errstate(all="ignore"):
        if rule in ("MS", "OMS", "NMS"):
            min1 = np.full(inn.shape[:-1], FLT_MAX, F32)
            min2 = min1.copy()
            for i in range(deg):
                min2 = _fmin(min2, _fmax(a[..., i], min1))
                min1 = _fmin(min1, a[..., i])
            if rule == "MS":
                cst1, cst2 = _fmax(F32(0), min2), _fmax(F32(0), min1)
            elif rule == "OMS":
                cst1, cst2 = _fmax(F32(0), (min2 - param).astype(F32)), _fmax(F32(0), (min1 - param).astype(F32))
            else:
                cst1, cst2 = (min2 * param).astype(F32), (min1 * param).astype(F32)
            r = np.where(a == min1[..., None], cst1[..., None], cst2[..., None])
        elif rule == "SPA":
            t = np.tanh(a * F32(0.5)).astype(F32)
            product = np.ones(inn.shape[:-1], F32)
            for i in range(deg):
                product = (product * t[..., i]).astype(F32)
            q = (product[..., None] / t).astype(F32)
            q = np.where(q < F32(1), q, ONE_MINUS_EPS).astype(F32)
            r = (F32(2) * np.arctanh(q)).astype(F32)
        elif rule == "LSPA":
            t = np.tanh(a * F32(0.5)).astype(F32)
            lt = np.where(t != 0, np.log(np.where(t != 0, t, F32(1))), FLT_MIN).astype(F32)
            s = np.zeros(inn.shape[:-1], F32)
            for i in range(deg):
                s = (s + lt[..., i]).astype(F32)
            q = (s[..., None] - lt).astype(F32)
            q = np.where(q != 0, np.exp(q), ONE_MINUS_EPS).astype(F32)
            r = (F32(2) * np.arctanh(q)).astype(F32)
        else:
            mn = np.full(inn.shape[:-1], FLT_MAX, F32)
            dmin = mn.copy()
            for i in range(deg):
                lt = a[..., i] < mn
                other = np.where(lt, mn, a[..., i])
                mn = np.where(lt, a[..., i], mn)
                dmin = _ams_min(rule, dmin, other)
            delta = _fmax(F32(0), _ams_min(rule, dmin, mn))
            dmin = _fmax(F32(0), dmin)
            r = np.where(a == mn[..., None], dmin[..., None], delta[..., None])
    neg = np.logical_xor(sign[..., None], sg)
    return np.copysign(r.astype(F32), np.where(neg, F32(-1), F32(1))).astype(F32)


def syndrome_zero(ex, post, target=None):
    """check_syndrome_soft on post[F, N]: True where every check's parity of signbit(post) equals its target (0 without one)"""
    s = np.signbit(post)[:, ex["cn_var"]]
    cs = np.logical_xor.reduceat(s, ex["cn_ptr"][:-1], axis=1)
    if target is not None:
        cs = np.logical_xor(cs, np.asarray(target).astype(bool))
    return ~cs.any(axis=1)


def _runs(ex, order, class_ptr):
    """per run of check-disjoint VNs, per slot index t, per check degree: (vns, edge k of (v, c), first edge b, deg)"""
    cn_ptr, vn_ptr, vn_chk, tr = ex["cn_ptr"].astype(np.int64), ex["vn_ptr"].astype(np.int64), ex["vn_chk"], ex["transpose"]
    E = len(tr)
    slot_to_edge = np.empty(E, np.int64)
    slot_to_edge[tr] = np.arange(E)
    order = np.asarray(order, np.int64)
    if class_ptr is None:
        class_ptr = np.arange(len(order) + 1)
    plan = []
    for l in range(len(class_ptr) - 1):
        vs = order[class_ptr[l]:class_ptr[l + 1]]
        dv = vn_ptr[vs + 1] - vn_ptr[vs]
        steps = []
        for t in range(int(dv.max()) if len(vs) else 0):
            sel = vs[dv > t]
            slots = vn_ptr[sel] + t
            c = vn_chk[slots].astype(np.int64)
            assert len(np.unique(c)) == len(c), "VNs of one run share a check"
            k = slot_to_edge[slots]
            b = cn_ptr[c]
            deg = cn_ptr[c + 1] - b
            for d in np.unique(deg):
                m = deg == d
                steps.append((sel[m], k[m], b[m], int(d), c[m]))
        plan.append(steps)
    return plan


def decode(ex, llr, rule="NMS", param=0.0, n_ite=10, schedule="vlayered", order=None, class_ptr=None, enable_syndrome=True,
           syndrome_depth=1, target=None):
    """ex = O.Graph.export(); llr[F, N].  Returns dict(post, hard, iters, synd_ok) like O.decode.
    schedule "hlayered": checks c = 0..M-1 (decode_hlayered); "vlayered": VNs in `order` (default 0..N-1)."""
    cn_ptr, cn_var = ex["cn_ptr"].astype(np.int64), ex["cn_var"].astype(np.int64)
    llr = np.ascontiguousarray(llr, F32)
    if llr.ndim == 1:
        llr = llr[None, :]
    Fn, N = llr.shape
    M, E = len(cn_ptr) - 1, len(cn_var)
    tgt = None if target is None else np.asarray(target).reshape(Fn, M).astype(bool)
    post = llr.copy()
    msg = np.zeros((Fn, E), F32)
    iters = np.full(Fn, n_ite, np.int32)
    depth = np.zeros(Fn, np.int64)
    act = np.ones(Fn, bool)
    syndrome_depth = max(1, int(syndrome_depth))
    if schedule == "vlayered":
        plan = _runs(ex, np.arange(N) if order is None else order, class_ptr)
    for ite in range(n_ite):
        idx = np.nonzero(act)[0]
        if len(idx) == 0:
            break
        P, Mg = post[idx], msg[idx]
        T = None if tgt is None else tgt[idx]
        if schedule == "hlayered":
            for c in range(M):
                b, e = cn_ptr[c], cn_ptr[c + 1]
                vs = cn_var[b:e]
                inn = P[:, vs] - Mg[:, b:e]
                out = fold(inn, rule, param, None if T is None else T[:, c])
                Mg[:, b:e] = out
                P[:, vs] = inn + out
        else:
            for steps in plan:
                for vs, k, b, d, c in steps:
                    e = b[:, None] + np.arange(d)[None, :]            # [n, d] edges of the checks
                    inn = P[:, cn_var[e]] - Mg[:, e]                   # [F, n, d]
                    out = fold(inn, rule, param, None if T is None else T[:, c])
                    p = (k - b)[None, :, None]
                    own_in = np.take_along_axis(inn, p, axis=2)[:, :, 0]
                    own_out = np.take_along_axis(out, p, axis=2)[:, :, 0]
                    Mg[:, k] = own_out
                    P[:, vs] = own_in + own_out
        post[idx], msg[idx] = P, Mg
        if enable_syndrome:
            z = syndrome_zero(ex, P, T)
            depth[idx] = np.where(z, (depth[idx] + 1) % syndrome_depth, 0)
            stop = z & (depth[idx] == 0)
            iters[idx[stop]] = ite + 1
            act[idx[stop]] = False
    hard = (~(post >= 0)).astype(np.int32)
    s = hard[:, cn_var].astype(bool)
    par = np.logical_xor.reduceat(s, cn_ptr[:-1], axis=1)
    if tgt is not None:
        par = np.logical_xor(par, tgt)
    return dict(post=post, hard=hard, iters=iters, synd_ok=(~par.any(axis=1)).astype(np.int32))


def vn_levels(ex):
    """number of levels of level(v) = 1 + max level of any earlier VN sharing a check (the natural-order schedule)"""
    vn_ptr, vn_chk = ex["vn_ptr"], ex["vn_chk"]
    last = np.zeros(len(ex["cn_ptr"]) - 1, np.int64)
    top = 0
    for v in range(len(vn_ptr) - 1):
        cs = vn_chk[vn_ptr[v]:vn_ptr[v + 1]]
        l = (int(last[cs].max()) if len(cs) else 0) + 1
        last[cs] = l
        top = max(top, l)
    return top

"""Float64 restatement of the soft check-node rules, the forests that isolate one check update, and their input families.

Plain numpy, no device.  cn_out(rule, param, x) restates cn_update of oracle/qldpc_oracle.c -- AFF3CT's tools::Update_rule_{SPA,LSPA,AMS}
semantics, to which the oracle is pinned, NOT "true" belief propagation -- in float64, in the oracle's edge order:

  SPA    the division form prod_all / t_i with t = tanh(|x| / 2); NaN (an erased edge's own message, 0 / 0) or a value >= 1 becomes
         1 - 2^-23; then 2 atanh.  An erased edge's own message is therefore the clamp, 2 atanh(1 - 2^-23) = 16.6355.
  LSPA   the log-domain form: term = log t, FLT_MIN (a POSITIVE number, AFF3CT's quirk) for an erased edge; s = sum - term_i;
         v = exp(s), or 1 - 2^-23 where s == 0; then the kernel's documented extra clamp "t < 1 ? t : 1 - eps"; then 2 atanh.
         The oracle has no such clamp and returns inf there, through atanhf(1) (fp32 exp of a tiny negative s rounds to 1): those elements
         are left out of the oracle comparison only (tests/test_check_rules_host.py counts them), never out of a kernel comparison.
  AMS_MINSTAR / AMS_MINSTAR_L2   the min* recursion over the edges in order, starting from FLT_MAX, as the oracle runs it.

The min-sum family (MS, OMS, NMS, AMS_MIN) needs no restatement: the oracle is its bit-exact reference.
Domain: finite inputs (no inf, no NaN).

forest(degrees): a code of disjoint checks, check c owns degrees[c] VNs of degree 1.  One iteration with enable_syndrome=False then gives
post[v] = fl32(y[v] + m[v]) with m the rule applied to the channel values of that check, on both engines, under the flooding and the
horizontal-layered schedule: a VN with one edge sends y (flooding: (y + 0) - 0, see sent()).  The vertical-layered sweep works through a
check once per VN and rebuilds the inputs of the VNs it has already swept as (y_i + m_i) - m_i, which is not y_i in fp32 (and is +0.0 for
y_i = -0.0, and 0 for |y_i| below an ulp of m_i): only the VN of each check that is swept first sees the channel values themselves
(first_swept()).  The bit-exact reference of that schedule is tests/vlayered_ref.py.

Tolerances (derivation in DESIGN.md, "Check-node rules against a float64 restatement"): with M the restatement's message,
  SPA, LSPA   tol = K * 2^-23 * (dc * sinh(min(|M|, 17)) + |M| + 1) + 2^-23 * |y + M|
  min* rules  tol = K * 2^-23 * dc * (1 + |M|)                     + 2^-23 * |y + M|
The last term is the rounding of the fp32 posterior through which the message is observed.  worst_k() returns the smallest K that covers an
observed posterior array.

The syndrome form: cn_out(..., s) and messages(..., target=) take a target bit per (frame, check); a set bit flips the sign of every message of
its check and changes nothing else, so the tolerances hold as they are.  targets() builds the bits, forest W gives a target row three words.
Binary16 message storage (flooding): f16_interval() restates the stored message as a binary16 number between lo16 and hi16, accept_f16() holds
a posterior to it -- bit-exactly where lo16 == hi16.
"""
import numpy as np

SOFT_RULES = [("SPA", 0.0), ("LSPA", 0.0), ("AMS_MINSTAR", 0.0), ("AMS_MINSTAR_L2", 0.0)]
MS_RULES = [("MS", 0.0), ("OMS", 0.35), ("NMS", 0.75), ("AMS_MIN", 0.0)]

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
EPS = 2.0 ** -23
CLAMP = 1.0 - EPS

FORESTS = {
    "A": (1, 2, 3, 8, 9, 12, 13, 20, 21, 27),      # every register bucket (caps 8, 12, 20, 40) and its first overflow; <= 27 and <= 32 keep the compressed check state and the chain available
    "B": (28, 32, 33, 40, 41, 64),                 # the top bucket, the generic any-degree body, the edge engine's largest segment
    "C": (65, 100, 127),                           # generic body only
    "W": (1, 2, 3, 8, 9, 12, 13) * 10,             # M = 70: a target row spans three MSB-first words, the last one ragged (A, B, C have M <= 10); degrees <= 13 keep the compressed check state, the one-launch sweep and the edge engine available
}
F_FRAMES = 130      # two full 64-frame groups and a ragged one

# Caps on K.  SPA / LSPA: twice what the fp32 oracle itself needs against this restatement (at most 7.8 over these families, degrees 1 .. 127, in
# 20 draws each; 6.4 on input_sets());
# a kernel is another fp32 evaluation of the same function, so it is held to the reference's own bound, the factor 2 is headroom for the
# finite sample.  min* rules: twice the oracle's measured worst K on the inputs of tests/test_check_rules_host.py (values next to the constants).
K_MEASURED = {"AMS_MINSTAR": 0.212, "AMS_MINSTAR_L2": 0.190}      # the oracle's worst K over input_sets() (0.211 and 0.189, rounded up), measured on the CPU by tests/test_check_rules_host.py
K_MAX = {
    "SPA": 16.0,
    "LSPA": 16.0,
    "AMS_MINSTAR": 2.0 * K_MEASURED["AMS_MINSTAR"],
    "AMS_MINSTAR_L2": 2.0 * K_MEASURED["AMS_MINSTAR_L2"],
}


def forest(degrees):
    """(N, M, var, chk): check c owns degrees[c] consecutive VNs, each VN has that one edge."""
    degrees = np.asarray(degrees, np.int64)
    N = int(degrees.sum())
    var = np.arange(N, dtype=np.int32)
    chk = np.repeat(np.arange(len(degrees), dtype=np.int32), degrees)
    return N, len(degrees), var, chk


def first_swept(degrees, vn_order):
    """mask[N]: the VN of each check that comes first in vn_order (Code.vlayer_order()), the one the vertical-layered sweep updates from the
    channel values alone"""
    pos = np.empty(len(vn_order), np.int64)
    pos[np.asarray(vn_order, np.int64)] = np.arange(len(vn_order))
    mask = np.zeros(len(vn_order), bool)
    for sl in check_slices(degrees):
        mask[sl.start + int(np.argmin(pos[sl]))] = True
    return mask


def check_slices(degrees):
    at = 0
    for d in degrees:
        yield slice(at, at + int(d))
        at += int(d)


# ---------------------------------------------------------------- the rules, float64 ----------

def _signs(x, s=0):
    """(-1)^(signbit of the other edges' product, times the check's target bit s), AFF3CT's std::signbit fold: -0.0 counts as negative.  The
    syndrome form starts the sign product from s: a set bit flips every outgoing message of the check, SPA's clamp message on an erased edge
    and the sign of a zero included"""
    neg = np.signbit(x)
    other = np.logical_xor(np.logical_xor.reduce(neg), neg)
    if s:
        other = ~other
    return np.where(other, -1.0, 1.0)


def _spa(x, s=0):
    a = np.abs(x)
    t = np.tanh(a * 0.5)
    prod = np.prod(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = prod / t
    v = np.where(v < 1.0, v, CLAMP)      # NaN and >= 1 both fail "v < 1"
    return _signs(x, s) * 2.0 * np.arctanh(v)


def _lspa(x, s=0):
    a = np.abs(x)
    t = np.tanh(a * 0.5)
    with np.errstate(divide="ignore"):
        term = np.where(t != 0.0, np.log(np.where(t != 0.0, t, 1.0)), FLT_MIN)
    tot = 0.0
    for r in term:      # the oracle's left-to-right sum
        tot += r
    d = tot - term
    v = np.where(d != 0.0, np.exp(d), CLAMP)
    v = np.where(v < 1.0, v, CLAMP)      # the kernel's extra clamp; the oracle returns inf here
    return _signs(x, s) * 2.0 * np.arctanh(v)


def _min_star(a, b):
    return min(a, b) + np.log1p(np.exp(-(a + b))) - np.log1p(np.exp(-abs(a - b)))


def _corr_l2(x):
    return max(0.6 - 0.24 * abs(x), 0.0)


def _min_star_l2(a, b):
    return max(min(a, b) + _corr_l2(a + b) - _corr_l2(a - b), 0.0)


def _ams(x, f, s=0):
    a = np.abs(x)
    mn, delta_min = FLT_MAX, FLT_MAX
    for ai in a:
        if ai < mn:
            other, mn = mn, ai
        else:
            other = ai
        delta_min = f(delta_min, other)
    delta = max(0.0, f(delta_min, mn))
    delta_min = max(0.0, delta_min)
    return _signs(x, s) * np.where(a == mn, delta_min, delta)


def cn_out(rule, param, x, s=0):
    """messages m[dc] of one check with inputs x[dc] (any float dtype; evaluated in float64) and target bit s (the syndrome form: the check
    must come out with parity s)"""
    x = np.asarray(x, np.float64)
    assert x.ndim == 1 and np.isfinite(x).all()
    if rule == "SPA":
        return _spa(x, s)
    if rule == "LSPA":
        return _lspa(x, s)
    if rule == "AMS_MINSTAR":
        return _ams(x, _min_star, s)
    if rule == "AMS_MINSTAR_L2":
        return _ams(x, _min_star_l2, s)
    raise ValueError("no restatement for %s: the oracle is the bit-exact reference of the min-sum family" % rule)


def sent(y, schedule):
    """what a VN of degree 1 with channel value y sends in the first iteration: the flooding schedule forms (y + 0) - 0, which turns -0.0
    into +0.0 (LSPA and the min-sum family fold the sign of a zero in); the layered schedules form y - 0, which keeps it"""
    y = np.asarray(y, np.float32)
    return (y + np.float32(0.0)) - np.float32(0.0) if schedule == "flooding" else y


def messages(rule, param, degrees, y, schedule="hlayered", target=None):
    """M[F, N] float64: cn_out on every check of the forest, every frame of the channel values y[F, N] as `schedule` sends them; target
    uint8 [F, M]: the target bit of every (frame, check), None = all 0"""
    y = sent(y, schedule)
    out = np.empty(y.shape, np.float64)
    for c, sl in enumerate(check_slices(degrees)):
        for f in range(y.shape[0]):
            out[f, sl] = cn_out(rule, param, y[f, sl], 0 if target is None else int(target[f, c]))
    return out


def per_vn(degrees, a):
    """a[F, M], one value per check -> [F, N], the value of each VN's check"""
    return np.repeat(np.asarray(a), np.asarray(degrees, np.int64), axis=1)


def targets(degrees, y, seed):
    """target bits uint8 [F, M] for the frames y[F, N]: frame 0 all 0 (it must reproduce the run without a target), frame 1 all 1, frames with
    f % 4 == 2 consistent (s_c = parity of signbit(y) over check c: every message then agrees in sign with its own VN, the hard decision is
    sign(y) and its syndrome is s), the others Bernoulli(1/2) per (frame, check)"""
    rng = np.random.default_rng(seed)
    F = len(y)
    t = rng.integers(0, 2, (F, len(degrees))).astype(np.uint8)
    t[0] = 0
    if F > 1:
        t[1] = 1
    neg = np.signbit(np.asarray(y, np.float32))
    for c, sl in enumerate(check_slices(degrees)):
        t[2::4, c] = np.logical_xor.reduce(neg[2::4, sl], axis=1)
    return t


# ---------------------------------------------------------------- tolerance --------------------

def tol_unit(rule, degrees, y, M):
    """(per-K part, K-free part) of the tolerance on the posterior fl32(y + M)"""
    dc = np.repeat(np.asarray(degrees, np.float64), degrees)[None, :]
    aM = np.abs(M)
    if rule in ("SPA", "LSPA"):
        per_k = EPS * (dc * np.sinh(np.minimum(aM, 17.0)) + aM + 1.0)
    else:
        per_k = EPS * dc * (1.0 + aM)
    return per_k, EPS * np.abs(np.asarray(y, np.float64) + M)


def worst_k(rule, degrees, y, M, post, skip=None):
    """smallest K with |post - (y + M)| <= tol(K) on every element (those of the boolean mask `skip` aside); inf if a posterior is not finite"""
    per_k, fixed = tol_unit(rule, degrees, y, M)
    post = np.asarray(post, np.float64)
    want = np.asarray(y, np.float64) + M
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(post - want)
        k = np.maximum(err - fixed, 0.0) / per_k
    k = np.where(np.isfinite(post) | ~np.isfinite(want), k, np.inf)
    k = np.where(np.isnan(k), np.inf, k)
    if skip is not None:
        k = np.where(skip, 0.0, k)
    return float(k.max()), k


def hard_ref(rule, degrees, y, M):
    """(hard[F, N] uint8, skip[F, N] bool): the hard decision !(y + M >= 0) of the restatement's posterior, and the elements whose sign an
    fp32 evaluation inside the tolerance may turn: 0 < |y + M| <= tol(K_MAX), or an exact cancellation y + M == 0 against a non-zero M"""
    want = np.asarray(y, np.float64) + M
    per_k, fixed = tol_unit(rule, degrees, y, M)
    skip = ((want != 0) & (np.abs(want) <= K_MAX[rule] * per_k + fixed)) | ((want == 0) & (M != 0))
    return (~(want >= 0)).astype(np.uint8), skip


def syndrome_matches(degrees, hard, target):
    """ok[F]: the parity of hard[F, N] over every check equals target[F, M]"""
    par = np.stack([np.bitwise_xor.reduce(np.asarray(hard, np.uint8)[:, sl], axis=1) for sl in check_slices(degrees)], axis=1)
    return (par == np.asarray(target, np.uint8)).all(axis=1)


# ---------------------------------------------------------------- input families --------------

SOFT_FAMILIES = ("bsc", "qkd", "u8", "u30", "logu", "weak")
MS_FAMILIES = SOFT_FAMILIES + ("zeros", "extremes")
PINNED = 23.025850929840455
BSC_MAG = 2.6


def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def draw(rng, family, dc):
    """dc channel values of one check of one frame (float32)"""
    if family == "bsc":
        x = BSC_MAG * _sign(rng, dc)
    elif family == "qkd":      # what a QKD frame feeds a check: channel bits, pinned bits, punctured (erased) bits
        x = rng.choice(np.array([BSC_MAG, -BSC_MAG, PINNED, -PINNED, 0.0]), dc, p=[0.3, 0.3, 0.125, 0.125, 0.15])
    elif family == "u8":
        x = rng.uniform(-8.0, 8.0, dc)
    elif family == "u30":
        x = rng.uniform(-30.0, 30.0, dc)
    elif family == "logu":
        x = np.exp(rng.uniform(np.log(1e-5), np.log(40.0), dc)) * _sign(rng, dc)
    elif family == "weak":
        x = rng.uniform(10.0, 25.0, dc) * _sign(rng, dc)
        x[rng.integers(dc)] = 0.3 * (1.0 if rng.random() < 0.5 else -1.0)
    elif family == "zeros":      # +-0.0 among ordinary values: std::signbit(-0.0) flips the check's sign, |x| == min1 ties
        x = rng.uniform(-8.0, 8.0, dc)
        z = rng.random(dc) < 0.5
        x[z] = np.where(rng.random(int(z.sum())) < 0.5, -0.0, 0.0)
    elif family == "extremes":      # fp32 denormals and FLT_MAX among ordinary values
        x = rng.uniform(-8.0, 8.0, dc)
        pick = rng.random(dc)
        den = pick < 0.25
        x[den] = rng.integers(1, 1 << 23, int(den.sum())).astype(np.float64) * 2.0 ** -149 * _sign(rng, int(den.sum()))
        big = pick > 0.8
        x[big] = FLT_MAX * _sign(rng, int(big.sum()))
    else:
        raise ValueError(family)
    return np.asarray(x, np.float32)


def frames(degrees, families, seed, F=F_FRAMES):
    """(y[F, N] float32, fam[F, M] indices into families): each (frame, check) is its own draw of its own family; the families rotate over
    (frame + check) so every degree meets every family F / len(families) times"""
    rng = np.random.default_rng(seed)
    N = int(np.sum(degrees))
    y = np.empty((F, N), np.float32)
    fam = np.empty((F, len(degrees)), np.int32)
    for f in range(F):
        for c, sl in enumerate(check_slices(degrees)):
            fam[f, c] = (f + c) % len(families)
            y[f, sl] = draw(rng, families[fam[f, c]], sl.stop - sl.start)
    return y, fam


def w_frames(y_a):
    """The soft inputs of forest W: block j of seven checks holds the inputs that the first seven checks of forest A (the same degrees) hold
    in frame (f + 13 j) mod F.  Every (check, inputs) pair of W is one of A, so the caps K_MAX -- the min* ones are twice a maximum measured
    on A's draws, and fresh draws of 700 small checks exceed it on the oracle itself about every second seed (dc = 2, two inputs of 1e-5:
    K = 0.35 .. 0.60 over six seeds against the cap 0.424) -- hold on W for the reason they hold on A; what W adds is where the check
    stands: M = 70, ten copies of each degree, another frame's target bit"""
    deg = FORESTS["W"]
    n = int(np.sum(deg[:7]))
    assert deg[:7] == FORESTS["A"][:7] and deg == deg[:7] * 10
    F = len(y_a)
    return np.concatenate([y_a[(np.arange(F) + 13 * j) % F, :n] for j in range(10)], axis=1)


HIGH_DEGREES = (128, 129, 130, 200)     # past the degree below which the SPA fold's product of (1 + e_j) stays finite in fp32
HIGH_FAMILIES = ("w001", "logu")


def high_frames(seed, F=24):
    """forest HIGH_DEGREES: |x| = 0.01 throughout (every 1 + e_j is 1.99) and the log-uniform family, alternating over (frame + check)"""
    rng = np.random.default_rng(seed)
    y = np.empty((F, int(np.sum(HIGH_DEGREES))), np.float32)
    for f in range(F):
        for c, sl in enumerate(check_slices(HIGH_DEGREES)):
            dc = sl.stop - sl.start
            y[f, sl] = (np.float32(0.01) * _sign(rng, dc)).astype(np.float32) if (f + c) % 2 == 0 else draw(rng, "logu", dc)
    return y


TINY_VALUES = (1e-8, 2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 1e-6)      # non-zero inputs at and below the point where fp32 exp(-|x|) rounds to 1
TINY_DEGREES = (2, 6, 41)
SPA_DOMAIN_MIN = 2.0 ** -24      # the SPA kernels' stated domain: x = 0 or |x| >= 2^-24 (qldpc_kernels.h); LSPA and the AMS rules take every finite input


def tiny_frames(seed, draws=4):
    """forest TINY_DEGREES: one edge of every check holds +-TINY_VALUES[f % 5], the others U(-8, 8); frames 0 .. 4 give the degree-2 check 3.0 as
    its other input.  Returns (y[F, N] float32, tiny[F, N] bool)"""
    rng = np.random.default_rng(seed)
    F = len(TINY_VALUES) * draws
    N = int(np.sum(TINY_DEGREES))
    y = rng.uniform(-8.0, 8.0, (F, N)).astype(np.float32)
    tiny = np.zeros((F, N), bool)
    for f in range(F):
        for sl in check_slices(TINY_DEGREES):
            p = sl.start + int(rng.integers(sl.stop - sl.start))
            y[f, p] = np.float32(TINY_VALUES[f % len(TINY_VALUES)]) * (1.0 if rng.random() < 0.5 else -1.0)
            tiny[f, p] = True
            if f < len(TINY_VALUES) and sl.stop - sl.start == 2:
                y[f, sl.start + sl.stop - 1 - p] = np.float32(3.0)
    return y, tiny


def qkd_frames(degrees, seed, F=F_FRAMES):
    """The QKD-mix family in its coded form: (y[F, N] float32, bits[F, N] u8, mag[F] float32, cls[N] u8, erase[F, N] u8) with y the LLRs that
    load_bits(bits, mag, cls) + load_erasures(erase) stand for: class 0 = +-mag[f], class 1 = +-23.03 (pinned), class 2 = 0 (punctured), and
    an erasure row zeroes single VNs of single frames.  A zero is the harness's `LLR = 0`: +0.0 whatever bit was received"""
    rng = np.random.default_rng(seed)
    N = int(np.sum(degrees))
    cls = rng.choice(np.array([0, 0, 0, 1, 2], np.uint8), N)
    cls[0] = 0
    bits = rng.integers(0, 2, (F, N)).astype(np.uint8)
    mag = rng.uniform(1.5, 6.0, F).astype(np.float32)
    mag[::3] = np.float32(BSC_MAG)
    erase = (rng.random((F, N)) < 0.1).astype(np.uint8)
    m = np.where(cls[None, :] == 0, mag[:, None], np.where(cls[None, :] == 1, np.float32(PINNED), np.float32(0.0))).astype(np.float32)
    m[erase == 1] = 0.0
    y = np.where((bits == 1) & (m != 0), -m, m).astype(np.float32)
    return y, bits, mag, cls, erase


# ---------------------------------------------------------------- the shared inputs and their reference, computed once ----------

_SETS = None
_MSG = {}


def input_sets():
    """every input set of the tolerance comparisons, host and GPU: name -> (degrees, y[F, N] float32)"""
    global _SETS
    if _SETS is None:
        s = {}
        for i, (name, deg) in enumerate(FORESTS.items()):
            s[name] = (deg, w_frames(s["A"][1]) if name == "W" else frames(deg, SOFT_FAMILIES, seed=100 + i)[0])
            s[name + "-coded"] = (deg, qkd_frames(deg, seed=200 + i)[0])
        s["high"] = (HIGH_DEGREES, high_frames(seed=300))
        ty, tmask = tiny_frames(seed=400)
        s["tiny"] = (TINY_DEGREES, ty)
        in_domain = np.abs(ty[tmask].reshape(len(ty), -1)[:, 0]) >= np.float32(SPA_DOMAIN_MIN)
        s["tiny-spa"] = (TINY_DEGREES, ty[in_domain].copy())      # the frames of "tiny" inside the SPA kernels' domain
        for v in s.values():
            v[1].setflags(write=False)
        _SETS = s
    return _SETS


def messages_cached(rule, param, name, degrees, y, schedule, target=None):
    """messages() of an input set, computed once per (rule, set, target) -- twice where the set holds a -0.0, which flooding sends as +0.0.
    A target bit only flips the sign of its check's messages, exactly (_signs), so the set is evaluated once without a target and negated
    per check; tests/test_check_rules_host.py holds this to messages(..., target=) itself, bit for bit"""
    flood = schedule == "flooding" and bool((np.signbit(y) & (y == 0)).any())
    key = (rule, name, flood, None)
    if key not in _MSG:
        _MSG[key] = messages(rule, param, degrees, y, "flooding" if flood else "hlayered")
        _MSG[key].setflags(write=False)
    if target is None:
        return _MSG[key]
    tkey = (rule, name, flood, np.asarray(target, np.uint8).tobytes())
    if tkey not in _MSG:
        _MSG[tkey] = np.where(per_vn(degrees, target) != 0, -_MSG[key], _MSG[key])
        _MSG[tkey].setflags(write=False)
    return _MSG[tkey]


_HARD = None
HARD_FAMILIES = ("bsc", "u8", "logu")


def hard_sets():
    """The soft inputs of the flag and hard-word tests, name -> (degrees, y): forests A, B and W (W from A's draws, as above) with the three
    families whose messages stay clear of the clamp.  tol(K_MAX) grows with sinh |M|, and it decides which hard decisions the comparison must
    leave open (hard_ref): on input_sets() that is 2 .. 5 % of the SPA elements (the QKD mix: 28 %), here at most 1 % on A and B
    (tests/test_check_rules_host.py).  W stays above 1 % whatever the inputs -- a check of degree 1 sends the clamp, 16.6, whose tolerance is
    15.8, and W has 10 of them among 480 VNs -- so W serves the flag comparison, which leaves nothing out, and not the hard-word one"""
    global _HARD
    if _HARD is None:
        y_a = frames(FORESTS["A"], HARD_FAMILIES, seed=700)[0]
        _HARD = {"A-hard": (FORESTS["A"], y_a), "B-hard": (FORESTS["B"], frames(FORESTS["B"], HARD_FAMILIES, seed=701)[0]),
                 "W-hard": (FORESTS["W"], w_frames(y_a))}
        for v in _HARD.values():
            v[1].setflags(write=False)
    return _HARD


def get_set(name):
    return hard_sets()[name] if name.endswith("-hard") else input_sets()[name]


_TGT = {}


def target_cached(name):
    """the target bits of an input set, uint8 [F, M] (targets(), one seed per set)"""
    if name not in _TGT:
        deg, y = get_set(name)
        _TGT[name] = targets(deg, y, seed=600 + sum(map(ord, name)))
        _TGT[name].setflags(write=False)
    return _TGT[name]


# ---------------------------------------------------------------- binary16 message storage ----------

def rne16(a):
    """round to nearest even to binary16 and back to float32 (what the oracle's stq() does, tests/test_oracle.py)"""
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float16).astype(np.float32)


def f16_interval(rule, param, degrees, y, target=None):
    """The restatement with binary16 message storage under flooding: (x16, M, lo16, hi16).  x16 = rne16((y + 0) - 0) is what qk_first_v2c stores,
    M = cn_out on x16 in float64 (under `target`, if one is given), and the stored check-to-variable message is a binary16 number between
    lo16 = float16(M - t) and hi16 = float16(M + t), t the K-dependent part of the tolerance at K_MAX[rule] (the fp32 evaluation error before
    the rounding)"""
    x16 = rne16(sent(y, "flooding"))
    M = messages(rule, param, degrees, x16, target=target)
    t = K_MAX[rule] * tol_unit(rule, degrees, y, M)[0]
    with np.errstate(over="ignore"):
        return x16, M, (M - t).astype(np.float16), (M + t).astype(np.float16)


# The share of elements with lo16 == hi16, where accept_f16() is a bit-exact comparison, measured on the CPU by tests/test_check_rules_host.py on
# input_sets(); the test there asserts a floor of 0.8 x these, so that a later change of inputs or caps cannot empty the bit-exact part unseen.
SHARP_MEASURED = {
    "SPA": {"A": 0.480, "B": 0.262, "C": 0.084},
    "LSPA": {"A": 0.608, "B": 0.343, "C": 0.084},
    "AMS_MINSTAR": {"A": 0.586, "B": 0.328, "C": 0.181},
    "AMS_MINSTAR_L2": {"A": 0.661, "B": 0.494, "C": 0.359},
}

_F16 = {}


def f16_interval_cached(rule, param, name, target=False):
    """f16_interval() of an input set, under target_cached(name) if `target`"""
    if (rule, name, target) not in _F16:
        deg, y = get_set(name)
        _F16[rule, name, target] = f16_interval(rule, param, deg, y, target_cached(name) if target else None)
        for a in _F16[rule, name, target]:
            a.setflags(write=False)
    return _F16[rule, name, target]


def accept_f16(y, post, lo16, hi16):
    """bool per element: there is a binary16 h with lo16 <= h <= hi16 whose fl32(y + fl32(0 + h)) -- the flooding posterior of a VN with one
    edge -- equals post bit for bit.  The candidates are float16(float64(post) - y) and its two binary16 neighbours, and lo16 and hi16
    themselves: fl32(y + h) is monotone in h, so the h that give post form an interval around post - y; if it reaches beyond [lo16, hi16]
    one of the two ends lies in it, if not its binary16 numbers include a neighbour of post - y (under a large y an ulp of the posterior
    spans several binary16 numbers, so the neighbours alone would not do).  Infinities compare as themselves.  Sharp in two ways: the
    posterior must be y plus a binary16 NUMBER (a message kept in fp32, or rounded toward zero, fails), and where lo16 == hi16 the comparison
    is bit-exact"""
    y = np.asarray(y, np.float32)
    post = np.ascontiguousarray(post, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h0 = (post.astype(np.float64) - y.astype(np.float64)).astype(np.float16)
        ok = np.zeros(y.shape, bool)
        for h in (h0, np.nextafter(h0, np.float16(np.inf)), np.nextafter(h0, np.float16(-np.inf)), np.asarray(lo16), np.asarray(hi16)):
            got = (y + (np.float32(0.0) + h.astype(np.float32))).astype(np.float32)
            ok |= (lo16 <= h) & (h <= hi16) & (got.view(np.uint32) == post.view(np.uint32))
    return ok

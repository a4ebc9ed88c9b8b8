"""Guessing rounds restated in numpy (test infrastructure, shared by tests/test_guess_host.py, tests/test_guess_gpu.py and
tests/test_mc_guess_gpu.py): the trial rows by ranks over np.flatnonzero, the verdict over the trials, the schedule as a rule over the pool
count, the pool as a Python stack, and the per-frame loop over mc_frames_host -> encoder -> LLRs -> CPU oracle.  Nothing here calls the library
under test except where a function takes the schedule function as an argument."""
import numpy as np

import blind_ref
import mc_oracle
import mc_ref

FRESH, TRIALS = 1, 2


def trial_bits(weak, hard, t):
    """weak, hard [N] 0/1 -> (known, value) [N] 0/1 of trial t: the VN of rank j of the guess set is pinned to hard ^ bit j of t"""
    vns = np.flatnonzero(weak)
    known = np.zeros(weak.size, np.uint8)
    value = np.zeros(weak.size, np.uint8)
    known[vns] = 1
    value[vns] = [int(hard[v]) ^ ((t >> j) & 1) for j, v in enumerate(vns)]
    return known, value


def trial_rows(N, g, weak_row, hard_row):
    """packed rows of one source -> (known, value) uint32 [2^g, ceil(N/32)] of all its trials.  The rule is stated on the words of the row, so the
    restatement unpacks all 32 W positions: a guess row from the select never has a bit at or beyond N"""
    W = (N + 31) // 32
    weak, hard = blind_ref.unpack_row(weak_row, 32 * W), blind_ref.unpack_row(hard_row, 32 * W)
    rows = [trial_bits(weak, hard, t) for t in range(1 << g)]
    return np.stack([blind_ref.pack_row(k) for k, _ in rows]), np.stack([blind_ref.pack_row(v) for _, v in rows])


def pick(N, ok, hard_rows):
    """ok [T], packed hard rows [T, W] -> (winner or -1, n_ok, ambiguous): the lowest ok trial; ambiguous iff an ok trial differs from it in a valid bit"""
    good = np.flatnonzero(np.asarray(ok) != 0)
    if good.size == 0:
        return -1, 0, 0
    bits = np.stack([blind_ref.unpack_row(r, N) for r in hard_rows])
    return int(good[0]), int(good.size), int(any((bits[t] != bits[good[0]]).any() for t in good))


def next_launch(g, batch, pool, input_left):
    """the schedule (include/qldpc.h, "guessing rounds inside the Monte-Carlo loop") -> (kind, n) or None"""
    S = batch // (1 << g)
    if pool and pool >= S:
        return TRIALS, S
    if input_left:
        return FRESH, min(batch, input_left)
    return (TRIALS, pool) if pool else None


def replay(failed, g, batch, schedule=next_launch, stop=None):
    """The pool as a stack of frame slots, driven by `schedule`: failed[i] = the first decode of input frame i fails.  A fresh launch appends its
    failed frames in slot order (none with g = 0, which pools nothing); a trial launch takes the last n.  stop(launch) -> True ends the input after
    that launch.  -> (launches = dict(kind, frames, src = the fresh launch each slot came in with), the largest pool count, frames drawn)"""
    pool, drawn, left, launches, peak, src_of = [], 0, len(failed), [], 0, {}
    while True:
        nxt = schedule(g, batch, len(pool), left)
        if nxt is None:
            break
        kind, n = nxt
        if kind == FRESH:
            assert 1 <= n <= min(batch, left)
            slots = list(range(drawn, drawn + n))
            for i in slots:
                src_of[i] = len(launches)
            drawn, left = drawn + n, left - n
            if g:
                pool.extend(i for i in slots if failed[i])
            peak = max(peak, len(pool))
        else:
            assert kind == TRIALS and 1 <= n <= len(pool) and n << g <= batch
            slots = pool[len(pool) - n:]
            del pool[len(pool) - n:]
        launches.append(dict(kind=kind, frames=slots, src=[src_of[i] for i in slots]))
        if stop is not None and stop(launches[-1]):
            left = 0
    assert not pool
    return launches, peak, drawn


def loop(decode, llr, chan, g):
    """Per frame: decode(llr[F', N]) -> dict(post, hard, synd_ok, iters) is the oracle.  A frame whose first decode fails takes its g weakest channel
    VNs (chan[N] bool) and is decoded again 2^g times from the same LLRs with the trial's values pinned.
    -> dict(first = the first decodes, weak [F, N] 0/1 guess sets, winner [F] (-1: none; -2: the first decode closed), n_ok [F], ambiguous [F],
    trial_iters [F] = the iterations of all trials of the frame, last = dict(hard, synd_ok, iters): the winner's decode of a rescued frame, else the first)"""
    F, N = llr.shape
    first = decode(llr)
    last = {k: np.array(first[k], copy=True) for k in ("hard", "synd_ok", "iters")}
    weak = np.zeros((F, N), np.uint8)
    winner, n_ok, amb, t_it = np.full(F, -2, np.int32), np.zeros(F, np.int64), np.zeros(F, np.int64), np.zeros(F, np.int64)
    for f in np.flatnonzero(first["synd_ok"] == 0):
        winner[f] = -1
        if g == 0:
            continue
        weak[f, blind_ref.weakest_vns(first["post"][f], g, chan.astype(np.uint8))] = 1
        rows = [trial_bits(weak[f], first["hard"][f], t) for t in range(1 << g)]
        res = decode(blind_ref.pinned(np.repeat(llr[f][None], len(rows), 0), np.stack([k for k, _ in rows]), np.stack([v for _, v in rows])))
        good = np.flatnonzero(res["synd_ok"] != 0)
        t_it[f], n_ok[f] = int(res["iters"].sum()), good.size
        if good.size:
            w = winner[f] = int(good[0])
            amb[f] = int(any((res["hard"][t] != res["hard"][w]).any() for t in good))
            last["hard"][f], last["synd_ok"][f], last["iters"][f] = res["hard"][w], res["synd_ok"][w], res["iters"][w]
    return dict(first=first, weak=weak, winner=winner, n_ok=n_ok, ambiguous=amb, trial_iters=t_it, last=last)


ROW = mc_oracle.COUNTERS + ("disclosed",)


def rows_of(ref, sel=None):
    """the three counter rows -- closed at once, rescued, open -- of the frames sel (None = all) of a reference"""
    w = ref["winner"]
    sel = np.arange(w.size) if sel is None else np.asarray(sel)
    rows = []
    for idx in (sel[w[sel] == -2], sel[w[sel] >= 0], sel[w[sel] == -1]):
        ctr = mc_oracle.tally({k: v[idx] for k, v in ref["f"].items()}, ref["n_chan"])[0]
        ctr["disclosed"] = 0
        rows.append(ctr)
    return rows


def sums_of(ref, g, sel=None):
    w = ref["winner"]
    sel = np.arange(w.size) if sel is None else np.asarray(sel)
    failed = int((w[sel] != -2).sum())
    return dict(rescued=int((w[sel] >= 0).sum()), open=int((w[sel] == -1).sum()), trials=(failed << g) if g else 0, trial_iter_sum=int(ref["trial_iters"][sel].sum()),
                n_ok_sum=int(ref["n_ok"][sel].sum()), ambiguous=int(ref["ambiguous"][sel].sum()))


def reference(s, kind, qber, first, n, g, erased=()):
    """frames [first, first + n) of _Setup s through the loop -> the dict of loop() plus f = the verdicts of the last decodes, n_chan and rows; computed
    once per argument set and left unchanged"""
    key = ("guess", kind, qber, first, n, g, tuple(int(v) for v in erased))
    if key in s._ref:
        return s._ref[key]
    info_w, flip_w = s.q.mc_frames_host(s.K, s.N, mc_oracle.SEED, qber, first, n, info_bits_pos=s.pos)
    cw = s.codewords(info_w)
    flips = mc_ref.unpack(flip_w, s.N)
    llr = mc_oracle.bsc_llrs(s.q, cw ^ flips, s.cls, qber, erased)
    out = loop(lambda rows: mc_oracle.oracle(s, kind, rows), llr, s.cls == 0, g)
    out["f"] = mc_oracle.verdicts(out["last"], cw, s.pos, flips, s.cls == 0)
    out["n_chan"] = int((s.cls == 0).sum())
    out["rows"] = rows_of(out)
    for a in (out["weak"], out["winner"], out["n_ok"], out["ambiguous"], out["trial_iters"]):
        a.setflags(write=False)
    s._ref[key] = out
    return out


def got_rows(res):
    """the rows of a MonteCarlo.guess result as dicts"""
    return [{k: int(row[k]) for k in ROW} for row in res["rows"]]


def add_rows(a, b):
    return [{k: (max(x[k], y[k]) if k == "iter_max" else x[k] + y[k]) for k in ROW} for x, y in zip(a, b)]


def errors_of(rows):
    """what the stop rule counts: frames closed or rescued wrong, and the open ones"""
    return rows[0]["frame_errors"] + rows[1]["frame_errors"] + rows[2]["frames"]

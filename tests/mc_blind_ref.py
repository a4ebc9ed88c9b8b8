"""Blind reconciliation rounds of the Monte-Carlo loop restated in numpy (test infrastructure, shared by tests/test_mc_blind.py and
tests/test_mc_blind_gpu.py): the schedule as a rule over the pool counts, the pools as Python stacks, and the per-frame round loop over
mc_frames_host -> encoder -> LLRs -> CPU oracle.  Nothing here calls the library under test except where a function takes the schedule
function as an argument."""
import numpy as np

import blind_ref
import mc_oracle
import mc_ref


def next_launch(pool, input_left, batch):
    """the schedule (include/qldpc.h, "blind reconciliation rounds"): pool[R + 1] counts, pool[0] not read -> (level, n) or None"""
    R = len(pool) - 1
    full = [r for r in range(1, R + 1) if pool[r] >= batch]
    if full:
        return max(full), batch
    if input_left:
        return 0, min(batch, input_left)
    waiting = [r for r in range(1, R + 1) if pool[r]]
    return (min(waiting), pool[min(waiting)]) if waiting else None


def replay(close_round, R, batch, schedule=next_launch, stop=None):
    """The pools as stacks of frame slots, driven by `schedule`: close_round[i] = the round in which input frame i closes (-1: never).  A launch
    at level r takes the last n entries of pool r; its frames with close_round != r go on to pool r + 1 in slot order (after round R: they end
    open).  stop(launch) -> True ends the input after that launch.  -> list of launches dict(level, frames = the slots in launch order, opened =
    how many went on, src = the level-0 launch each slot came in with), and the largest count any pool reached."""
    n_in = len(close_round)
    pools = [[] for _ in range(R + 1)]
    drawn, left, launches, peak, src_of = 0, n_in, [], 0, {}
    while True:
        nxt = schedule([len(p) for p in pools], left, batch)
        if nxt is None:
            break
        level, n = nxt
        if level == 0:
            slots = list(range(drawn, drawn + n))
            for i in slots:
                src_of[i] = len(launches)
            drawn, left = drawn + n, left - n
        else:
            assert 1 <= n <= len(pools[level])
            slots = pools[level][len(pools[level]) - n:]
            del pools[level][len(pools[level]) - n:]
        assert 1 <= n <= batch and len(slots) == n
        on = [i for i in slots if close_round[i] != level]
        if level < R:
            pools[level + 1].extend(on)
            peak = max(peak, len(pools[level + 1]))
        launches.append(dict(level=level, frames=slots, opened=len(on), src=[src_of[i] for i in slots]))
        if stop is not None and stop(launches[-1]):
            left = 0
    assert all(not p for p in pools)
    return launches, peak, drawn


def loop(decode, llr, alice, chan, d, R):
    """The round loop per frame: decode(llr[F', N]) -> dict(post, hard, synd_ok, iters) is the oracle.  Round 0 .. R; a frame closes in the
    first round with synd_ok; a frame still open after round r < R asks for its min(d, candidates) weakest positions among the channel VNs
    (chan[N] bool) it does not know yet and gets Alice's bits there; it is decoded again from the same LLRs with the known bits pinned.
    -> (close_round[F] or -1, known[F, N] 0/1 at the frame's last decode, last = dict(hard, synd_ok, iters) of the frame's last decode)"""
    F, N = llr.shape
    known = np.zeros((F, N), np.uint8)
    close = np.full(F, -1, np.int32)
    last = dict(hard=np.zeros((F, N), np.int32), synd_ok=np.zeros(F, np.int32), iters=np.zeros(F, np.int32))
    for r in range(R + 1):
        live = np.flatnonzero(close < 0)
        if live.size == 0:
            break
        res = decode(blind_ref.pinned(llr[live], known[live], alice[live]))
        for i, f in enumerate(live):
            last["hard"][f], last["synd_ok"][f], last["iters"][f] = res["hard"][i], res["synd_ok"][i], res["iters"][i]
            if res["synd_ok"][i]:
                close[f] = r
            elif r < R:
                cand = (chan & (known[f] == 0)).astype(np.uint8)
                known[f, blind_ref.weakest_vns(res["post"][i], d, cand)] = 1
    return close, known, last


def rows_of(close, known, f, n_chan, R, sel=None):
    """the R + 2 counter rows (the counters of a run over the frame's last decode, and `disclosed`) of the frames sel (None = all), f =
    mc_oracle.verdicts of the last decodes"""
    sel = np.arange(close.size) if sel is None else np.asarray(sel)
    rows = []
    for r in list(range(R + 1)) + [-1]:
        idx = sel[close[sel] == r]
        ctr = mc_oracle.tally({k: v[idx] for k, v in f.items()}, n_chan)[0]
        ctr["disclosed"] = int(known[idx].sum())
        rows.append(ctr)
    return rows


def reference(s, kind, qber, first, n, d, R, erased=()):
    """frames [first, first + n) of _Setup s through the round loop -> dict(close, known, f = verdicts of the last decodes, rows), computed
    once per argument set and left unchanged"""
    key = ("blind", kind, qber, first, n, d, R, tuple(int(v) for v in erased))
    if key in s._ref:
        return s._ref[key]
    info_w, flip_w = s.q.mc_frames_host(s.K, s.N, mc_oracle.SEED, qber, first, n, info_bits_pos=s.pos)
    cw = s.codewords(info_w)
    flips = mc_ref.unpack(flip_w, s.N)
    llr = mc_oracle.bsc_llrs(s.q, cw ^ flips, s.cls, qber, erased)
    close, known, last = loop(lambda rows: mc_oracle.oracle(s, kind, rows), llr, cw, s.cls == 0, d, R)
    f = mc_oracle.verdicts(last, cw, s.pos, flips, s.cls == 0)
    n_chan = int((s.cls == 0).sum())
    out = dict(close=close, known=known, f=f, n_chan=n_chan, rows=rows_of(close, known, f, n_chan, R))
    for a in (close, known):
        a.setflags(write=False)
    s._ref[key] = out
    return out


ROW = mc_oracle.COUNTERS + ("disclosed",)


def got_rows(res):
    """the rows of a MonteCarlo.blind result as dicts"""
    return [{k: int(row[k]) for k in ROW} for row in res["rounds"]]


def add_rows(a, b):
    return [{k: (max(x[k], y[k]) if k == "iter_max" else x[k] + y[k]) for k in ROW} for x, y in zip(a, b)]

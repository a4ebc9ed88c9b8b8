"""numpy restatement of the QBER sweep's schedule (include/qldpc.h, "The QBER sweep"), shared by tests/test_mc_sweep.py and
tests/test_mc_sweep_gpu.py.  Nothing here calls the library.

    open       done_q < max_frames and (max_fe == 0 or fe_q < max_fe);  need_q = ceil((max_frames - done_q) / C)
    deal       cycle over the open points in ascending q, one chunk per visit to a point with give_q < need_q, until the S slots are used or a
               whole cycle has given nothing

The deal is stated here in closed form, not as the cycle: after t whole cycles every open point holds min(need_q, t) chunks, so t is the
largest count with sum_q min(need_q, t) <= S, and the slots that are left go, one each, to the lowest open points that still need more.
"""
import numpy as np

CLOSED_MAX_FE, CLOSED_MAX_FRAMES = 1, 2


def needs(done, fe, C, max_frames, max_fe):
    """chunks each point still needs (python ints: max_frames may pass 2^32); 0 for a closed point"""
    return [-(-(int(max_frames) - int(d)) // int(C)) if int(d) < int(max_frames) and (int(max_fe) == 0 or int(e) < int(max_fe)) else 0 for d, e in zip(done, fe)]


def deal(done, fe, C, S, max_frames, max_fe):
    """give[P] (int64) of one round"""
    need = needs(done, fe, C, max_frames, max_fe)
    capped = np.array([min(n, S) for n in need], np.int64)          # no point can receive more than S
    t = 0
    while t < S and int(np.minimum(capped, t + 1).sum()) <= S:
        t += 1
    give = np.minimum(capped, t)
    left = S - int(give.sum())
    for q in np.nonzero(capped > t)[0][:left]:
        give[q] += 1
    return give


def schedule(fail, C, S, max_frames, max_fe):
    """fail[q][k] = does frame k of point q fail (bool [P, >= max_frames]) -> dict(frames[P], frame_errors[P], last_round[P], closed_by[P],
    rounds, gives = the give[] of every round).  Terminates: every round gives at least one chunk, and a chunk has at least one frame."""
    fail = np.asarray(fail, bool)
    P = fail.shape[0]
    done, fe, last = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
    gives = []
    while True:
        give = deal(done, fe, C, S, max_frames, max_fe)
        if give.sum() == 0:
            break
        for q in np.nonzero(give)[0]:
            n = min(int(give[q]) * C, max_frames - int(done[q]))     # only the last chunk of a point is ragged
            fe[q] += int(fail[q, done[q]:done[q] + n].sum())
            done[q] += n
            last[q] = len(gives)
        gives.append(give)
    closed = np.where(done >= max_frames, CLOSED_MAX_FRAMES, CLOSED_MAX_FE)
    return dict(frames=done, frame_errors=fe, last_round=last, closed_by=closed, rounds=len(gives), gives=gives)

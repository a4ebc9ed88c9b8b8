"""The merged form of the syndrome-weight QBER count (csrc/qldpc_qber_core.h, MERGING) restated in Python integers: chain, links, runs, the odd-multiplicity
degree and what is left out.  Test infrastructure: written from the rule's text, not from the library's code; VN states, tables, score and sigma come from
qber_ref."""
import numpy as np

import qber_ref
from qber_ref import ERASED, NOISY

MAX_RUN = 16
MAX_DEGREE = 63
ROWS = MAX_DEGREE + 1


def is_chain(var, chk, N, M):
    """VN K + c on exactly checks c and c + 1 (c < M - 1), VN K + M - 1 on check M - 1 only, K = N - M"""
    K = N - M
    if K < 0:
        return False
    on = {}
    for v, c in zip(var, chk):
        if int(v) >= K:
            on.setdefault(int(v), []).append(int(c))
    return all(sorted(on.get(K + c, [])) == ([c, c + 1] if c < M - 1 else [c]) for c in range(M))


def runs(st, N, M):
    """the runs of a frame as (head, tail) pairs, tail inclusive: maximal sets of consecutive checks joined by erased VNs K + c, c < M - 1"""
    K = N - M
    out, h = [], 0
    for c in range(M):
        if c == M - 1 or st[K + c] != ERASED:
            out.append((h, c))
            h = c + 1
    return out


def counts(var, chk, N, M, bits, vn_class=None, n_channel=None, synd=None, erase=None, known=None, value=None, detail=None):
    """merged counts[64][2] of one frame as Python ints.  detail (a dict) receives what the cases of the tests ask about: the runs, and per run
    why it was left out, its degree and the multiplicities of its noisy VNs"""
    assert is_chain(var, chk, N, M)
    K = N - M
    st, val = qber_ref.states(N, bits, vn_class, n_channel, erase, known, value)
    rows = [[] for _ in range(M)]
    for v, c in zip(var, chk):
        rows[int(c)].append(int(v))
    out = [[0, 0] for _ in range(ROWS)]
    notes = []
    for h, t in runs(st, N, M):
        links = set(range(K + h, K + t))
        u, mult = 0, {}
        for c in range(h, t + 1):
            u ^= 0 if synd is None else int(synd[c])
            for v in rows[c]:
                u ^= int(val[v])
                mult[v] = mult.get(v, 0) + 1
        assert all(mult[v] == 2 for v in links)                      # the links occur twice and cancel
        erased_other = any(st[v] == ERASED for v in mult if v not in links)
        d = sum(1 for v, n in mult.items() if v not in links and st[v] == NOISY and n % 2)
        why = "erased" if erased_other else "long" if t - h + 1 > MAX_RUN else "degree" if d > MAX_DEGREE else None
        notes.append(dict(head=h, tail=t, left_out=why, d=d, mults={n for v, n in mult.items() if v not in links and st[v] == NOISY}))
        if why:
            continue
        out[d][0] += 1
        out[d][1] += u
    if detail is not None:
        detail["runs"] = notes
    return out


def frame_counts(var, chk, N, M, f, i, detail=None):
    """merged counts of frame i of a qber_ref.frames() dict"""
    pick = lambda a: None if a is None else a[i]
    return counts(var, chk, N, M, f["bits"][i], f["cls"], None if f["nch"] is None else f["nch"][i], pick(f["synd"]), pick(f["erase"]), pick(f["known"]),
                  pick(f["value"]), detail)


def host_counts(q, code, f, i):
    """the library's merged host mirror on frame i of a frames() dict"""
    pick = lambda a: None if a is None else q.pack_bits(a[i])
    return q.qber_counts_merged_host(code, q.pack_bits(f["bits"][i]), f["cls"], None if f["nch"] is None else int(f["nch"][i]), pick(f["synd"]),
                                     pick(f["erase"]), pick(f["known"]), pick(f["value"]))


def punct_at(j, p, M):
    """is parity position j punctured when p of M are, evenly spaced (the sessions' rule)"""
    return (j + 1) * p // M > j * p // M


def spaced(N, M, p):
    """erase row [N]: p of the M parity VNs, evenly spaced"""
    e = np.zeros(N, np.uint8)
    e[N - M + np.array([j for j in range(M) if punct_at(j, p, M)], np.int64)] = 1
    return e


PATTERNS = ("spaced25", "spaced50", "spaced60", "random40")
NAMED = ("head0", "last", "known_link", "erased_info", "long", "degree", "repeat")


def repeats(var, chk, N, M):
    """(v3, (a, b, c)), (v2, (a, b)): an information VN on three checks within MAX_RUN of each other, and another one on two neighbouring-ish checks
    inside the same span if there is one, else anywhere (None where the code has none)"""
    K = N - M
    on = {}
    for v, c in zip(var, chk):
        if int(v) < K:
            on.setdefault(int(v), []).append(int(c))
    three = two = None
    for v, cs in sorted(on.items()):
        cs = sorted(cs)
        for i in range(len(cs) - 2):
            if three is None and cs[i + 2] - cs[i] < MAX_RUN:
                three = (v, (cs[i], cs[i + 1], cs[i + 2]))
    for v, cs in sorted(on.items()):
        cs = sorted(cs)
        for i in range(len(cs) - 1):
            if three and v != three[0] and two is None and three[1][0] <= cs[i] and cs[i + 1] <= three[1][2]:
                two = (v, (cs[i], cs[i + 1]))
    return three, two


def overlay(rng, var, chk, N, M, f, named):
    """frames() dict f with an erase pattern laid over frame i: PATTERNS[i], then (named) the constructed cases NAMED, cycling.  Named cases need
    known / value / n_channel rows and add them where f has none.  -> (frames dict, the case name of every frame)"""
    K, F = N - M, f["bits"].shape[0]
    g = dict(f)
    g["erase"] = np.zeros((F, N), np.uint8) if f["erase"] is None else f["erase"].copy()
    if named:
        g["known"] = np.zeros((F, N), np.uint8) if f["known"] is None else f["known"].copy()
        g["value"] = rng.integers(0, 2, (F, N)).astype(np.uint8) if f["value"] is None else f["value"].copy()
        g["nch"] = np.full(F, N, np.int32) if f["nch"] is None else f["nch"].copy()
    rows = [[] for _ in range(M)]
    for v, c in zip(var, chk):
        rows[int(c)].append(int(v))
    cases = PATTERNS + (NAMED if named else ())
    names = []
    for i in range(F):
        name = cases[i % len(cases)]
        names.append(name)
        er = g["erase"][i]
        if name.startswith("spaced"):
            er |= spaced(N, M, M * int(name[6:]) // 100)
        elif name == "random40":
            er[K:] |= (rng.random(M) < 0.4).astype(np.uint8)
        elif name == "head0":                      # a run that starts at check 0
            er[K:K + 2] = 1
        elif name == "last":                       # VN K + M - 1 erased, at the end of a run of two
            er[K + M - 2:] = 1
        elif name == "known_link":                 # three erased links, the middle one known: two runs of two
            er[K + 10:K + 13] = 1
            g["known"][i, K + 11] = 1
        elif name == "erased_info":                # an erased information VN inside a run of two
            er[K + 20] = 1
            er[min(v for v in rows[21] if v < K)] = 1
        elif name == "long":                       # runs of 17, 16 and 31 checks; few noisy VNs, so that the run of 16 stays below degree 64
            er[K + 30:K + 46] = 1
            er[K + 50:K + 65] = 1
            er[K + 100:K + 130] = 1
            g["nch"][i] = 40
        elif name == "degree":                     # four checks, every VN noisy
            er[K + 70:K + 73] = 1
        elif name == "repeat":                     # a VN three times and a VN twice in one run, most other VNs known
            three, two = repeats(var, chk, N, M)
            if three:
                keep = [three[0]] + ([two[0]] if two else [])
                g["known"][i, :K] = (rng.random(K) < 0.9).astype(np.uint8)
                g["known"][i, keep] = 0
                er[keep] = 0
                er[K + three[1][0]:K + three[1][2]] = 1
    return g, names


def session_runs(var, chk, code_k, code_m, n_punct, key_bits):
    """the number of counted runs of a session frame, from its plan and its code's edges alone: parity position j erased iff punct_at(j), key VNs below
    key_bits noisy, everything else exact.  A run counts unless it has more than MAX_RUN checks, ends in an erased last parity VN, or has more than
    MAX_DEGREE noisy VNs of odd multiplicity"""
    rows = [[] for _ in range(code_m)]
    for v, c in zip(var, chk):
        rows[int(c)].append(int(v))
    n, h = 0, 0
    for c in range(code_m):
        if c == code_m - 1 or not punct_at(c, n_punct, code_m):
            mult = {}
            for cc in range(h, c + 1):
                for v in rows[cc]:
                    if v < key_bits:
                        mult[v] = mult.get(v, 0) + 1
            d = sum(m % 2 for m in mult.values())
            if c - h + 1 <= MAX_RUN and d <= MAX_DEGREE and not (c == code_m - 1 and punct_at(c, n_punct, code_m)):
                n += 1
            h = c + 1
    return n

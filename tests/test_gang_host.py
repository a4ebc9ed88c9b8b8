"""Host suite (no GPU) of the decoder gangs (qldpc.h "decoder gangs"): the block -> (member, local block) mapping the gang kernels use
(qldpc_gang_locate_host runs the kernels' own inline function) and the launch plan (qldpc_gang_plan, the planner qldpc_gang_create uses)."""
import itertools
import os

import numpy as np
import pytest

CAPS = (8, 12, 20, 40)


def load(q, gold, name):
    p = os.path.join(gold, name)
    return q.Code.from_qc(p) if name.endswith(".qc") else q.Code.from_alist(p)


def cap_of(deg):
    """a check's cap: the smallest of 8, 12, 20, 40 that holds its degree, else 0"""
    for c in CAPS:
        if deg <= c:
            return c
    return 0


def layer_caps(code):
    """per layer: the set of caps of its checks (one solo launch each)"""
    order, ptr, _ = code.layer_order()
    var, chk = code.edges()
    deg = np.bincount(chk, minlength=code.M)
    return [set(cap_of(int(d)) for d in deg[order[ptr[l]:ptr[l + 1]]]) for l in range(len(ptr) - 1)]


def recount(codes, rules, compressed):
    """what the plan must say, from Code.layer_order(), the degrees of Code.edges() and the cap rule"""
    fam = {"MS": 0, "OMS": 0, "NMS": 0, "SPA": 1, "LSPA": 2}
    per = [layer_caps(c) for c in codes]
    steps = max(len(p) for p in per)
    solo = sum(len(s) for p in per for s in p)
    gang = 0
    for s in range(steps):
        classes = set()
        for i, p in enumerate(per):
            if s < len(p):
                classes |= {(cap, fam.get(rules[i], 3), bool(compressed[i])) for cap in p[s]}
        gang += len(classes)
    return steps, gang, solo


# ---- the block mapping ------------------------------------------------------------------------------------------------------------------

def ragged_prefixes(n):
    """block counts of n members out of {0, 1, 3, 4}: every pattern for n <= 4 (zero-block members at the front, in the middle, at the end,
    several in a row, all of them), and for larger n the patterns with zeros at each of those places"""
    if n <= 4:
        pats = list(itertools.product((0, 1, 3, 4), repeat=n))
    else:
        base = [(k % 4) + 1 for k in range(n)]
        pats = [tuple(base)]
        for zeros in ([0], [n - 1], [n // 2], [0, 1], [n - 2, n - 1], [0, n // 2, n - 1], [1, 2, 3], list(range(n))):
            pats.append(tuple(0 if k in zeros else base[k] for k in range(n)))
        rng = np.random.default_rng(n)
        pats += [tuple(int(x) for x in rng.choice((0, 0, 1, 2, 5, 9), n)) for _ in range(8)]
    return pats


@pytest.mark.parametrize("n", range(1, 9))
def test_gang_locate_maps_every_block_to_the_member_whose_range_holds_it(q, n):
    for counts in ragged_prefixes(n):
        prefix = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        total = int(prefix[-1])
        for block in range(total):
            want = [m for m in range(n) if prefix[m] <= block < prefix[m + 1]]
            assert len(want) == 1
            assert q.gang_locate(prefix, block) == (want[0], block - int(prefix[want[0]])), (counts, block)
        for block in (total, total + 1, total + 1000):
            with pytest.raises(q.QldpcError) as e:
                q.gang_locate(prefix, block)
            assert e.value.status == -1, (counts, block)


def test_gang_locate_refuses_bad_prefixes(q):
    for prefix, block in (([1, 2], 1), ([0, 3, 2], 0), ([0, 1], -1), ([0] + [1] * 9, 0)):
        with pytest.raises(q.QldpcError) as e:
            q.gang_locate(prefix, block)
        assert e.value.status == -1


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["PEGReg504x1008.alist", "NR_1_7_30.qc"])
def test_plan_of_three_copies_of_one_code(q, gold, name):
    code = load(q, gold, name)
    p = q.gang_plan([code] * 3, ["NMS"] * 3, [1, 1, 1])
    assert p["launches_per_sweep"] * 3 == p["solo_launches_per_sweep"]
    assert p["steps"] == len(code.layer_order()[1]) - 1
    assert p == q.gang_plan([code] * 3, ["NMS"] * 3)      # the state changes the class of all three alike


MIX = ["PEGReg504x1008.alist", "NR_1_7_30.qc", "1998.5.3.2665.alist", "20.alist"]


def test_plan_of_mixed_codes(q, gold):
    codes = [load(q, gold, n) for n in MIX]
    caps = [set().union(*layer_caps(c)) for c in codes]
    assert caps == [{8}, {8, 12, 20}, {40}, {8, 12}], caps      # what the mix is chosen for
    rules = ["NMS"] * 4
    p = q.gang_plan(codes, rules, [0] * 4)
    steps, gang, solo = recount(codes, rules, [0] * 4)
    assert p == dict(steps=steps, launches_per_sweep=gang, solo_launches_per_sweep=solo)
    assert steps == max(len(c.layer_order()[1]) - 1 for c in codes)
    assert p["launches_per_sweep"] < p["solo_launches_per_sweep"]

    # compressed state for the three codes of degree <= 32: they no longer share a class with the explicit-message member
    comp = [1, 1, 0, 1]
    pc = q.gang_plan(codes, rules, comp)
    assert pc == dict(zip(("steps", "launches_per_sweep", "solo_launches_per_sweep"), recount(codes, rules, comp)))
    assert pc["launches_per_sweep"] < pc["solo_launches_per_sweep"]
    # one member alone in the compressed state: cap-8 checks of the first and the last code now fall into different classes
    p1 = q.gang_plan(codes, rules, [1, 0, 0, 0])
    assert p1 == dict(zip(("steps", "launches_per_sweep", "solo_launches_per_sweep"), recount(codes, rules, [1, 0, 0, 0])))
    assert p1["launches_per_sweep"] > p["launches_per_sweep"]

    # two rule families: the classes split by family
    rules2 = ["NMS", "SPA", "NMS", "SPA"]
    p2 = q.gang_plan(codes, rules2, [0] * 4)
    assert p2 == dict(zip(("steps", "launches_per_sweep", "solo_launches_per_sweep"), recount(codes, rules2, [0] * 4)))
    assert p["launches_per_sweep"] < p2["launches_per_sweep"] <= p2["solo_launches_per_sweep"]
    assert p2["solo_launches_per_sweep"] == p["solo_launches_per_sweep"]
    # members of one family (MS / OMS / NMS) share their launches
    assert q.gang_plan(codes, ["MS", "OMS", "NMS", "MS"], [0] * 4) == p


def test_plan_refusals(q, gold):
    code = load(q, gold, "1998.5.3.2665.alist")      # degree 36
    peg = load(q, gold, "PEGReg504x1008.alist")
    for args in (([code], ["NMS"], [1]), ([peg], ["SPA"], [1]), ([], [], None), ([peg] * 33, ["NMS"] * 33, None)):
        with pytest.raises(q.QldpcError) as e:
            q.gang_plan(*args)
        assert e.value.status == -1

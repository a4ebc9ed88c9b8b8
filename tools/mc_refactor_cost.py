#!/usr/bin/env python3
"""Same outputs and same speed of two builds of libqldpc.so over the Monte-Carlo cost tools (mc_cost.py --leg split, mc_search_cost.py,
mc_sweep_cost.py, mc_strata_cost.py at their default headline shapes).  Run every tool twice per build, alternating, one process each, the
other build selected with QLDPC_LIB, every run with its own --out:

    for run in 1 2; do for build in parent head; do            # parent: QLDPC_LIB=<the other library>
        timeout -k 10 600 python tools/mc_cost.py --leg split --out profiles/mc_refactor_cost/cost_${build}${run}.json && ... search, sweep, strata
    done; done
    python tools/mc_refactor_cost.py profiles/mc_refactor_cost

Then this tool (no device) reads the 16 files and writes summary.json beside them:
integers: every integer both builds print (frames, frame errors, rows, rounds) must be equal in all four runs of a tool.
times:    per quantity -- the per-round hipEvent time of a stage the Monte-Carlo kernels own, and the whole call per round -- the four numbers
          and the verdict: mean(head) - mean(parent) <= |parent1 - parent2|, the parent's own spread.  The kernels are about 1 % of a round
          beside the decode, so total_ms cannot resolve them; the stage times are the measurement.
"""
import json
import os
import sys

BATCH = 4096


def integers(x, pre=""):
    """every integer (and list of integers) of a result, by its path"""
    if isinstance(x, dict):
        return {k: v for key in sorted(x) for k, v in integers(x[key], pre + "." + key).items()}
    if isinstance(x, bool) or not (isinstance(x, int) or (isinstance(x, list) and all(isinstance(v, int) for v in x))):
        return {}
    return {pre[1:]: x}


def stages(d, keys):
    return {k: d[k + "_ms"] for k in keys}


def times(tool, r):
    """the quantities of one run: name -> ms per round"""
    if tool == "cost":
        s = r["split"]
        return dict(stages(s["per_batch_ms"], ("source", "channel", "monitor")), total=BATCH * 1e3 / s["frames_per_s"])
    if tool == "search":
        out = dict(stages(r["search"]["per_round_ms"], ("pattern", "expand", "generate", "monitor")), total=BATCH * 1e3 / r["search"]["frames_per_s"])
        out.update({"run_" + k: v for k, v in stages(r["run"]["per_batch_ms"], ("source", "channel", "monitor")).items()})
        return out
    legs = ("sweep",) if tool == "sweep" else ("strata", "sweep")
    out = {}
    for leg in legs:
        pre = leg + "_" if len(legs) > 1 else ""
        out.update({pre + k: v for k, v in stages(r[leg]["per_round_ms"], ("source", "channel", "erase", "monitor")).items()})
        out[pre + "total"] = r[leg]["total_ms"] / r[leg]["rounds"]
    return out


def main():
    where = sys.argv[1]
    summary, ok = {}, True
    for tool in ("cost", "search", "sweep", "strata"):
        runs = {b + n: json.load(open(os.path.join(where, "%s_%s%s.json" % (tool, b, n)))) for b in ("parent", "head") for n in "12"}
        ints = {k: integers(r) for k, r in runs.items()}
        same = all(ints[k] == ints["parent1"] for k in ints)
        t = {k: times(tool, r) for k, r in runs.items()}
        quantities = {}
        for name in t["parent1"]:
            p1, p2, h1, h2 = (t[k][name] for k in ("parent1", "parent2", "head1", "head2"))
            excess, spread = (h1 + h2) / 2 - (p1 + p2) / 2, abs(p1 - p2)
            quantities[name] = dict(parent_ms=[p1, p2], head_ms=[h1, h2], head_minus_parent_ms=excess, parent_spread_ms=spread, within=excess <= spread)
        summary[tool] = dict(integers_equal=same, integers=ints["parent1"] if same else ints, per_round=quantities)
        ok = ok and same
    summary["what"] = ("two builds of libqldpc.so over the Monte-Carlo cost tools, two alternating runs each: the integers all four runs print, and per stage "
                       "time the four numbers; within = mean(head) - mean(parent) <= |parent1 - parent2|")
    summary["all_integers_equal"] = ok
    summary["quantities_outside_the_parents_spread"] = sorted(t + "." + n for t in summary if isinstance(summary[t], dict) and "per_round" in summary[t]
                                                                 for n, v in summary[t]["per_round"].items() if not v["within"])
    with open(os.path.join(where, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: summary[k] for k in ("all_integers_equal", "quantities_outside_the_parents_spread")}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())

"""bench.py keeps its contract: one JSON line with the driver's keys plus `roofline` and, with --full, `cpu_baseline` and the other legs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "256", "--n", "8192", "--k", "6554",
                        "--n-ite", "12", "--fer-frames", "8192", "--full"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == "reconciled_key_Mbit_s" and d["unit"] == "Mbit/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["achieved"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and c["gpu_matches_oracle_on_sample"] is True
    assert d["value"] > 0 and d["fer"] < 0.5
    assert d["int8_messages"]["fixed"]["value"] > 0 and d["fp16_messages"]["fixed"]["value"] > 0
    assert "parity unpinned against AFF3CT" in d["parity_note"]
    assert d["spa_rule"]["fixed"]["value"] > 0 and d["spa_rule"]["early_exit"]["value"] > 0      # "NMS and SPA"


@pytest.mark.gpu
def test_default_bench_line_covers_configs_2_3_5_and_every_moved_frac_is_at_most_one():
    """one default run puts BASELINE configs 2 (the line itself), 3 and 5 in front of the driver, each with its own roofline,
    moved bytes beside algorithmic bytes, and no fraction above 1 (round 1's layered mode summed one pass three times)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu", "--full"], capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.strip()][-1])
    assert "configs[1]" in d["config"]["workload"] and d["config"]["frames_per_gpu"] == 4096
    r = d["roofline"]
    assert r["traffic"] is not None and 0.95 < r["traffic"] / r["alg_bytes_per_launch"] < 1.1      # PMC traffic of the check pass ~ its algorithmic bytes
    cp = r["copy_probe"]      # the device's own copy rate, measured in the same run: the check pass runs at (nearly) all of it
    assert 4000 < cp["rows_256B_GBs"] < 8000 and 4000 < cp["wide_16B_per_lane_GBs"] < 8000 and 0.85 < cp["frac_of_copy"] < 1.15
    fracs = [r["frac"], r["vn_update"]["frac"], r["vn_update"]["moved_frac"], r["whole_step"]["frac"], r["whole_step"]["moved_frac"]]
    assert r["vn_update"]["moved_bytes_per_pass"] < r["vn_update"]["alg_bytes_per_pass"]              # coded LLRs: fewer bytes than SURVEY 8d prices
    e = d["early_exit"]
    assert e["compactions"] >= 1 and 0.9 < e["useful_work"] <= 1.0 and e["value"] > 2.5 * d["value"]
    c3, c5 = d["config3_multirate_stream"], d["config5_layered_1e6"]
    assert c3["value"] > 0 and c3["fer"] <= 0.01 and 0.25 < c3["leaked_fraction"] < 0.33 and sum(c3["epochs_per_rate"].values()) == 512
    assert c5["early_exit"]["value"] > c5["fixed"]["value"] > 0 and c5["early_exit"]["avg_sweeps"] < 10 and c5["fixed"]["fer"] == 0.0
    assert c3["undetected_errors"] == 0 and 0.0 < c3["wall_frac"] <= 1.0 and c3["value"] > 1200
    # the FER half of the metric: >= 2^20 frames at the headline QBER with undetected errors counted, plus the waterfall
    fd = d["fer_deep"]
    h = fd["headline_qber"]
    assert h["frames"] >= 1 << 20 and h["qber"] == 0.02 and h["undetected_errors"] == 0 and h["frame_errors"] <= 2
    assert 0.0 < h["fer_upper_95"] < 1e-5 and 9 < h["avg_iterations"] < 14 and h["max_iterations"] <= 50
    hl = fd["layered_schedule"]      # the same frames through the layered sweeps: no worse than flooding, half the iterations
    assert hl[0]["frames"] >= 1 << 20 and hl[0]["frame_errors"] <= 2 and hl[0]["undetected_errors"] == 0 and hl[0]["avg_iterations"] < 0.6 * h["avg_iterations"]
    assert all(p_["undetected_errors"] == 0 for p_ in hl)
    wf = fd["waterfall_seeded_shuffle"]
    assert len(wf) == 8 and all(p_["frames"] == 65536 and p_["undetected_errors"] == 0 for p_ in wf)
    assert wf[0]["fer"] < 0.01 < wf[3]["fer"]              # NMS: clean at 2.5 %, inside the waterfall at 3.25 %
    assert wf[4]["fer"] < wf[0]["fer"] + 1e-3 and wf[7]["fer"] < wf[3]["fer"]      # SPA is the better rule at every point
    # round 3: min-sum layered sweeps run on the compressed check state -- fewer bytes moved than section 8(d) prices, same words
    assert c5["fixed"]["roofline"]["moved_bytes_per_sweep"] < 0.7 * c5["fixed"]["roofline"]["alg_bytes_per_sweep"] and "compressed" in c5["fixed"]["roofline"]["kernel"]
    ls = d["layered_schedule"]      # the headline code and batch on AFF3CT's other schedule
    assert ls["fixed"]["fer"] == 0.0 and ls["early_exit"]["fer"] == 0.0 and ls["fixed"]["value"] > d["value"] and ls["early_exit"]["value"] > e["value"] and ls["early_exit"]["avg_sweeps"] < 8
    # (config 5's frac prices section 8(d)'s 4 E rows per sweep against a kernel that moves 0.61 of them: it sits at 0.93 - 0.97 and may pass 1 on a fast box; what is bounded by 1 is the moved share)
    assert 0.5 < c5["fixed"]["roofline"]["frac"] < 1.0 / 0.6 and abs(c5["fixed"]["roofline"]["moved_frac"] / c5["fixed"]["roofline"]["frac"] - c5["fixed"]["roofline"]["moved_bytes_per_sweep"] / c5["fixed"]["roofline"]["alg_bytes_per_sweep"]) < 1e-6
    fracs += [c3["roofline"]["frac"], c5["fixed"]["roofline"]["moved_frac"], c5["early_exit"]["roofline"]["moved_frac"], ls["fixed"]["roofline_moved_frac"]]
    sp = d["spa_rule"]      # SURVEY 8(d) config 2 names SPA beside NMS (the harness default): same code and batch, tolerance class
    assert sp["fixed"]["fer"] == 0.0 and sp["early_exit"]["fer"] == 0.0 and sp["early_exit"]["avg_iterations"] < e["avg_iterations"] and sp["fixed"]["value"] > 0.6 * d["value"]
    fracs += [sp["fixed"]["cn_update_frac"]]
    assert all(0.0 < f <= 1.0 for f in fracs), fracs


@pytest.mark.gpu
def test_plain_bench_times_the_headline_only_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain run times exactly --steps steps of the headline and nothing else; --dump-outputs writes the last timed step (float32 /
    float64 .npy, at most 64 MB), and two runs with the same arguments write the same arrays."""
    import numpy as np
    dumps = []
    for run in range(2):
        d_out = tmp_path / ("run%d" % run)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--frames", "256", "--n", "8192", "--k", "6554",
                            "--n-ite", "12", "--dump-outputs", str(d_out)], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["metric"] == "reconciled_key_Mbit_s" and d["unit"] == "Mbit/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0 and d["fer"] < 0.5
        assert d["roofline"]["launches"] % 3 == 0 and d["iterations_executed"] == 12 and d["roofline"]["copy_probe"] is None      # no probe run
        for leg in ("cpu_baseline", "early_exit", "layered_schedule", "fp16_messages", "int8_messages", "spa_rule", "fer_deep",
                    "config3_multirate_stream", "config5_layered_1e6"):
            assert d[leg] is None, leg
        files = sorted(f.name for f in d_out.iterdir())
        assert files == sorted(n + ".npy" for n in ("decoded_bits", "decoded_frame_index", "decoded_ones", "frame_iterations", "frame_syndrome_ok", "frame_reconciled"))
        assert sum(f.stat().st_size for f in d_out.iterdir()) <= 64 << 20
        a = {f[:-4]: np.load(d_out / f) for f in files}
        assert all(v.dtype in (np.float32, np.float64) for v in a.values())
        assert a["decoded_bits"].shape == (128, 8192) and set(np.unique(a["decoded_bits"])) <= {0.0, 1.0}
        assert a["decoded_ones"].shape == a["frame_reconciled"].shape == (256,)
        assert (a["frame_iterations"] <= 12).all() and abs(a["frame_reconciled"].mean() - (1.0 - d["fer"])) < 1e-9
        dumps.append(a)
    for k in dumps[0]:
        assert (dumps[0][k] == dumps[1][k]).all(), k

"""What the cost tools of the polar subsystem (polar_cost.py, polar_wide_cost.py, polar_list_cost.py) share: the hipEvent timing of a call and the
frames they decode."""
import numpy as np


def event_ms(torch, fn, runs):
    """hipEvent ms of fn() on the current stream, `runs` times after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"median": float(np.median(out)), "best": float(min(out)), "worst": float(max(out)), "runs": [round(v, 4) for v in out]}


def awgn_frames(rng, n, F, messages):
    """F frames of the all-zero word of a code of 2^n bits on AWGN (noise 0.7 on +1): int8 levels in -32 .. 31, or float LLRs -> [F, N]"""
    noise = 1.0 + 0.7 * rng.standard_normal((F, 1 << n), dtype=np.float32)
    return np.clip(np.floor(noise * 7.75), -32, 31).astype(np.int8) if messages == "i8" else (2.0 * noise / 0.49).astype(np.float32)

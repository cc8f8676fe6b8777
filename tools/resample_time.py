"""Times of the device resampler (resample.Resampler, vqa_resample) and of the host path, and the kernel's error
against the fp64 reference as a share of the derived bound (tests/test_gpu_resample.py):
  - one 30 s track of 22050 Hz and a batch of 16, int16, 22050 -> 3000, "best" and "fast";
  - 3000 -> 22050 of the results' length;
  - 22050 -> 16001 (tap table in global memory);
  - resample.resample_reference (numpy fp64, the path of data_utils.load_audio) on one track.
Every call runs between two device events after a warm-up of its shape; the median of REPS alternating repeats is
reported with the rate 2 P flops per output reaches. Shares are of 157.3 TFLOP/s, the device's fp32 vector peak with
packed instructions; the library is built without them, so a plain fused multiply-add stream tops out at half.
    python tools/resample_time.py [profiles/resample.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]
import resample as RS  # noqa: E402
import vqa_lib as V  # noqa: E402

REPS, PEAK = 20, 157.3e12
DEV = "cuda:0"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def error_ratios(lines):
    cases = [(22050, 3000, "best"), (22050, 3000, "fast"), (3000, 22050, "best"), (44100, 22050, "best"),
             (48000, 44100, "best"), (22050, 16001, "best"), (2, 3, "best")]
    lines.append("error against resample_reference as a share of (P + 2) 2^-24 max_r sum|T[r]| max|x|, worst over "
                 "n = 4099, 611, 5, 1 and 3 rows")
    worst_all = 0.0
    for case in cases:
        plan = RS.design(*case)
        bound = (plan.P + 2) * 2.0 ** -24 * plan.abs_row_sum()
        taps = plan.device_table(DEV)
        lds, tile = V.resample_route(plan.up, plan.down, plan.P)
        for kind in ("int16", "fp32"):
            worst = 0.0
            for n in (4099, 611, 5, 1):
                rng = np.random.default_rng(1000 + n)
                if kind == "int16":
                    a = rng.integers(-32768, 32768, (3, n)).astype(np.int16)
                    v = a.astype(np.float64) / 32768.0
                else:
                    a = rng.uniform(-1.0, 1.0, (3, n)).astype(np.float32)
                    v = a.astype(np.float64)
                out = torch.empty(3, plan.output_length(n), dtype=torch.float32, device=DEV)
                V.resample(torch.from_numpy(a).to(DEV), out, taps, plan.up, plan.down)
                err = np.abs(out.cpu().numpy().astype(np.float64) - RS.resample_reference(v, plan)).max()
                worst = max(worst, float(err) / bound)
            worst_all = max(worst_all, worst)
            lines.append(f"  {case[0]:>5} -> {case[1]:<5} {case[2]:<4} {kind:<5} P {plan.P:>3} "
                         f"{'lds' if lds else 'global':<6} tile {tile:>3}  bound {bound:.3g}  worst ratio {worst:.4f}")
    lines.append(f"  worst ratio of all cases: {worst_all:.4f}")


def main():
    assert torch.cuda.is_available(), "resample_time.py measures on the GPU"
    lines = [f"tools/resample_time.py on {torch.cuda.get_device_name(0)}: median of {REPS} repeats, device events"]
    error_ratios(lines)
    n = 30 * 22050
    rng = np.random.default_rng(7)
    track = rng.integers(-32768, 32768, (16, n)).astype(np.int16)
    x16 = torch.from_numpy(track).to(DEV)
    runs = {}
    for q in ("best", "fast"):
        rs = RS.Resampler(22050, 3000, q, DEV)
        for rows in (1, 16):
            x = x16[:rows].contiguous()
            out = torch.empty(rows, rs.plan.output_length(n), dtype=torch.float32, device=DEV)
            runs[f"22050 -> 3000  {q} int16 B={rows}"] = (rs, x, out)
    back = RS.Resampler(3000, 22050, "best", DEV)
    far = RS.Resampler(22050, 16001, "best", DEV)
    low = torch.empty(16, 90000, dtype=torch.float32, device=DEV).uniform_(-1, 1)
    for rows in (1, 16):
        x = low[:rows].contiguous()
        runs[f"3000  -> 22050 best fp32  B={rows}"] = (back, x, torch.empty(rows, back.plan.output_length(90000),
                                                                          dtype=torch.float32, device=DEV))
    runs["22050 -> 16001 best int16 B=1"] = (far, x16[:1].contiguous(),
                                              torch.empty(1, far.plan.output_length(n), dtype=torch.float32,
                                                          device=DEV))
    for rs, x, out in runs.values():
        rs(x, out=out)
    ms = {k: [] for k in runs}
    for _ in range(REPS):
        for k, (rs, x, out) in runs.items():
            ms[k].append(timed(lambda: rs(x, out=out)))
    lines.append("device: one vqa_resample launch per call (30 s tracks of 22050 Hz; 90,000 samples of 3000 Hz)")
    for k, (rs, x, out) in runs.items():
        t = sorted(ms[k])
        med = t[len(t) // 2]
        flops = 2.0 * rs.plan.P * out.numel()
        rate = flops / (med * 1e-3)
        lines.append(f"  {k:<32} P {rs.plan.P:>3}  median {med:8.4f} ms (min {t[0]:.4f}, max {t[-1]:.4f})  "
                     f"{rate / 1e12:7.3f} TFLOP/s = {100 * rate / PEAK:5.2f} % of {PEAK / 1e12:.1f}")
    lines.append("host: resample.resample_reference (numpy fp64), one 30 s track, wall clock, best of 3")
    for q in ("best", "fast"):
        plan = RS.design(22050, 3000, q)
        v = track[0].astype(np.float64) / 32768.0
        best = min(_wall(lambda: RS.resample_reference(v, plan)) for _ in range(3))
        lines.append(f"  22050 -> 3000  {q}: {best * 1e3:9.1f} ms")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


def _wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


if __name__ == "__main__":
    main()

"""Time the optimizer launches of one step with and without the weights' moving average.

    python tools/ema_time.py [cfg2|cfg4|both] [applies] [repeats]

cfg2: the benched VQ-VAE's store (968,835 parameters). cfg4: the config-4 prior's (SMALL_PRIOR, ctx 8192). Three
variants, in this one process and on the same buffers (weights, gradient, moments; the weights are restored before
each variant):
  plain     Adam.apply without an average (adam_stride_kernel<false> + the step counter's increment)
  fused     Adam.apply with average_decay (adam_stride_kernel<true> + the increment): the average in the Adam launch
  unfused   the plain apply followed by a separate averaging pass written with torch ops on the flat buffers,
            a.sub_((a - w) * (1 - d)): what user code outside the library would run
Every variant is warmed up, then timed `repeats` times over `applies` eager applies between two device events;
the variants take turns within a repeat, so drift of the device meets all three alike. Printed: the median and the
range over the repeats, in microseconds per apply.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]

import torch  # noqa: E402

from clip_time import store_of  # noqa: E402
from vqa_optim import Adam  # noqa: E402

DECAY = 0.999


def timed(fn, applies):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(applies):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / applies * 1e3


def run(which, applies, repeats):
    st = store_of(which)
    g = torch.Generator(device="cuda").manual_seed(5)
    st.grad[:st.size].copy_(torch.randn(st.size, device="cuda", generator=g) * 1e-2)
    print(f"{which}: {st.count} parameters, {st.size} floats ({st.size * 4 / 1e6:.2f} MB per buffer)")
    plain, fused, base = Adam(1e-4), Adam(1e-4, average_decay=DECAY), Adam(1e-4)
    for opt in (plain, fused, base):
        opt.build(st)
    side = st.flat.clone()   # the unfused alternative's average
    omd = 1.0 - DECAY

    def unfused():
        base.apply(st)
        side.sub_((side - st.flat) * omd)

    variants = [("plain", lambda: plain.apply(st)), ("fused", lambda: fused.apply(st)), ("unfused", unfused)]
    for _, fn in variants:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(timed(fn, applies))
    for name, _ in variants:
        t = times[name]
        print(f"  {name:8s} median {statistics.median(t):7.1f} us / apply   range {min(t):7.1f} .. {max(t):7.1f} "
              f"({repeats} repeats of {applies} eager applies)")
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"  fused - plain {med['fused'] - med['plain']:+.1f} us, unfused - plain {med['unfused'] - med['plain']:+.1f} us, "
          f"fused / unfused {med['fused'] / med['unfused']:.3f}")


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    applies = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    for w in (("cfg2", "cfg4") if which == "both" else (which,)):
        run(w, applies, repeats)


if __name__ == "__main__":
    main()

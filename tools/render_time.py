"""VQVAE.render / decode_chunked against decode_level at BASELINE config 2, level 0 ("Codes to audio"):
B = 16 items of 65,536 random codes, bf16. Every call runs between two device events on an idle stream, every shape
is warmed first, the calls alternate, and the peak of allocated device memory over each call is recorded.
    python tools/render_time.py [out.json]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]
from vqvae import VQVAE  # noqa: E402

CFG2 = dict(levels=3, latent_dim=64, down_depth=[3, 2, 2], strides=[2, 2, 2], num_embeddings=2048,
            residual_width=32, residual_depth=4, dilation_factor=3)
B, CODES, REPS = 16, 65536, 10


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return a.elapsed_time(b), peak


def main():
    m = VQVAE((65536, 1), dtype="bf16", device="cuda:0", **CFG2)
    zq = torch.randint(0, 2048, (B, CODES), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(5))
    out = {"B": B, "codes": CODES, "halo": [m.decode_halo(l) for l in range(3)], "hops": m.decode_hops}
    runs = {"decode_level": lambda: m.decode_level(zq, 0),
            "render_4096": lambda: m.render(zq, 0, chunk_codes=4096),
            "render_16384": lambda: m.render(zq, 0, chunk_codes=16384),
            "render_1024": lambda: m.render(zq, 0, chunk_codes=1024),
            "decode_chunked_4096": lambda: m.decode_chunked(zq, 0, chunk_codes=4096)}
    for fn in runs.values():
        timed(fn)
    res = {k: [] for k in runs}
    for _ in range(REPS):
        for k, fn in runs.items():
            res[k].append(timed(fn))
    for k, v in res.items():
        ms = sorted(t for t, _ in v)
        out[k] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1],
                  "peak_MiB": max(p for _, p in v) / 2 ** 20}
    out["chunked_equals_whole"] = bool(torch.equal(m.decode_chunked(zq, 0), m.decode_level(zq, 0)))
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

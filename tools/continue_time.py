"""What continuing a recording costs ("Continue a recording"), three measurements on one GPU:
  render    VQVAE.render without a prompt at BASELINE config 2, level 0, bf16, B = 4 items of 65,536 codes: the path
            every earlier caller takes. Run it on two builds (--pkg) alternately to see that it did not move.
  splice    vqa_pcm_splice against vqa_pcm_encode at the same n (B = 16 rows of 2^22 samples): a launch wholly before
            the fade (copies p), wholly past the seam (encodes x), wholly inside the fade (reads both), and the encode.
  continue  continue_audio against sample_audio for the same piece: config 2's VQ-VAE with 1024 codes (the decode
            kernel takes at most 2048 bins, the start token included), priors of 256 / 64 / 16 codes, 4 items, 64
            top-level codes, half of them the prompt.
Every call runs between two device events on an idle stream, every shape is warmed first and the calls alternate.
    python tools/continue_time.py [--pkg DIR] [--only render|splice|continue] [out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--pkg", default=os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"))
ap.add_argument("--only", choices=["render", "splice", "continue"])
ap.add_argument("out", nargs="?")
ARGS = ap.parse_args()
sys.path[:0] = [ARGS.pkg, ROOT]

import torch  # noqa: E402

CFG2 = dict(levels=3, latent_dim=64, down_depth=[3, 2, 2], strides=[2, 2, 2], num_embeddings=2048,
            residual_width=32, residual_depth=4, dilation_factor=3)


def timed(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    del r
    return a.elapsed_time(b)


def alternate(runs, reps):
    for fn in runs.values():
        timed(fn)
    res = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            res[k].append(timed(fn))
    out = {}
    for k, v in res.items():
        ms = sorted(v)
        out[k] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "reps": reps}
    return out


def render():
    from vqvae import VQVAE
    m = VQVAE((65536, 1), dtype="bf16", device="cuda:0", **CFG2)
    zq = torch.randint(0, 2048, (4, 65536), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(5))
    return alternate({"render_4096": lambda: m.render(zq, 0, chunk_codes=4096),
                      "render_16384": lambda: m.render(zq, 0, chunk_codes=16384)}, 12)


def splice():
    import vqa_lib as V
    B, n = 16, 1 << 22
    g = torch.Generator("cuda:0").manual_seed(6)
    x = torch.rand(B, n, device="cuda:0", generator=g) * 2 - 1
    p = torch.rand(B, n, device="cuda:0", generator=g) * 2 - 1
    out = torch.empty(B, n, dtype=torch.int16, device="cuda:0")
    clipped = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    res = alternate({"pcm_encode": lambda: V.pcm_encode(x, out, clipped=clipped),
                     "splice_pure_x": lambda: V.pcm_splice(x, p, out, 0, 0, clipped=clipped),
                     "splice_pure_p": lambda: V.pcm_splice(x, p, out, n, 0, clipped=clipped),
                     "splice_all_fade": lambda: V.pcm_splice(x, p, out, n, n, clipped=clipped)}, 30)
    res["bytes"] = {"pcm_encode": B * n * 6, "splice_pure_x": B * n * 6, "splice_pure_p": B * n * 6,
                    "splice_all_fade": B * n * 10}
    return res


def cont():
    from sampler import VQVAESampler
    from vqvae import VQVAE
    m = VQVAE((65536, 1), dtype="bf16", device="cuda:0", **{**CFG2, "num_embeddings": 1024})
    s = VQVAESampler([3, 2, 2], [2, 2, 2], [256, 64, 16], codebook_size=1025, dtype="fp32", device="cuda", seed=4)
    for pr in s.priors:  # as in a trained model, the start token is never drawn
        pr.prior.store.view(pr.prior.out_bias)[-1] = -1e4
    n, total, hop_top = 4, 64, 128
    audio = torch.rand(n, total // 2 * hop_top, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(7))
    audio = audio * 0.5 - 0.25
    return alternate({"sample_audio": lambda: s.sample_audio(n, m, seed=9, total_length=total),
                      "continue_audio": lambda: s.continue_audio(audio, m, seed=9, total_length=total,
                                                                 fade_samples=256),
                      "sample": lambda: s.sample(n, seed=9, total_length=total)}, 5)


def main():
    parts = {"render": render, "splice": splice, "continue": cont}
    out = {"pkg": ARGS.pkg}
    for k, fn in parts.items():
        if ARGS.only in (None, k):
            out[k] = fn()
    print(json.dumps(out))
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

"""Prior measurements (BASELINE configs 4 and 5) on one MI355X: prints one JSON line per workload.

  train : SMALL_PRIOR (width 128, depth 6, heads 2, blocks 4, row/col/prev-row, bins 2048) Prior.train_step over
          ctx = 8192 top-level codes, bf16 activations, the whole step (two teacher-forcing passes, backward, Adam)
          replayed from a hipGraph; tokens/s = B * ctx * steps / seconds.
  sample: SMALL_UPSAMPLER-style ancestral decode (the same transformer conditioned on upper-level codes through
          ConditionerNet) — one persistent decode launch for N samples x L positions; tokens/s.
Synthetic codes (uniform over the codebook), random-init weights. The cpu leg times the oracle's train step
(oracle/prior_ref.py, torch CPU fp32) on a bounded sample.
    python tools/bench_prior.py [--batch 8] [--steps 10] [--samples 16] [--sample-len 2048] [--no-cpu]
The sample leg takes the primed decode's options: --prime-len P (the first P positions are given, random codes;
P = --sample-len times the primed positions alone, head skipped), --temperature, --top-k, --top-p, and --repeats R
(R timed launches in one process; ms_per_position is their median, ms_per_position_repeats lists them).
  feed  : (--only feed; never part of the default run) the config-4 train step fed three ways, in one process:
          (a) captured, codes copied in (the `train` leg's step), (b) captured on a code_feed.CodeFeed over a
          device-resident corpus of random codes (--tracks tracks of 4 ctx codes, windows hopping by ctx / 2),
          (c) eager from raw audio through the frozen VQ-VAE encoder (config 2's level 2, window ctx * 128 samples;
          --audio-ctx for a shorter window), with the eager step on codes beside it. (a) and (b) alternate for
          --repeats rounds of --steps steps, each round between two device events after a synchronize; the JSON
          line holds every round, the median and the range.
  feed-kernel : (--only feed-kernel) --steps CodeFeed.next() calls at that shape and nothing else, for a
          `rocprofv3 --kernel-trace --stats` run of its own.
  encode-mem  : (--only encode-mem) peak torch.cuda.max_memory_allocated of encode_level and of encode_chunked
          for one item of 2^20 samples at level 0 of config 2.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vae-based-music--deep-generative-models_amd"), ROOT]

import torch  # noqa: E402


def _code_feed(a, dev):
    """A one-level corpus of random codes (the top level: unconditioned) and its feed at the config-4 shape."""
    import numpy as np
    from code_feed import CodeCorpus, CodeFeed
    rng = np.random.default_rng(1)
    tracks = [rng.integers(0, a.bins - 1, 4 * a.ctx) for _ in range(a.tracks)]
    corpus = CodeCorpus.from_codes([tracks], None, [128], a.bins - 1, device=dev)
    return CodeFeed(corpus, 0, n_ctx=a.ctx, batch_size=a.batch, hop=a.ctx // 2, seed=1)


def _rounds(fn, steps, rounds):
    """ms/step of `rounds` rounds of `steps` calls, each between two device events on an idle stream."""
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return out


def _stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 4), "min": round(s[0], 4), "max": round(s[-1], 4),
            "rounds": [round(x, 4) for x in v]}


def feed_mode(a):
    from prior import Prior
    from vqvae import VQVAE
    kw = dict(width=128, depth=6, heads=2, blocks=4, attn_stacks=1, drop_out_rate=0.0)
    dev = torch.device("cuda:0")

    def prior(vq=None, ctx=a.ctx):
        return Prior(2, [(ctx * 16,), (ctx * 4,), (ctx,)], a.bins, [3, 2, 2], [2, 2, 2], vq, kw, None, dtype=a.dtype,
                     device="cuda")

    g = torch.Generator(device=dev).manual_seed(1)
    codes = torch.randint(0, a.bins - 1, (a.batch, a.ctx), device=dev, generator=g)
    pa, pb = prior(), prior()
    feed = _code_feed(a, dev)
    pa.capture_train_step(codes, warmup=a.warmup)
    pb.capture_train_step(feed, warmup=a.warmup)
    for _ in range(3):  # the first replays upload the graphs
        pa.train_step(codes)
        pb.train_step(feed)
    ra, rb = [], []
    for _ in range(max(1, a.repeats)):  # alternating, so that drift of the device's state falls on both
        ra += _rounds(lambda: pa.train_step(codes), a.steps, 1)
        rb += _rounds(lambda: pb.train_step(feed), a.steps, 1)
    out = {"metric": "ms/step prior train step by feed (SMALL_PRIOR, config 4)", "unit": "ms/step", "n_gpus": 1,
           "batch": a.batch, "ctx": a.ctx, "bins": a.bins, "dtype": a.dtype, "steps_per_round": a.steps,
           "windows": len(feed.starts_host), "feed_step": feed.step,
           "a_captured_codes_copied_in": _stats(ra), "b_captured_code_feed": _stats(rb)}
    del pa, pb
    torch.cuda.empty_cache()
    # eager legs: from codes, and from raw audio through the frozen encoder (level 2 of config 2)
    actx = a.audio_ctx or a.ctx
    T = actx * 128
    vq = VQVAE((T, 1), 3, 64, [3, 2, 2], [2, 2, 2], num_embeddings=a.bins - 1, residual_width=64, residual_depth=4,
               dilation_factor=3, dtype=a.dtype, device="cuda")
    pc = prior(vq, actx)
    x = torch.rand(a.batch, T, 1, device=dev, generator=g) * 2 - 1
    ec = codes[:, :actx].contiguous()
    n = max(2, a.steps // 2)
    for _ in range(2):
        pc.train_step(ec)
        pc.train_step(x)
    out["audio_ctx"] = actx
    out["eager_codes"] = _stats(_rounds(lambda: pc.train_step(ec), n, max(1, a.repeats)))
    out["c_eager_raw_audio"] = _stats(_rounds(lambda: pc.train_step(x), n, max(1, a.repeats)))
    out["c_over_b"] = round(out["c_eager_raw_audio"]["median"] / out["b_captured_code_feed"]["median"], 3)
    print(json.dumps(out), flush=True)


def feed_kernel_mode(a):
    dev = torch.device("cuda:0")
    feed = _code_feed(a, dev)
    for _ in range(a.steps):
        feed.next()
    torch.cuda.synchronize()
    print(json.dumps({"mode": "feed-kernel", "launches": a.steps, "batch": a.batch, "ctx": a.ctx,
                      "bytes_per_launch": a.batch * a.ctx * (8 + feed.corpus.codes[0].element_size()),
                      "step": feed.step}), flush=True)


def encode_mem_mode(a):
    from vqvae import VQVAE
    dev = torch.device("cuda:0")
    T = 1 << 20
    m = VQVAE((T, 1), 3, 64, [3, 2, 2], [2, 2, 2], num_embeddings=a.bins - 1, residual_width=64, residual_depth=4,
              dilation_factor=3, dtype=a.dtype, device="cuda")
    x = torch.rand(1, T, 1, device=dev) * 2 - 1
    out = {"mode": "encode-mem", "samples": T, "level": 0, "dtype": a.dtype, "halo_codes": m.encode_halo(0)}
    whole = None
    for name, fn in (("encode_level", lambda: m.encode_level(x, 0)),
                     ("encode_chunked_65536", lambda: m.encode_chunked(x, 0, chunk_samples=1 << 16)),
                     ("encode_chunked_262144", lambda: m.encode_chunked(x, 0, chunk_samples=1 << 18))):
        fn()  # every shape warmed (workspaces, kernels)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        z = fn()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        out[name] = {"peak_MiB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
                     "ms": round(el * 1e3, 2)}
        whole = z if whole is None else whole
        out[name]["equals_encode_level"] = bool(torch.equal(z, whole))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=8192)
    ap.add_argument("--bins", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--sample-len", type=int, default=2048)
    ap.add_argument("--prime-len", type=int, default=0)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--logprobs", action="store_true",
                    help="sample mode: ask for the log-probabilities (the scored decode kernel)")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--tracks", type=int, default=32)
    ap.add_argument("--audio-ctx", type=int, default=0)
    a = ap.parse_args()
    if a.only in ("feed", "feed-kernel", "encode-mem"):
        return {"feed": feed_mode, "feed-kernel": feed_kernel_mode, "encode-mem": encode_mem_mode}[a.only](a)
    from prior import Prior, FMHABasedAutoregressiveModel
    kw = dict(width=128, depth=6, heads=2, blocks=4, attn_stacks=1, drop_out_rate=0.0)
    dev = torch.device("cuda:0")
    if a.only in ("", "train"):
        pr = Prior(2, [(a.ctx * 16,), (a.ctx * 4,), (a.ctx,)], a.bins, [3, 2, 2], [2, 2, 2], None, kw, None,
                   dtype=a.dtype, device="cuda")
        g = torch.Generator(device=dev).manual_seed(1)
        codes = torch.randint(0, a.bins - 1, (a.batch, a.ctx), device=dev, generator=g)
        pr.capture_train_step(codes, warmup=a.warmup)
        pr.train_step(codes)  # first replay uploads the graph
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            pr.train_step(codes)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        tok = a.batch * a.ctx * a.steps / el
        out = {"metric": "tokens/sec/GPU prior train step (SMALL_PRIOR, ctx 8192)", "value": round(tok, 1),
               "unit": "tokens/s", "n_gpus": 1, "steps": a.steps, "ms_per_step": round(el / a.steps * 1e3, 3),
               "dtype": a.dtype, "data": "synthetic uniform codes, random-init weights",
               "config": {"workload": "BASELINE config 4 (per GPU)", "batch": a.batch, "ctx": a.ctx, "bins": a.bins,
                          **kw}, "loss": float(pr.results()["loss"])}
        # kernel-level rooflines of the step's dominant pieces, timed as hipGraph replays (HIP events on the
        # launching stream): the sequence-linear layer (HBM-bound: bytes = X + Y + residual), the row
        # attention forward and the fused head (MFMA work, exp-heavy)
        import vqa_lib as V
        M = a.batch * a.ctx
        cdt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
        esz = 2 if a.dtype == "bf16" else 4
        x = torch.randn(a.batch, a.ctx, 128, device=dev).to(cdt)
        r = torch.randn_like(x)
        y = torch.empty_like(x)
        w = torch.randn(128, 128, device=dev) * 0.05
        bb = torch.zeros(128, device=dev)
        q = torch.randn(a.batch, a.ctx, 32, device=dev).to(cdt)
        o = torch.empty_like(q)
        lse = torch.empty(a.batch, a.ctx, 2, device=dev)
        wt = torch.empty(a.bins, 128, dtype=cdt, device=dev)
        V.head_wt(torch.randn(128, a.bins, device=dev) * 0.05, wt)
        hb = torch.zeros(a.bins, device=dev)
        hl = torch.empty(M, device=dev)
        am = torch.empty(M, dtype=torch.int64, device=dev)

        def timed(fn, reps=20):
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(reps):
                    fn()
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps * 1e3  # us

        wp = torch.empty(1, 128, 128, dtype=cdt, device=dev)
        V.seqlin_prep([(w, wp, 1, 128, 128, False)], cdt)
        t_lin = timed(lambda: V.seqlin_fwd_prepped(x, wp, bb, y, a.ctx, residual=r))
        lin_bytes = 3 * M * 128 * esz
        t_att = timed(lambda: V.attn_fwd(q, q, q, o, lse, 0, a.ctx // 4, 2, 0.25))
        att_flop = a.batch * 2 * 4 * (a.ctx // 4) * (a.ctx // 4 + 64) / 2 * 16 * 2 * 2
        t_head = timed(lambda: V.head_fwd(x, wt, hb, hl, amax=am))
        head_flop = 2.0 * M * 128 * a.bins
        out["roofline"] = {"kernel": "seqlin_d_kernel<bf16,128,1,8,8> (Dense 128->128 + residual, the mlp form, prepared weights)",
                           "bound": "hbm", "achieved": round(lin_bytes / t_lin / 1e3, 1), "peak": 8000.0,
                           "unit": "GB/s", "frac": round(lin_bytes / t_lin / 1e3 / 8000.0, 4),
                           "avg_launch_us": round(t_lin, 2), "algorithmic_bytes_per_launch": lin_bytes}
        out["kernels"] = {
            "attn_fwd_row": {"us": round(t_att, 1), "tflops": round(att_flop / t_att / 1e6, 1),
                             "mfma_frac": round(att_flop / t_att / 1e6 / 2500.0, 4)},
            "head_fwd": {"us": round(t_head, 1), "tflops": round(head_flop / t_head / 1e6, 1),
                         "mfma_frac": round(head_flop / t_head / 1e6 / 2500.0, 4)}}
        if not a.no_cpu:
            import numpy as np
            from oracle import prior_ref as P
            torch.set_num_threads(min(16, os.cpu_count() or 1))
            cfg = P.PriorConfig(bins=a.bins, ctx=a.ctx, width=128, depth=6, heads=2, blocks=4, attn_stacks=1)
            p = P.to_torch(P.init_params(cfg, 1), torch.float32)
            c = torch.randint(0, a.bins - 1, (1, a.ctx))
            m = torch.zeros(1, a.ctx, dtype=torch.bool)
            t0 = time.perf_counter()
            P.train_step_grads(p, cfg, c, m)
            ce = time.perf_counter() - t0
            out["cpu_baseline"] = {"value": round(a.ctx / ce, 1), "unit": "tokens/s", "cores": torch.get_num_threads(),
                                   "kind": "port", "sample": f"oracle torch-CPU fp32 train step (both passes + "
                                   f"autograd), 1 x {a.ctx} tokens, {ce:.1f} s"}
        print(json.dumps(out), flush=True)
        del pr
        torch.cuda.empty_cache()
    if a.only in ("", "sample"):
        m = FMHABasedAutoregressiveModel(a.bins, 128, 6, 4, heads=2, attn_stacks=1, drop_out_rate=0.0,
                                         context_length=(a.ctx,), level=0, levels=2, zq_shapes=[(a.ctx,), (a.ctx // 4,)],
                                         downs=[3, 2], strides=[2, 2],
                                         cond_kwargs=dict(dilation_factor=3, dilation_cycle=4, residual_width=32,
                                                          residual_depth=8), dtype="fp32", device="cuda")
        g = torch.Generator(device=dev).manual_seed(2)
        up = torch.randint(0, a.bins - 1, (a.samples, a.ctx // 4), device=dev, generator=g)
        prime = (torch.randint(0, a.bins - 1, (a.samples, a.prime_len), device=dev, generator=g)
                 if a.prime_len else None)
        opts = dict(prime=prime, temperature=a.temperature, top_k=a.top_k, top_p=a.top_p)
        lp = dict(return_logprobs=True) if a.logprobs else {}
        opts.update(lp)
        m.sample(a.samples, max_length=16, x_cond=up, seed=1, temperature=a.temperature,
                 top_k=a.top_k, top_p=a.top_p, **lp)  # warm-up (conditioner + the decode kernel that is timed)
        torch.cuda.synchronize()
        els = []
        for _ in range(max(1, a.repeats)):  # one window per launch; an error raises and ends the run
            t0 = time.perf_counter()
            out_tok = m.sample(a.samples, max_length=a.sample_len, x_cond=up, seed=2, **opts)
            if a.logprobs:
                out_tok = out_tok[0]
            torch.cuda.synchronize()
            els.append(time.perf_counter() - t0)
        el = sorted(els)[len(els) // 2]
        print(json.dumps({"metric": "tokens/sec ancestral decode (upsampler prior + ConditionerNet)",
                          "value": round(a.samples * a.sample_len / el, 1), "unit": "tokens/s", "n_gpus": 1,
                          "ms_per_position": round(el / a.sample_len * 1e3, 4),
                          "ms_per_position_repeats": [round(e / a.sample_len * 1e3, 4) for e in els],
                          "prime_len": a.prime_len, "temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p,
                          "samples": a.samples, **({"logprobs": True} if a.logprobs else {}),
                          "positions": a.sample_len, "dtype": "fp32 (decode)",
                          "config": {"workload": "BASELINE config 5", "ctx": a.ctx, "bins": a.bins, **kw},
                          "tokens_in_range": bool(((out_tok >= 0) & (out_tok < a.bins)).all())}), flush=True)

    if a.only in ("", "sampler"):
        # Sampler.py end to end: three levels top-down (n_ctxs of Sampler.py:127, the SMALL_* prior / conditioner
        # settings of :24-25), each window one persistent decode launch, the lower ones conditioned on the codes
        # drawn above them through ConditionerNet
        from sampler import VQVAESampler
        n_ctxs = [8192, 8192, 6144]
        s = VQVAESampler([3, 2, 2], [2, 2, 2], n_ctxs, codebook_size=a.bins, dtype="fp32", device="cuda")
        VQVAESampler([3, 2, 2], [2, 2, 2], [64, 16, 4], codebook_size=a.bins, priors=None, dtype="fp32",
                     device="cuda").sample(a.samples, seed=1)  # warm-up (every kernel, conditioner included)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zs = s.sample(a.samples, seed=2)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        ntok = a.samples * sum(n_ctxs)
        print(json.dumps({"metric": "tokens/sec VQVAESampler 3-level ancestral sampling (Sampler.py)",
                          "value": round(ntok / el, 1), "unit": "tokens/s", "n_gpus": 1, "seconds": round(el, 3),
                          "samples": a.samples, "n_ctxs": n_ctxs, "dtype": "fp32 (decode)",
                          "config": {"workload": "BASELINE config 5 (Sampler.py)", "bins": a.bins, **kw},
                          "shapes": [list(z.shape) for z in zs],
                          "tokens_in_range": bool(all(((z >= 0) & (z < a.bins)).all() for z in zs))}), flush=True)


if __name__ == "__main__":
    main()

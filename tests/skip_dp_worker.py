"""One rank of the step guard's data-parallel test (tests/test_gpu_skip_train.py; not collected by pytest).

tests/dp_worker.py's cfg1 model and batches, compiled with an Adam that skips non-finite steps: one clean eager train
step on this rank's shard of the global batch (gloo, every rank on cuda:0), then one step in which only rank 1's shard
holds a NaN sample. The state before and after that second step is saved.
    python tests/skip_dp_worker.py OUT   (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dp_worker as W  # noqa: E402  (puts the package on sys.path)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

BAD_RANK = 1


def build(B):
    from vqa_optim import Adam
    m = W.build(B)
    m.compile(Adam(skip_nonfinite=True, average_decay=0.9))
    return m


def state(m):
    """Everything a skipped step has to leave alone, as host tensors."""
    torch.cuda.synchronize()
    opt = m.optimizer
    out = {"weights": m.store.flat, "adam_m": opt.m, "adam_v": opt.v, "average": opt.average,
           "iterations": opt.iterations, "trackers": m._macc}
    for l, vq in enumerate(m.vqs):
        out.update({f"vq{l}/E": vq.embeddings, f"vq{l}/ET": vq.ET, f"vq{l}/m_t": vq.m_t, f"vq{l}/N_t": vq.N_t,
                    f"vq{l}/calls": vq.calls, f"vq{l}/esq": vq.e_sqnorm, f"vq{l}/E3": vq.E3})
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def poisoned(x):
    """The batch with one NaN sample in its first item."""
    x = x.clone()
    x[0, x.shape[1] // 2] = float("nan")
    return x


def main():
    out = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = build(W.B_LOCAL)
    xs = [x[rank * W.B_LOCAL:(rank + 1) * W.B_LOCAL] for x in W.batches(world)]
    m.train_step(xs[0])
    before = state(m)
    x = torch.as_tensor(xs[1])
    if rank == BAD_RANK:
        x = poisoned(x)
    m.train_step(x)
    after = state(m)
    skips = {k: int(v) for k, v in m.optimizer.skip_stats().items()}
    torch.save({"before": before, "after": after, "skips": skips,
                "local_input_finite": bool(torch.isfinite(x).all())}, out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

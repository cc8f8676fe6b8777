"""One rank of the clipped data-parallel test (tests/test_gpu_clip_train.py; not collected by pytest).

tests/dp_worker.py's cfg1 model and batches, compiled with a clipping Adam: one eager train step on this rank's
shard of the global batch (gloo, every rank on cuda:0), then the state and the optimizer's clipping statistics
are saved.
    python tests/clip_dp_worker.py OUT MODE THRESHOLD   (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set)
MODE is clipvalue, clipnorm or global_clipnorm.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dp_worker as W  # noqa: E402  (puts the package on sys.path)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

STEPS = 1


def build(B, clip):
    from vqa_optim import Adam
    m = W.build(B)
    m.compile(Adam(**clip))
    return m


def run(m, xs):
    for x in xs[:STEPS]:
        m.train_step(x)
    torch.cuda.synchronize()
    opt = m.optimizer
    return {"weights": m.store.flat.detach().cpu().clone(), "adam_m": opt.m.cpu().clone(),
            "adam_v": opt.v.cpu().clone(), "grads": m.store.grad[:m.store.size].detach().cpu().clone(),
            "stats": torch.stack([v for v in opt.grad_stats().values()]).cpu(),
            "var_norms": opt.variable_grad_norms().cpu().clone()}


def main():
    out, mode, thr = sys.argv[1], sys.argv[2], float(sys.argv[3])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = build(W.B_LOCAL, {mode: thr})
    xs = [x[rank * W.B_LOCAL:(rank + 1) * W.B_LOCAL] for x in W.batches(world)]
    torch.save(run(m, xs), out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

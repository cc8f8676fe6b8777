"""One rank of the weight-averaging data-parallel test (tests/test_gpu_ema_train.py; not collected by pytest).

tests/dp_worker.py's cfg1 model and batches, compiled with an Adam that averages the weights: three eager train steps
on this rank's shard of the global batch (gloo, every rank on cuda:0), then the state and the average are saved.
    python tests/ema_dp_worker.py OUT   (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dp_worker as W  # noqa: E402  (puts the package on sys.path)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

STEPS = 3
AVERAGE = dict(average_decay=0.9, average_start_step=1)


def build(B):
    from vqa_optim import Adam
    m = W.build(B)
    m.compile(Adam(**AVERAGE))
    return m


def run(m, xs):
    for x in xs[:STEPS]:
        m.train_step(x)
    torch.cuda.synchronize()
    opt = m.optimizer
    return {"weights": m.store.flat.detach().cpu().clone(), "adam_m": opt.m.cpu().clone(),
            "adam_v": opt.v.cpu().clone(), "average": opt.average.cpu().clone(),
            "iterations": int(opt.iterations.item())}


def main():
    out = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = build(W.B_LOCAL)
    xs = [x[rank * W.B_LOCAL:(rank + 1) * W.B_LOCAL] for x in W.batches(world)]
    torch.save(run(m, xs), out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

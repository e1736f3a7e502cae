"""Worker of tests/test_gpu_eval_metrics.py: one process = one rank of a validation epoch accumulated with
passt_amd.metrics.EvalAccumulator -- every rank on the single GPU of the test box, transport "gloo" on device tensors, as
tests/ddp_worker.py does for the training step.

    python tests/ddp_eval_worker.py --out one                     single process, all 257 samples  -> one.rank0.pt
    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/ddp_eval_worker.py --out two
                                                                  rank 0 holds the first 150 samples, rank 1 the other 107
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from passt_amd.metrics import EvalAccumulator  # noqa: E402
from tests import eval_metrics_cases as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    group = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
        group = dist.group.WORLD
    s, t, m = K.case(dict(np.load(K.GOLDEN)), "masked", 257, 20)
    lo, hi = (0, 257) if world == 1 else ((0, 150), (150, 257))[rank]
    acc = EvalAccumulator(20, capacity=64)
    for b0 in range(lo, hi, 20):
        b1 = min(b0 + 20, hi)
        acc.update(*[torch.from_numpy(np.ascontiguousarray(a[b0:b1])).to(dev) for a in (s, t, m)])
    res = acc.compute(process_group=group)
    torch.cuda.synchronize()
    torch.save({k: v.cpu() for k, v in res.items()}, f"{args.out}.rank{rank}.pt")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""Worker of tests/test_gpu_grad_clip.py: one process = one data-parallel rank of TrainStep(clip_grad_norm=c, accumulate=2, AdamW) --
every rank on the single GPU of the test box over gloo, as tests/ddp_worker.py.  Two micro-batches of 8 clips per update (the golden
batch and its reverse); rank r of two takes rows [4 r, 4 r + 4) of each, a single process takes all 8.

    python tests/ddp_clip_worker.py --out ref.pt --clip 0.05
    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/ddp_clip_worker.py --out dp.pt --clip 0.05 [--comm-dtype bf16]

Saved by rank 0: params / init (flat), flags [(replicas identical, micro-batch losses)] per rank, norms [grad_norm per update] per rank,
allreduces [collectives launched by each step() call], buckets (the reducer's non-empty buckets), world."""
import argparse
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from passt_amd.train import TrainStep  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--clip", type=float, required=True)
    ap.add_argument("--comm-dtype", default="fp32")
    ap.add_argument("--updates", type=int, default=2)
    args = ap.parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    case = dict(G.CASES["model_small_train"], B=8, seed=333)
    cfg = case["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"], s_patchout_f=cfg["s_patchout_f"],
                              img_size=cfg["img_size"], patch_size=cfg["patch"], stride=cfg["stride"],
                              num_classes=cfg["num_classes"], embed_dim=cfg["embed_dim"], depth=cfg["depth"],
                              num_heads=cfg["num_heads"], distilled=True)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in detgen.passt_state_dict(cfg, case["seed"]).items()}, strict=True)
    net = net.to(dev).train()
    net.precision = "fp32"
    x, y = G.model_inputs(case)
    xg, yg = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    micro = [(xg, yg), (xg.flip(0).contiguous(), yg.flip(0).contiguous())]
    if world > 1:
        per = x.shape[0] // world
        micro = [(a[rank * per:(rank + 1) * per].contiguous(), b[rank * per:(rank + 1) * per].contiguous()) for a, b in micro]
    ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=False, comm_dtype=args.comm_dtype, clip_grad_norm=args.clip,
                   accumulate=2)
    init = ts.flat_p.clone()
    launched, real = [0], ts.reducer._all_reduce

    def counted(t):
        launched[0] += 1
        return real(t)
    ts.reducer._all_reduce = counted
    losses, norms, allreduces = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for u in range(args.updates):
            for i, (a, b) in enumerate(micro):
                torch.manual_seed(900 + 2 * u + i)      # the SAME patchout draws on every rank and in the single-process run
                np.random.seed(900 + 2 * u + i)
                before = launched[0]
                losses.append(float(ts.step(a, b).item()))
                allreduces.append(launched[0] - before)
                assert ts.t == u + i, (ts.t, u, i)
            norms.append(float(ts.grad_norm))
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        mine, ref0 = ts.flat_p.clone(), ts.flat_p.clone()
        dist.broadcast(ref0, 0)
        flags, all_norms = [None] * world, [None] * world
        dist.all_gather_object(flags, (bool(torch.equal(mine, ref0)), losses))
        dist.all_gather_object(all_norms, norms)
    else:
        flags, all_norms = [(True, losses)], [norms]
    if rank == 0:
        torch.save({"params": ts.flat_p.cpu(), "init": init.cpu(), "flags": flags, "norms": all_norms, "allreduces": allreduces,
                    "buckets": len(ts._spans()), "world": world}, args.out)
    ts.close()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

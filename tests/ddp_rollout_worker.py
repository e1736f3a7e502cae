"""Worker of tests/test_gpu_rollout.py's data-parallel test: one backward of ``net(x, rollout="cam")`` under passt_amd.ddp.attach -- every
rank on the single GPU of the test box, transport gloo on device tensors, as tests/ddp_hidden_worker.py.

    python tests/ddp_rollout_worker.py --out ref.pt      single process, no reducer: the two half-batches one after the other
    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/ddp_rollout_worker.py --out dp.pt

Saved by rank 0: ``rows`` = per half-batch (single process) resp. per rank the (4, 2, Ntok) ``roll.grad``, ``depth``, ``world``.
"""
import argparse
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_hidden_golden as HG  # noqa: E402


def backward_once(net, x, a, b):
    """``roll.grad`` of the fixture's loss on one half-batch"""
    net.zero_grad()
    torch.manual_seed(900)                       # the same Patchout draws for every half-batch, rank and run
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, feat, roll = net(x, rollout="cam")
    ((logits * a).sum() + (feat * b).sum()).backward()
    torch.cuda.synchronize()
    return roll.grad.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world)
    case = dict(G.CASES["model_small_train"], B=8, T=250, seed=335)
    cfg = case["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"], s_patchout_f=cfg["s_patchout_f"],
                              img_size=cfg["img_size"], patch_size=cfg["patch"], stride=cfg["stride"], num_classes=cfg["num_classes"],
                              embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], distilled=True)
    sd = detgen.passt_state_dict(cfg, case["seed"])
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    net = net.to(dev).train()
    net.precision = "fp32"
    x, a, b = (torch.from_numpy(t).to(dev) for t in HG.inputs(case))
    half = lambda t, r: t[4 * r:4 * r + 4].contiguous()  # noqa: E731
    if world == 1:
        res = [backward_once(net, half(x, r), half(a, r), half(b, r)) for r in range(2)]
    else:
        from passt_amd import ddp
        ddp.attach(net, comm_dtype="fp32", transport="torch")
        mine = backward_once(net, half(x, rank), half(a, rank), half(b, rank))
        res = [None] * world
        dist.all_gather_object(res, mine)
        ddp.detach(net)
    if rank == 0:
        torch.save({"rows": res, "depth": cfg["depth"], "world": world}, args.out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

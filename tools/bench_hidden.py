#!/usr/bin/env python
"""Cost of asking for token outputs, ``net(x, hidden=...)``: passt_s size (768 / 12 / 12, stride 10, 128 x 998 = 1190 tokens, eval, no
Patchout), every parameter frozen, x.requires_grad, bf16, one GPU: forward + backward of one batch.  One JSON line per configuration.

  requests   none        net(x)                                   loss = (features * w).sum() + (logits * v).sum()
             mid         net(x, hidden=(3, 7, 10))                + sum_l h_l.square().sum()   (torch elementwise kernels, timed with it)
             last        net(x, hidden=(-1,))                     likewise
             last_norm   net(x, hidden=(-1, "norm"))              likewise
             none_d11    net(x) with the last block removed: ``none`` minus this is what ONE ordinary block costs, forward and
                         backward, in the same run -- the yardstick for what ``last`` adds over ``none``
  Every configuration runs in a fresh child process, --reps times; the driver reports medians.
  --against DIR: ``none`` is also measured in another checkout (the parent commit), this checkout and DIR alternating in ABBA order
  (A B B A ...), and the two medians are reported with the run-to-run spread of each.

    python tools/bench_hidden.py --batch 16 --against ../parent_checkout
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUESTS = {"none": None, "none_d11": None, "mid": (3, 7, 10), "last": (-1,), "last_norm": (-1, "norm")}


def run_child(a):
    import torch
    sys.path.insert(0, a.root)
    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527, s_patchout_t=0, s_patchout_f=0)
        if a.request == "none_d11":
            net.blocks = torch.nn.Sequential(*list(net.blocks)[:-1])
        net = net.cuda().eval().requires_grad_(False)
    net.precision = "bf16"
    hidden = REQUESTS[a.request]
    x = ((torch.rand(a.batch, 1, 128, 998, device="cuda") * 2 - 1) * 1.5).requires_grad_()
    w, v = torch.rand(a.batch, 768, device="cuda"), torch.rand(a.batch, 527, device="cuda")

    def step():
        x.grad = None
        if hidden is None:
            logits, feat = net(x)
            hs = ()
        else:
            logits, feat, hs = net(x, hidden=hidden)
        loss = (feat * w).sum() + (logits * v).sum()
        for h in hs:
            loss = loss + h.square().sum()
        loss.backward()

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps({"request": a.request, "root": os.path.abspath(a.root), "B": a.batch, "ms_median": round(statistics.median(ms), 3),
                      "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                      "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}), flush=True)


def run_driver(a):
    def child(root, request):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--request", request, "--root", root, "--batch", str(a.batch),
               "--warmup", str(a.warmup), "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"{request} in {root} failed with exit status {r.returncode}")
        return json.loads(r.stdout.strip().splitlines()[-1])["ms_median"]

    def summary(v):
        return {"ms": round(statistics.median(v), 3), "ms_per_rep": v, "spread_ms": round(max(v) - min(v), 3)}

    base = {"bench": "hidden_states", "B": a.batch, "precision": "bf16", "tokens": 1190, "frozen": True}
    here = []
    if a.against:
        other = []
        for r in range(a.reps):             # A B B A ...
            pair = [(a.root, here), (a.against, other)]
            for root, sink in (pair if r % 2 == 0 else pair[::-1]):
                sink.append(child(root, "none"))
        s_here, s_other = summary(here), summary(other)
        diff = s_here["ms"] - s_other["ms"]
        print(json.dumps(dict(base, request="none", this_checkout=s_here, other_checkout=s_other, diff_ms=round(diff, 3),
                              within_spread=abs(diff) <= max(s_here["spread_ms"], s_other["spread_ms"]))), flush=True)
    else:
        here = [child(a.root, "none") for _ in range(a.reps)]
        print(json.dumps(dict(base, request="none", **summary(here))), flush=True)
    none_ms = statistics.median(here)
    res = {}
    for request in ("none_d11", "mid", "last", "last_norm"):
        res[request] = summary([child(a.root, request) for _ in range(a.reps)])
        print(json.dumps(dict(base, request=request, **res[request], minus_none_ms=round(res[request]["ms"] - none_ms, 3))), flush=True)
    block = none_ms - res["none_d11"]["ms"]
    print(json.dumps(dict(base, summary="cost of the last-block request next to one ordinary block", one_block_fwd_bwd_ms=round(block, 3),
                          last_minus_none_ms=round(res["last"]["ms"] - none_ms, 3),
                          last_norm_minus_none_ms=round(res["last_norm"]["ms"] - none_ms, 3),
                          mid_minus_none_ms=round(res["mid"]["ms"] - none_ms, 3),
                          last_over_one_block=round((res["last"]["ms"] - none_ms) / block, 3) if block > 0 else None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="measure one request in this process")
    ap.add_argument("--request", default="none", choices=list(REQUESTS))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--root", default=HERE, help="checkout to import passt_amd from")
    ap.add_argument("--against", default="", help="another checkout (the parent commit) whose `none` step is measured alternately")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    run_child(a) if a.child else run_driver(a)


if __name__ == "__main__":
    main()

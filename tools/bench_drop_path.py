#!/usr/bin/env python
"""Cost of stochastic depth (drop_path_rate > 0) in the fused training step, config-#2 shapes: passt_s (768 / 12 / 12, stride 10, 128
mel bands, 998 frames, s_patchout_t = 40, s_patchout_f = 4 -> 474 tokens), B = 64, bf16, one GPU.  One JSON line per measurement.

  step     a full passt_amd.train.TrainStep (spectrograms in; mixup + forward + BCE + backward + per-bucket AdamW) of two models in ONE
           process -- A: drop_path_rate = 0 (the step as it always was), B: --rate (default 0.1) -- in blocks of --iters steps,
           alternating A B B A ... --reps times, device events around every block with a synchronise behind it.  Reports the per-step
           medians, every block's value and B - A.
  kernels  the launches that carry the factor, alone on the step's shapes (M = 64 x 474 rows, operands warm in the caches, so these
           are kernel times in isolation, not their share of the step): proj's and fc2's residual GEMM and the LayerNorm backward,
           each without and with a row factor, alternating, median of --kiters launches timed one by one with device events.

    python tools/bench_drop_path.py --out profiles/drop_path.txt
"""
import argparse
import json
import os
import statistics
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B, TOKENS, D = 64, 474, 768


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def bench_step(a):
    import numpy as np
    import torch

    import passt_amd
    from passt_amd.train import TrainStep
    steps = {}
    for tag, rate in (("A", 0.0), ("B", a.rate)):
        torch.manual_seed(0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = passt_amd.PaSST(s_patchout_t=40, s_patchout_f=4, img_size=(128, 998), stride=10, num_classes=527, embed_dim=D, depth=12,
                                  num_heads=12, distilled=True, drop_path_rate=rate).cuda().train()
        net.precision = "bf16"
        steps[tag] = TrainStep(net, None, lr=2e-5, weight_decay=1e-4, use_mixup=True, loss="bce", graph=a.graph)
    x = torch.randn(B, 1, 128, 998, device="cuda")
    y = (torch.rand(B, 527, device="cuda") < 0.05).float()
    np.random.seed(0)

    def block(ts, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ts.step(x, y)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for ts in steps.values():
            block(ts, a.warmup)
        ms = {"A": [], "B": []}
        for r in range(a.reps):
            for tag in ("ABBA" if r % 2 == 0 else "BAAB"):
                ms[tag].append(round(block(steps[tag], a.iters), 4))
    mA, mB = statistics.median(ms["A"]), statistics.median(ms["B"])
    emit(a, {"bench": "drop_path_train_step", "precision": "bf16", "batch": B, "tokens": TOKENS, "graph": bool(a.graph), "rate_B": a.rate,
             "steps_per_block": a.iters, "A_rate0_ms_per_step": mA, "A_blocks": ms["A"], "B_ms_per_step": mB, "B_blocks": ms["B"],
             "B_minus_A_ms": round(mB - mA, 4), "B_over_A": round(mB / mA, 5),
             "A_spread_ms": round(max(ms["A"]) - min(ms["A"]), 4)})


def bench_kernels(a):
    import torch

    from passt_amd import ops
    from passt_amd._lib import PA_BF16
    M = B * TOKENS
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g) * 2 - 1  # noqa: E731
    keep = 0.9
    rs = (torch.floor(keep + torch.rand(B, device="cuda", generator=g)) / keep).repeat_interleave(TOKENS).contiguous()
    resid = rnd(M, D)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.kiters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
        return out

    def pair(name, plain, scaled):
        us = {"plain": [], "rowscale": []}
        for r in range(2):
            for tag, fn in ((("plain", plain), ("rowscale", scaled)) if r == 0 else (("rowscale", scaled), ("plain", plain))):
                us[tag] += timed(fn)
        p, s = statistics.median(us["plain"]), statistics.median(us["rowscale"])
        emit(a, {"bench": "drop_path_kernel", "kernel": name, "M": M, "launches_each": 2 * a.kiters, "plain_us": round(p, 2),
                 "rowscale_us": round(s, 2), "delta_us": round(s - p, 2), "plain_min_max_us": [round(min(us["plain"]), 2), round(max(us["plain"]), 2)]})

    for name, K in (("resid_proj_K768", D), ("resid_fc2_K3072", 4 * D)):
        A, W, bias = rnd(M, K).bfloat16(), (rnd(D, K) * 0.05).bfloat16(), rnd(D)
        out = torch.empty_like(resid)
        pair(name, lambda: ops.linear_resid(A, W, bias, resid, PA_BF16, out=out),
             lambda: ops.linear_resid(A, W, bias, resid, PA_BF16, out=out, rowscale=rs))
    x, gam, bet = rnd(M, D) * 3 + 0.5, rnd(D) * 0.3 + 1, rnd(D)
    _, mean, rstd = ops.layernorm_fwd(x, gam, bet, 1e-6, PA_BF16)
    dy, dres = rnd(M, D).bfloat16(), rnd(M, D)
    dg, db, dc = (torch.empty(D, device="cuda") for _ in range(3))
    pair("layernorm_bwd", lambda: ops.layernorm_bwd(dy, x, gam, mean, rstd, dres, dg, db, True, dcolsum=dc, defer=[]),
         lambda: ops.layernorm_bwd(dy, x, gam, mean, rstd, dres, dg, db, True, dcolsum=dc, defer=[], rowscale=rs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="step,kernels")
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--graph", action="store_true", help="TrainStep(graph=True)")
    ap.add_argument("--out", default="", help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--kiters", type=int, default=30)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_drop_path.py measures on the GPU: no device found")
    if "step" in a.what:
        bench_step(a)
    if "kernels" in a.what:
        bench_kernels(a)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of attention dropout in the fused attention, at the headline shape: B = 64, H = 12, N = 474, bf16, pre-scaled q, one GPU.
One JSON line per measurement (appended to --out).

  kernels  pa_attention_fwd_dropout against pa_attention_fwd, pa_attention_bwd_dropout (always the dQ + dK/dV pair) against the plain
           pair (PA_ATTN_BWD_TWO_PASS), and the plain pair against the single pass (what pa_attention_bwd runs at this shape): the
           same random operands, launches alternating A B B A, each timed with device events, medians and min / max.
  step     a full passt_amd.train.TrainStep of two models in ONE process -- A: no dropout, B: attn_drop.p = --rate (default 0.1) on
           every block -- in blocks of --iters steps, alternating A B B A ... --reps times.

The cost ratio is what this measures, not a target.

    python tools/bench_attn_dropout.py --out profiles/attn_dropout.txt
"""
import argparse
import json
import os
import statistics
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B, H, TOKENS, D = 64, 12, 474, 768


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def bench_kernels(a):
    import torch

    from passt_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1)
    scale = 64 ** -0.5
    qkv = (torch.rand(B * TOKENS, 3 * D, device="cuda", generator=g) * 2 - 1)
    qkv[:, :D] *= scale * ops.LOG2E
    qkv = qkv.bfloat16()
    d_o = (torch.rand(B * TOKENS, D, device="cuda", generator=g) * 2 - 1).bfloat16()
    seed = torch.tensor([0x1234567, 0x89abcde], dtype=torch.int32, device="cuda")
    t = ops.attn_drop_t(a.rate)
    PRE = ops.ATTN_Q_PRESCALED
    o, lse = ops.attention_fwd(qkv, B, H, TOKENS, scale, flags=PRE)
    od, lsed = ops.attention_fwd_dropout(qkv, B, H, TOKENS, scale, seed, 0, t, flags=PRE)
    assert torch.equal(lse, lsed)
    arms = {
        "fwd_plain": lambda: ops.attention_fwd(qkv, B, H, TOKENS, scale, flags=PRE),
        "fwd_dropout": lambda: ops.attention_fwd_dropout(qkv, B, H, TOKENS, scale, seed, 0, t, flags=PRE),
        "bwd_pair_plain": lambda: ops.attention_bwd(qkv, o, d_o, lse, B, H, TOKENS, scale, flags=PRE | ops.ATTN_BWD_TWO_PASS),
        "bwd_pair_dropout": lambda: ops.attention_bwd_dropout(qkv, od, d_o, lse, B, H, TOKENS, scale, seed, 0, t, flags=PRE),
        "bwd_single_pass": lambda: ops.attention_bwd(qkv, o, d_o, lse, B, H, TOKENS, scale, flags=PRE | ops.ATTN_BWD_SINGLE_PASS),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def versus(name, x, y):
        us = {x: [], y: []}
        for fn in (arms[x], arms[y]):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for r in range(a.kiters):
            for tag in ((x, y, y, x) if r % 2 == 0 else (y, x, x, y)):
                us[tag].append(timed(arms[tag]))
        mx, my = statistics.median(us[x]), statistics.median(us[y])
        emit(a, {"bench": "attn_dropout_kernel", "pair": name, "B": B, "H": H, "N": TOKENS, "dtype": "bf16", "t": t, "launches_each": 2 * a.kiters,
                 x + "_us": round(mx, 2), y + "_us": round(my, 2), "ratio": round(my / mx, 4),
                 x + "_min_max_us": [round(min(us[x]), 2), round(max(us[x]), 2)], y + "_min_max_us": [round(min(us[y]), 2), round(max(us[y]), 2)]})

    versus("forward", "fwd_plain", "fwd_dropout")
    versus("backward_pair", "bwd_pair_plain", "bwd_pair_dropout")
    versus("pair_vs_single_pass", "bwd_single_pass", "bwd_pair_plain")


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
                                  num_heads=12, distilled=True).cuda().train()
        for blk in net.blocks:
            blk.attn.attn_drop.p = rate
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
    emit(a, {"bench": "attn_dropout_train_step", "precision": "bf16", "batch": B, "tokens": TOKENS, "graph": bool(a.graph), "p_B": a.rate,
             "t_B": __import__("passt_amd").ops.attn_drop_t(a.rate), "steps_per_block": a.iters, "A_no_dropout_ms_per_step": mA, "A_blocks": ms["A"],
             "B_ms_per_step": mB, "B_blocks": ms["B"], "B_minus_A_ms": round(mB - mA, 4), "B_over_A": round(mB / mA, 5),
             "A_spread_ms": round(max(ms["A"]) - min(ms["A"]), 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernels,step")
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--graph", action="store_true", help="TrainStep(graph=True)")
    ap.add_argument("--out", default="", help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kiters", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_dropout.py measures on the GPU: no device found")
    if "kernels" in a.what:
        bench_kernels(a)
    if "step" in a.what:
        bench_step(a)


if __name__ == "__main__":
    main()

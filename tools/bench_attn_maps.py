#!/usr/bin/env python
"""Cost of the attention maps (``net(x, attn=...)``), passt_s size (768 / 12 / 12, stride 10), bf16, one GPU.  One JSON line per
configuration.

  kernel   pa_attention_probs alone on a random qkv of the shape, in the four modes (rows all / prefix x heads each / mean): median
           time, and the fraction of bench_kernels.py's HBM peak its OUTPUT bytes reach (the kernel is write-bound in the "each"
           modes; the figure is a report, not a pass / fail)
  forward  the forward without ``attn`` against the forward with attn=(-1,) ("prefix" and "all") and attn=range(depth), in the four
           modes, under torch.no_grad()

Shapes: the eval model at 998 frames (1190 tokens) at B = 1 and B = 8, and the training shape (Patchout: 474 tokens) at B = 64.

    python tools/bench_attn_maps.py > profiles/attn_maps_bench.txt
"""
import argparse
import json
import os
import statistics
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
HBM_PEAK_GBS = 8000.0           # bench_kernels.py HBM_PEAK
SHAPES = [dict(name="eval_1190", B=1, train=False), dict(name="eval_1190", B=8, train=False), dict(name="train_474", B=64, train=True)]
MODES = [(rows, heads) for rows in ("all", "prefix") for heads in ("each", "mean")]


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def run_kernel(a, shape, N):
    import torch
    from passt_amd import ops
    B, H, scale = shape["B"], 12, 0.125
    qkv = ((torch.rand(B * N, 3 * H * 64, device="cuda") * 2 - 1) * 1.5).bfloat16()
    qkv[:, :H * 64] *= scale * ops.LOG2E
    for rows, heads in MODES:
        nq = 2 if rows == "prefix" else N
        _, lse = ops.attention_fwd(qkv, B, H, N, scale, nq=nq, flags=ops.ATTN_Q_PRESCALED)
        out = torch.empty((B, 1 if heads == "mean" else H, nq, N), device="cuda")
        ms = timed(lambda: ops.attention_probs(qkv, lse, B, H, N, scale, nq=nq, head_mean=heads == "mean", flags=ops.ATTN_Q_PRESCALED,
                                               out=out), a.warmup, a.iters)
        nbytes = out.numel() * 4
        print(json.dumps({"bench": "attention_probs_kernel", "shape": shape["name"], "B": B, "H": H, "N": N, "rows": rows, "heads": heads,
                          "ms_median": round(ms, 4), "out_mb": round(nbytes / 2 ** 20, 2), "write_gb_per_s": round(nbytes / ms / 1e6, 1),
                          "frac_hbm_peak": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)}), flush=True)
        del out


def run_forward(a, shape):
    import torch
    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527,
                                  **({} if shape["train"] else dict(s_patchout_t=0, s_patchout_f=0))).cuda().train(shape["train"])
    net.precision = "bf16"
    x = (torch.rand(shape["B"], 1, 128, 998, device="cuda") * 2 - 1) * 1.5
    depth = len(net.blocks)

    def fwd(**kw):
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return net(x, **kw)

    N = fwd(attn=(0,), attn_rows="prefix")[2][0].shape[-1]
    base = timed(fwd, a.warmup, a.iters)
    print(json.dumps({"bench": "forward", "shape": shape["name"], "B": shape["B"], "N": N, "attn": None, "ms_median": round(base, 3)}), flush=True)
    for rows, heads in MODES:
        for label, req in (("(-1,)", (-1,)), (f"range({depth})", tuple(range(depth)))):
            ms = timed(lambda: fwd(attn=req, attn_rows=rows, attn_heads=heads), a.warmup, a.iters)
            print(json.dumps({"bench": "forward", "shape": shape["name"], "B": shape["B"], "N": N, "attn": label, "rows": rows, "heads": heads,
                              "ms_median": round(ms, 3), "over_plain_forward": round(ms / base, 3)}), flush=True)
    return N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    for shape in SHAPES:
        N = run_forward(a, shape)
        run_kernel(a, shape, N)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of the attention maps' gradients (``net(x, attn=..., attn_grad=...)``), passt_s size (768 / 12 / 12, stride 10), bf16, one
GPU.  One JSON line per configuration; a report, not a pass / fail.

  kernel    pa_attention_probs_grad alone on a random qkv / d_o of the shape: "grad" (rows all / prefix, each head) and "cam" (rows
            all / prefix x heads each / mean): median time, and the fraction of bench_kernels.py's HBM peak its OUTPUT bytes reach
            (the "each" modes are write-bound; "cam" with the head mean writes 1 / H of the bytes for the same products)
  backward  the backward of a forward run with attn=(-1,) / attn=range(depth), without and with ``attn_grad``, in the same run and in
            ABBA order (without, with, with, without: a drift of the clocks falls on both alike); the forward is not timed

Shapes: the eval model at 998 frames (1190 tokens) at B = 1 and B = 8, and the training shape at B = 64 (train mode with the
reference's Patchout, s_patchout_t=40 / s_patchout_f=4: 474 tokens); a run whose token count is not the shape's stops.

    python tools/bench_attn_grad.py > profiles/attn_grad_bench.txt
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
# ``N``: the token count the shape stands for (2 + 12 x 99 patches in eval mode; 2 + 8 x 59 kept by the reference's training Patchout)
SHAPES = [dict(name="eval_1190", B=1, train=False, N=1190, patchout=dict(s_patchout_t=0, s_patchout_f=0)),
          dict(name="eval_1190", B=8, train=False, N=1190, patchout=dict(s_patchout_t=0, s_patchout_f=0)),
          dict(name="train_474", B=64, train=True, N=474, patchout=dict(s_patchout_t=40, s_patchout_f=4))]
# (attn_grad, attn_rows, attn_heads)
MODES = [("grad", "all", "each"), ("grad", "prefix", "each"), ("cam", "all", "each"), ("cam", "all", "mean"), ("cam", "prefix", "each"),
         ("cam", "prefix", "mean")]


def timed_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_kernel(a, shape, N):
    import torch
    from passt_amd import ops
    B, H, scale = shape["B"], 12, 0.125
    qkv = ((torch.rand(B * N, 3 * H * 64, device="cuda") * 2 - 1) * 1.5).bfloat16()
    qkv[:, :H * 64] *= scale * ops.LOG2E
    d_tok = (torch.rand(B * N, H * 64, device="cuda") * 2 - 1).bfloat16()
    for mode, rows, heads in MODES:
        nq = 2 if rows == "prefix" else N
        _, lse = ops.attention_fwd(qkv, B, H, N, scale, nq=nq, flags=ops.ATTN_Q_PRESCALED)
        out = torch.empty((B, 1 if heads == "mean" else H, nq, N), device="cuda")
        kw = dict(nq=nq, head_mean=heads == "mean", mode=ops.ATTN_PGRAD_CAM if mode == "cam" else ops.ATTN_PGRAD_GRAD,
                  flags=ops.ATTN_Q_PRESCALED, out=out)

        def launch():
            ops.attention_probs_grad(qkv, lse if mode == "cam" else None, d_tok, B, H, N, scale, **kw)

        for _ in range(a.warmup):
            launch()
        ms = statistics.median(timed_once(launch) for _ in range(a.iters))
        nbytes = out.numel() * 4
        print(json.dumps({"bench": "attention_probs_grad_kernel", "shape": shape["name"], "B": B, "H": H, "N": N, "attn_grad": mode,
                          "rows": rows, "heads": heads, "ms_median": round(ms, 4), "out_mb": round(nbytes / 2 ** 20, 2),
                          "write_gb_per_s": round(nbytes / ms / 1e6, 1), "frac_hbm_peak": round(nbytes / ms / 1e6 / HBM_PEAK_GBS, 4)}),
              flush=True)
        del out


def run_backward(a, shape):
    import torch
    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527,
                                  **shape["patchout"]).cuda().train(shape["train"])
    net.precision = "bf16"
    x = (torch.rand(shape["B"], 1, 128, 998, device="cuda") * 2 - 1) * 1.5
    depth = len(net.blocks)
    N = None

    def backward_ms(**kw):
        nonlocal N
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = net(x, **kw)
        N = out[2][0].shape[-1]
        if N != shape["N"]:
            raise RuntimeError(f"shape {shape['name']} stands for {shape['N']} tokens but the model ran on {N}")
        loss = out[0].sum() + out[1].sum()
        torch.cuda.synchronize()
        ms = timed_once(loss.backward)
        net.zero_grad(set_to_none=True)
        return ms

    for mode, rows, heads in MODES:
        for label, req in (("(-1,)", (-1,)), (f"range({depth})", tuple(range(depth)))):
            plain_kw = dict(attn=req, attn_rows=rows, attn_heads=heads)
            grad_kw = dict(plain_kw, attn_grad=mode)
            for _ in range(a.warmup):
                backward_ms(**plain_kw)
                backward_ms(**grad_kw)
            plain, grad = [], []
            for _ in range(max(1, a.iters // 2)):                   # A B B A
                plain.append(backward_ms(**plain_kw))
                grad.append(backward_ms(**grad_kw))
                grad.append(backward_ms(**grad_kw))
                plain.append(backward_ms(**plain_kw))
            p, g = statistics.median(plain), statistics.median(grad)
            print(json.dumps({"bench": "backward", "shape": shape["name"], "B": shape["B"], "N": N, "attn": label, "rows": rows, "heads": heads,
                              "attn_grad": mode, "ms_attn_only": round(p, 3), "ms_with_attn_grad": round(g, 3),
                              "over_attn_only": round(g / p, 3)}), flush=True)
    return N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=6)
    a = ap.parse_args()
    for shape in SHAPES:
        N = run_backward(a, shape)
        run_kernel(a, shape, N)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of the fused attention rollout (``net(x, rollout=...)``) against the route it replaces, passt_s size (768 / 12 / 12, stride
10), bf16, one GPU.  One JSON line per configuration; a report, not a pass / fail.

  kernel    pa_attention_rollout alone on a random qkv / d_o of the shape, two row vectors: ATTN and CAM, all query rows and the
            prefix-only tail's nq = 2: median time per block and the slice count the library chose
  route     the whole call, fused against unfused, in the same run and in ABBA order (unfused, fused, fused, unfused: a drift of the
            clocks falls on both alike), with torch.cuda.max_memory_allocated() of each:
              "attn"  unfused: maps = net(x, attn=range(depth), attn_heads="mean") under no_grad, then INTEGRATION.md 1.6's chain
                      roll = (0.5 a + 0.5 I) / rowsum @ roll in torch;  fused: net(x, rollout="attn") under no_grad
              "cam"   unfused: net(x, attn=range(depth), attn_heads="mean", attn_grad="cam"), the backward, then the chain
                      roll = roll + cam @ roll;  fused: net(x, rollout="cam") and the backward
            and the plain call (no maps, no rollout) for scale.

Shapes: the eval model at 998 frames (1190 tokens) at B = 1 and B = 8, and the training shape at B = 64 (train mode with the
reference's Patchout, s_patchout_t=40 / s_patchout_f=4: 474 tokens); a run whose token count is not the shape's stops.

    python tools/bench_rollout.py > profiles/rollout_bench.txt
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
# ``N``: the token count the shape stands for (2 + 12 x 99 patches in eval mode; 2 + 8 x 59 kept by the reference's training Patchout)
SHAPES = [dict(name="eval_1190", B=1, train=False, N=1190, patchout=dict(s_patchout_t=0, s_patchout_f=0)),
          dict(name="eval_1190", B=8, train=False, N=1190, patchout=dict(s_patchout_t=0, s_patchout_f=0)),
          dict(name="train_474", B=64, train=True, N=474, patchout=dict(s_patchout_t=40, s_patchout_f=4))]


def timed_once(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run_kernel(a, shape):
    import torch
    from passt_amd import _lib, ops
    B, H, N, scale = shape["B"], 12, shape["N"], 0.125
    qkv = ((torch.rand(B * N, 3 * H * 64, device="cuda") * 2 - 1) * 1.5).bfloat16()
    qkv[:, :H * 64] *= scale * ops.LOG2E
    d_tok = (torch.rand(B * N, H * 64, device="cuda") * 2 - 1).bfloat16()
    r = torch.rand(B, 2, N, device="cuda")
    out = torch.empty_like(r)
    for mode in ("attn", "cam"):
        for nq in (N, 2):
            _, lse = ops.attention_fwd(qkv, B, H, N, scale, nq=nq, flags=ops.ATTN_Q_PRESCALED)
            cam = mode == "cam"
            d_o = (d_tok.view(B, N, -1)[:, :2].reshape(2 * B, -1).contiguous() if nq == 2 else d_tok) if cam else None
            kw = dict(nq=nq, d_o=d_o, mode=ops.ATTN_ROLLOUT_CAM if cam else ops.ATTN_ROLLOUT_ATTN, do_compact=cam and nq == 2,
                      flags=ops.ATTN_Q_PRESCALED, out=out)

            def launch():
                ops.attention_rollout(qkv, lse, r, B, H, N, scale, 1.0, 1.0, **kw)

            for _ in range(a.warmup):
                launch()
            ms = statistics.median(timed_once(launch) for _ in range(a.iters))
            ws = _lib.load().pa_attention_rollout_ws_floats(B * N, B, N, nq, 2, 0)
            print(json.dumps({"bench": "attention_rollout_kernel", "shape": shape["name"], "B": B, "H": H, "N": N, "mode": mode, "nq": nq,
                              "slices": max(1, ws // (2 * B * N)), "ws_mb": round(ws * 4 / 2 ** 20, 2), "ms_median": round(ms, 4),
                              "map_mb_not_written": round(B * min(nq, N) * N * 4 / 2 ** 20, 1)}), flush=True)


def run_routes(a, shape):
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

    def call(grad, **kw):
        with warnings.catch_warnings(), (contextlib.nullcontext() if grad else torch.no_grad()):
            warnings.simplefilter("ignore")
            out = net(x, **kw)
        if grad:
            (out[0].sum() + out[1].sum()).backward()
        return out

    def plain(mode):
        call(mode == "cam")

    def unfused(mode):
        if mode == "attn":
            maps = call(False, attn=range(depth), attn_heads="mean")[2]
            roll = torch.eye(maps[0].shape[-1], device=x.device).expand_as(maps[0])
            for m in maps:
                m = 0.5 * m + 0.5 * torch.eye(m.shape[-1], device=m.device)
                roll = (m / m.sum(-1, keepdim=True)) @ roll
        else:
            cams = call(True, attn=range(depth), attn_heads="mean", attn_grad="cam")[2]
            roll = torch.eye(cams[0].shape[-1], device=x.device).expand_as(cams[0])
            for c in cams:
                roll = roll + c.grad @ roll
        return roll[:, :2]

    def fused(mode):
        roll = call(mode == "cam", rollout=mode)[2]
        return roll if mode == "attn" else roll.grad

    def measure(fn, mode):
        res = []

        def go():
            res.append(fn(mode))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = timed_once(go)
        peak = torch.cuda.max_memory_allocated()
        rows = res.pop()
        net.zero_grad(set_to_none=True)
        return ms, peak, rows

    for mode in ("attn", "cam"):
        for _ in range(a.warmup):
            for fn in (plain, unfused, fused):
                _, _, rows = measure(fn, mode)
        if rows.shape[-1] != shape["N"]:
            raise RuntimeError(f"shape {shape['name']} stands for {shape['N']} tokens but the model ran on {rows.shape[-1]}")
        t = {plain: [], unfused: [], fused: []}
        peak = {}
        for _ in range(max(1, a.iters // 2)):                       # A B B A
            for fn in (unfused, fused, fused, unfused, plain):
                ms, peak[fn], _ = measure(fn, mode)
                t[fn].append(ms)
        u, f, p = (statistics.median(t[fn]) for fn in (unfused, fused, plain))
        print(json.dumps({"bench": "route", "shape": shape["name"], "B": shape["B"], "N": shape["N"], "rollout": mode,
                          "what": "forward + chain" if mode == "attn" else "forward + backward + chain",
                          "ms_plain_call": round(p, 3), "ms_unfused": round(u, 3), "ms_fused": round(f, 3), "unfused_over_fused": round(u / f, 2),
                          "fused_over_plain": round(f / p, 3), "peak_mb_plain": round(peak[plain] / 2 ** 20, 1),
                          "peak_mb_unfused": round(peak[unfused] / 2 ** 20, 1), "peak_mb_fused": round(peak[fused] / 2 ** 20, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=4)
    a = ap.parse_args()
    for shape in SHAPES:
        run_routes(a, shape)
        run_kernel(a, shape)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of stochastic depth and attention dropout on ragged training batches (net.varlen_regularize = True), passt_s size (768 / 12 /
12, stride 10, 128 mel bands), bf16, one GPU, on the clip mix of tools/bench_varlen_step.py: B = 64 spectrograms whose lengths are drawn
uniformly between 2 s and 10 s under a fixed seed, structured Patchout 15 columns / 2 rows per clip, BCE, AdamW, mixup on.  One JSON
line per measurement (appended to --out).

  step     TrainStep.step on the same clips, five ways in ONE process, the variants alternating block by block (a .. e, e .. a, ...):
    a  ragged, switch on, every rate 0        (what the packed step launches without the feature)
    b  ragged, drop_path_rate = --rate
    c  ragged, attention dropout p = --rate on every block
    d  ragged, both
    e  the same clips zero-padded to the longest through the fixed step, both regularisers: what a user who wants them had to run
  kernels  pa_attention_fwd_varlen_dropout / pa_attention_bwd_varlen_dropout against the plain packed entries on the kept tokens of
           that mix (H = 12, bf16, pre-scaled q, t = round(256 rate)): the same operands, launches alternating A B B A, each timed
           with device events, medians and min / max.  profiles/attn_dropout.txt has the fixed entries' ratios to read these against.

The ratios are what this measures, not targets.

    python tools/bench_varlen_regularize.py --out profiles/varlen_regularize.txt
"""
import argparse
import json
import os
import statistics
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from tools.bench_varlen_step import B, N_MELS, S_PATCHOUT_F, S_PATCHOUT_T, lengths, timed  # noqa: E402

H, D = 12, 768


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def kept_tokens(frames):
    """tokens per clip behind structured Patchout: cls, dist and (12 - rows) x (columns - 15) patches"""
    return [2 + (12 - S_PATCHOUT_F) * ((n - 16) // 10 + 1 - S_PATCHOUT_T) for n in frames]


def model(drop_path, attn_p):
    import passt_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(s_patchout_t=S_PATCHOUT_T, s_patchout_f=S_PATCHOUT_F, img_size=(N_MELS, 998), stride=10, num_classes=527,
                              embed_dim=D, depth=12, num_heads=H, distilled=True, drop_path_rate=drop_path).cuda().train()
    for blk in net.blocks:
        blk.attn.attn_drop.p = attn_p
    net.precision = "bf16"
    net.varlen_train = net.varlen_regularize = True
    return net


def bench_steps(a, frames):
    import torch

    from passt_amd.train import TrainStep
    T = max(frames)
    torch.manual_seed(0)
    x = (torch.rand(B, 1, N_MELS, T, device="cuda") * 2 - 1) * 1.5
    for i, n in enumerate(frames):
        x[i, :, :, n:] = 0.0                            # the padded variant reads the padding
    y = (torch.rand(B, 527, device="cuda") < 0.05).float()
    r = a.rate
    rates = dict(a_ragged_off=(0.0, 0.0), b_ragged_drop_path=(r, 0.0), c_ragged_attn_drop=(0.0, r), d_ragged_both=(r, r), e_padded_both=(r, r))
    steps = {k: TrainStep(model(*v), None, lr=2e-5, weight_decay=1e-4, use_mixup=True) for k, v in rates.items()}
    fns = {k: ((lambda ts=ts: ts.step(x, y)) if k.startswith("e_") else (lambda ts=ts: ts.step(x, y, lengths=frames))) for k, ts in steps.items()}
    ms = {k: [] for k in fns}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for rep in range(a.reps):
            order = list(fns) if rep % 2 == 0 else list(fns)[::-1]
            for k in order:
                ms[k].append(round(timed(fns[k], a.warmup, a.iters), 3))
    med = {k: statistics.median(v) for k, v in ms.items()}
    kept = kept_tokens(frames)
    rec = {"bench": "varlen_regularize_step", "precision": "bf16", "B": B, "rate": r, "frames_min": min(frames), "frames_max": T,
           "frames_mean": round(sum(frames) / B, 1), "ragged_tokens": sum(kept), "padded_tokens": B * max(kept), "iters_per_block": a.iters,
           "blocks": a.reps}
    for k in fns:
        rec[k + "_ms"], rec[k + "_blocks"] = med[k], ms[k]
    rec.update(a_spread_ms=round(max(ms["a_ragged_off"]) - min(ms["a_ragged_off"]), 3),
               b_over_a=round(med["b_ragged_drop_path"] / med["a_ragged_off"], 4), c_over_a=round(med["c_ragged_attn_drop"] / med["a_ragged_off"], 4),
               d_over_a=round(med["d_ragged_both"] / med["a_ragged_off"], 4), d_over_e=round(med["d_ragged_both"] / med["e_padded_both"], 4))
    emit(a, rec)


def bench_kernels(a, frames):
    import numpy as np
    import torch

    from passt_amd import ops
    ntok = kept_tokens(frames)
    total, max_N = sum(ntok), max(ntok)
    cu = torch.from_numpy(np.concatenate([[0], np.cumsum(ntok)]).astype(np.int32)).cuda()
    g = torch.Generator(device="cuda").manual_seed(1)
    scale = 64 ** -0.5
    qkv = (torch.rand(total, 3 * D, device="cuda", generator=g) * 2 - 1)
    qkv[:, :D] *= scale * ops.LOG2E
    qkv = qkv.bfloat16()
    d_o = (torch.rand(total, D, device="cuda", generator=g) * 2 - 1).bfloat16()
    seed = torch.tensor([0x1234567, 0x89abcde], dtype=torch.int32, device="cuda")
    t = ops.attn_drop_t(a.rate)
    PRE = ops.ATTN_Q_PRESCALED
    o, lse = ops.attention_fwd_varlen(qkv, cu, B, H, max_N, scale, flags=PRE)
    od, lsed = ops.attention_fwd_varlen_dropout(qkv, cu, B, H, max_N, scale, seed, 0, t, flags=PRE)
    assert torch.equal(lse, lsed)
    arms = {
        "fwd_plain": lambda: ops.attention_fwd_varlen(qkv, cu, B, H, max_N, scale, flags=PRE),
        "fwd_dropout": lambda: ops.attention_fwd_varlen_dropout(qkv, cu, B, H, max_N, scale, seed, 0, t, flags=PRE),
        "bwd_pair_plain": lambda: ops.attention_bwd_varlen(qkv, o, d_o, lse, cu, B, H, max_N, scale, flags=PRE),
        "bwd_pair_dropout": lambda: ops.attention_bwd_varlen_dropout(qkv, od, d_o, lse, cu, B, H, max_N, scale, seed, 0, t, flags=PRE),
    }

    def once(fn):
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
                us[tag].append(once(arms[tag]))
        mx, my = statistics.median(us[x]), statistics.median(us[y])
        emit(a, {"bench": "varlen_regularize_kernel", "pair": name, "B": B, "H": H, "tokens": total, "max_N": max_N, "dtype": "bf16", "t": t,
                 "launches_each": 2 * a.kiters, x + "_us": round(mx, 2), y + "_us": round(my, 2), "ratio": round(my / mx, 4),
                 x + "_min_max_us": [round(min(us[x]), 2), round(max(us[x]), 2)], y + "_min_max_us": [round(min(us[y]), 2), round(max(us[y]), 2)]})

    versus("packed_forward", "fwd_plain", "fwd_dropout")
    versus("packed_backward_pair", "bwd_pair_plain", "bwd_pair_dropout")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernels,step")
    ap.add_argument("--rate", type=float, default=0.1, help="drop_path_rate and attention dropout p of the active variants")
    ap.add_argument("--out", default="", help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=3, help="alternating blocks per variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="steps per block")
    ap.add_argument("--kiters", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_varlen_regularize: needs a HIP device (a timing taken anywhere else says nothing)")
    frames = lengths()
    if "kernels" in a.what:
        bench_kernels(a, frames)
    if "step" in a.what:
        bench_steps(a, frames)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of the fused training step on a ragged batch (TrainStep.step(x, y, lengths=)), passt_s size (768 / 12 / 12, stride 10, 128 mel
bands), bf16, one GPU: B = 64 spectrograms whose lengths are drawn uniformly between 2 s and 10 s (200 .. 998 frames at hop 320 / 32
kHz) under a fixed seed, structured Patchout 15 columns / 2 rows per clip, BCE, AdamW.  One JSON line per measurement.

  step      one training step, three ways on the same clips, in ONE process, the variants alternating block by block (a b c, c b a, ...):
    a  ragged   TrainStep.step(x, y, lengths=frames), mixup on: the packed kernel sequence over the clips' own tokens
    b  padded   TrainStep.step(x, y) on the clips zero-padded to the longest: how this batch went through the fused step before (it
                computes other numbers -- the padding is mixed in and attended to)
    c  dropin   net(x, lengths=frames) + BCE + backward + passt_amd.optim.AdamW, no mixup: the ragged path there was before
  mixup     the spectrogram pass in isolation on the batch's own buffer (B, 1, 128, T_max): pa_mixup_varlen with full-length clips and
            with the ragged lengths against pa_mixup, alternating, --reps blocks each; the spread of the pa_mixup blocks is the noise
            floor the full-length comparison is read against.  Bytes: what each pass has to move (read a, read c, write out), computed
            from the lengths.

    python tools/bench_varlen_step.py --out profiles/varlen_step.txt
"""
import argparse
import json
import os
import statistics
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B, N_MELS, HOP, SR = 64, 128, 320, 32000
S_PATCHOUT_T, S_PATCHOUT_F = 15, 2
SEED = 20


def lengths():
    """frames per clip: durations uniform in [2 s, 10 s) under a fixed seed, at most the model's 998 frames"""
    import numpy as np
    sec = np.random.RandomState(SEED).uniform(2.0, 10.0, B)
    return [min(998, 1 + (int(s * SR) - 1) // HOP) for s in sec]


def timed(fn, warmup, iters):
    """milliseconds per call: device events around ``iters`` calls, after ``warmup`` calls"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def model():
    import passt_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527, s_patchout_t=S_PATCHOUT_T,
                                  s_patchout_f=S_PATCHOUT_F).cuda().train()
    net.precision = "bf16"
    return net


def bench_steps(a, frames):
    import torch

    import passt_amd
    import passt_amd.optim
    from passt_amd.train import TrainStep
    T = max(frames)
    torch.manual_seed(0)
    x = (torch.rand(B, 1, N_MELS, T, device="cuda") * 2 - 1) * 1.5
    for i, n in enumerate(frames):
        x[i, :, :, n:] = 0.0                            # the padded variant reads the padding
    y = (torch.rand(B, 527, device="cuda") < 0.05).float()
    nets = [model() for _ in range(3)]
    nets[0].varlen_train = nets[2].varlen_train = True
    ragged = TrainStep(nets[0], None, lr=2e-5, weight_decay=1e-4, use_mixup=True)
    padded = TrainStep(nets[1], None, lr=2e-5, weight_decay=1e-4, use_mixup=True)
    opt = passt_amd.optim.AdamW(nets[2].parameters(), lr=2e-5, weight_decay=1e-4)

    def dropin():
        opt.zero_grad()
        logits, _ = nets[2](x, lengths=frames)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()
        opt.step()
    fns = dict(a_ragged=lambda: ragged.step(x, y, lengths=frames), b_padded=lambda: padded.step(x, y), c_dropin=dropin)
    ms = {k: [] for k in fns}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for r in range(a.reps):
            order = list(fns) if r % 2 == 0 else list(fns)[::-1]
            for k in order:
                ms[k].append(round(timed(fns[k], a.warmup, a.iters), 3))
    med = {k: statistics.median(v) for k, v in ms.items()}
    kept = [2 + (12 - S_PATCHOUT_F) * ((n - 16) // 10 + 1 - S_PATCHOUT_T) for n in frames]
    emit(a, {"bench": "varlen_step", "precision": "bf16", "B": B, "frames_min": min(frames), "frames_max": T, "frames_mean": round(sum(frames) / B, 1),
             "s_patchout_t": S_PATCHOUT_T, "s_patchout_f": S_PATCHOUT_F, "ragged_tokens": sum(kept), "padded_tokens": B * max(kept),
             "iters_per_block": a.iters, "blocks": a.reps, "a_ragged_trainstep_ms": med["a_ragged"], "a_blocks": ms["a_ragged"],
             "b_padded_trainstep_ms": med["b_padded"], "b_blocks": ms["b_padded"], "c_dropin_ragged_ms": med["c_dropin"], "c_blocks": ms["c_dropin"],
             "a_over_b": round(med["a_ragged"] / med["b_padded"], 4), "a_over_c": round(med["a_ragged"] / med["c_dropin"], 4)})


def bench_mixup(a, frames):
    import torch

    from passt_amd import _lib, ops
    from passt_amd.train import MIXUP_PAD
    T = max(frames)
    torch.manual_seed(1)
    x = (torch.rand(B, 1, N_MELS, T, device="cuda") * 2 - 1) * 1.5
    perm = torch.randperm(B).to(torch.int32).cuda()
    lam = (torch.rand(B) * 0.5 + 0.5).cuda()
    full, rag = torch.full((B,), T, dtype=torch.int32).cuda(), torch.tensor(frames, dtype=torch.int32).cuda()
    out = torch.empty_like(x)
    assert torch.equal(ops.mixup_varlen(x, full, perm, lam, MIXUP_PAD), ops.mixup(x, perm, lam)) or (N_MELS * T) % 4
    # the entries themselves, through ctypes on buffers made once: at ~10 us a call the wrappers' host work would be in the figure
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    xp, pp, lp, op, fp, rp = (t.data_ptr() for t in (x, perm, lam, out, full, rag))
    fns = dict(mixup=lambda: lib.pa_mixup(xp, pp, lp, op, B, N_MELS * T, st),
               varlen_full=lambda: lib.pa_mixup_varlen(xp, fp, pp, lp, MIXUP_PAD, op, B, N_MELS, T, st),
               varlen_ragged=lambda: lib.pa_mixup_varlen(xp, rp, pp, lp, MIXUP_PAD, op, B, N_MELS, T, st))
    assert all(fn() == 0 for fn in fns.values())
    us = {k: [] for k in fns}
    for r in range(a.reps):
        order = list(fns) if r % 2 == 0 else list(fns)[::-1]
        for k in order:
            us[k].append(round(1e3 * timed(fns[k], a.warmup, a.mixup_iters), 2))
    med = {k: statistics.median(v) for k, v in us.items()}
    pj = [frames[j] for j in perm.tolist()]
    bytes_full = 3 * B * N_MELS * T * 4
    bytes_rag = 4 * N_MELS * sum(n + min(n, m) + T for n, m in zip(frames, pj))      # read a, read the partner's part, write every cell
    spread = (max(us["mixup"]) - min(us["mixup"])) / med["mixup"]
    emit(a, {"bench": "varlen_step_mixup_kernel", "shape": [B, 1, N_MELS, T], "vector_path": (N_MELS * T) % 4 == 0, "iters_per_block": a.mixup_iters,
             "blocks": a.reps, "pa_mixup_us": med["mixup"], "pa_mixup_blocks": us["mixup"], "pa_mixup_spread": round(spread, 4),
             "varlen_full_us": med["varlen_full"], "varlen_full_blocks": us["varlen_full"], "varlen_ragged_us": med["varlen_ragged"],
             "varlen_ragged_blocks": us["varlen_ragged"], "full_over_mixup": round(med["varlen_full"] / med["mixup"], 4),
             "full_within_mixup_spread": med["varlen_full"] <= max(us["mixup"]),
             "bytes_full": bytes_full, "bytes_ragged": bytes_rag, "pa_mixup_TBps": round(bytes_full / med["mixup"] / 1e6, 3),
             "varlen_full_TBps": round(bytes_full / med["varlen_full"] / 1e6, 3), "varlen_ragged_TBps": round(bytes_rag / med["varlen_ragged"] / 1e6, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=["all", "step", "mixup"])
    ap.add_argument("--out", default="", help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=4, help="alternating blocks per variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="steps per block")
    ap.add_argument("--mixup-iters", type=int, default=200, help="kernel calls per block")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_varlen_step: needs a HIP device (a timing taken anywhere else says nothing)")
    frames = lengths()
    if a.what in ("all", "mixup"):
        bench_mixup(a, frames)
    if a.what in ("all", "step"):
        bench_steps(a, frames)


if __name__ == "__main__":
    main()

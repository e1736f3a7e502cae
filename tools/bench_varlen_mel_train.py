#!/usr/bin/env python
"""Cost of the training-mode front end on a ragged batch (mel.varlen_train), one GPU, a fixed mix of FSD50K-like clip lengths
(0.3 s ... 30 s at 32 kHz), AugmentMelSTFT(freqm=48, timem=192, fmin_aug_range=10, fmax_aug_range=2000).  One JSON line.

  Three ways to get the batch's spectrograms, measured in this process one after the other, each `--iters` times after `--warmup`:
    packed_train   mel.train(); mel.varlen_train = True; mel(wave, lengths=...)    one launch, every clip its own jitter and masks
    loop_train     for i: mel.train()(wave[i:i+1, :lengths[i]])                     what a user had to do before: one launch per clip
    packed_eval    mel.eval()(wave, lengths=...)                                    the packed launch without the per-clip table
  and, with --backward, the same three with a waveform that requires a gradient and a backward through the spectrograms.
  The figure that matters is packed_train against loop_train OF THE SAME BUILD; packed_eval shows what the per-clip table and its
  upload cost on top of the packed launch.  Times are wall-clock per call (host draws and uploads included), synchronised.

    python tools/bench_varlen_mel_train.py --backward --out profiles/varlen_mel_train.txt
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDS = [10.0, 2.3, 0.7, 30.0, 5.1, 1.2, 12.8, 0.3, 7.7, 3.4, 18.0, 0.9, 6.0, 2.0, 10.0, 4.4]
LENGTHS = [int(s * 32000) for s in SECONDS]


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="append the result line to this file")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--backward", action="store_true", help="also time forward + backward to the waveform")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch

    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mel = passt_amd.AugmentMelSTFT(freqm=48, timem=192, fmin_aug_range=10, fmax_aug_range=2000).cuda()
    mel.varlen_train = True
    B, L = len(LENGTHS), max(LENGTHS)
    wave = torch.rand(B, L, device="cuda") * 0.4 - 0.2
    clips = [wave[i:i + 1, :n].contiguous() for i, n in enumerate(LENGTHS)]

    def variants(grad):
        w = wave.clone().requires_grad_(grad)
        cs = [c.clone().requires_grad_(grad) for c in clips]

        def packed():
            spec, _ = mel(w, lengths=LENGTHS)
            if grad:
                w.grad = None
                spec.sum().backward()

        def loop():
            for c in cs:
                spec = mel(c)
                if grad:
                    c.grad = None
                    spec.sum().backward()
        return packed, loop

    rec = {"bench": "varlen_mel_train", "seconds": SECONDS, "samples": sum(LENGTHS), "padded_samples": B * L, "iters": a.iters}
    for grad in ([False, True] if a.backward else [False]):
        packed, loop = variants(grad)
        tag = "fwd_bwd" if grad else "fwd"
        mel.train()
        pt = statistics.median(timed(packed, a.warmup, a.iters))
        lt = statistics.median(timed(loop, a.warmup, a.iters))
        mel.eval()
        pe = statistics.median(timed(packed, a.warmup, a.iters))
        rec.update({f"{tag}_packed_train_ms": round(pt, 3), f"{tag}_loop_train_ms": round(lt, 3), f"{tag}_packed_eval_ms": round(pe, 3),
                    f"{tag}_loop_over_packed": round(lt / pt, 3), f"{tag}_train_over_eval": round(pt / pe, 3)})
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

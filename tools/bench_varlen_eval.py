#!/usr/bin/env python
"""Eval forward over clips of DIFFERENT lengths, passt_s size, bf16, one GPU: three ways to run the same eight clips
(998 / 437 / 1203 / 16 / 251 / 640 / 998 / 33 frames):

  (a) loop    : one batch-1 forward per clip, cropped to its length -- the reference's way (ex_fsd50k.py:53-56)
  (b) packed  : net(x, lengths=...) -- one packed kernel sequence over the sum of the clips' tokens
  (c) padded  : the uniform batch of 8 clips padded to the longest -- WRONG numbers (padding is attended to), for orientation only:
                same launch count as (b), strictly more arithmetic through the fixed-length kernels

Each variant: warm-up, then `--rounds` measurements bracketed by HIP events in ABBA order (a b c c b a ...), median and min..max
per variant.  One JSON line.  `--only loop` runs (a) alone (it needs no `lengths` support: usable on an older checkout).

    python tools/bench_varlen_eval.py [--rounds 20] [--only loop]
"""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import passt_amd  # noqa: E402

LENGTHS = [998, 437, 1203, 16, 251, 640, 998, 33]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="comma list out of loop,packed,padded (default: all)")
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527, s_patchout_t=0,
                                  s_patchout_f=0).to(dev).eval()
    net.precision = "bf16"
    x = (torch.rand(len(LENGTHS), 1, 128, max(LENGTHS), device=dev) * 2 - 1) * 1.5
    clips = [x[i:i + 1, :, :, :n].contiguous() for i, n in enumerate(LENGTHS)]

    def loop():
        return [net(c) for c in clips]

    def packed():
        return net(x, lengths=LENGTHS)

    def padded():
        return net(x)

    variants = {"loop": loop, "packed": packed, "padded": padded}
    names = [n for n in variants if not a.only or n in a.only.split(",")]
    times = {n: [] for n in names}
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for n in names:
            for _ in range(a.warmup):
                variants[n]()
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for n in (names if r % 2 == 0 else names[::-1]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                variants[n]()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1))
    out = {"metric": "ms per 8 clips, eval forward passt_s bf16, lengths " + "/".join(map(str, LENGTHS)), "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    for n in names:
        t = sorted(times[n])
        out[n] = {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

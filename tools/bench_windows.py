#!/usr/bin/env python
"""Sliding-window inference over ONE long recording, passt_s size (768 / 12 / 12), bf16, one GPU: 60 000 frames (10 minutes at hop
320), window 998, hop 499 -> 120 windows, 142 800 packed tokens.  Three ways to get the same 120 per-window outputs:

  (a) loop     : one batch-1 forward per window slice -- what a caller of the reference does
  (b) unfold   : copy the windows into a (120, 1, 128, 998) batch, then net(unfolded, lengths=) -- today's packed path; the copy
                 is timed with it (it is part of what the caller has to do)
  (c) windows  : net.forward_windows(x, pool=None) -- the window gather reads the recording in place; alone, and with
                 max_tokens = 32 * 1190 (four packed passes)

(c) runs the same trunk kernels on the same rows as (b), so it is expected to equal it within run-to-run noise; the gap is reported,
not asserted.  Each variant: warm-up, then `--rounds` measurements bracketed by HIP events, the variants alternating in ABBA order
inside one process; median and min..max per variant.  The outputs of the variants are compared first (bit for bit where the
contract says so).  Also measured here, because the tests' pooling bound needs it: the largest error of the pool kernel's f32 sigmoid
against float64 torch.sigmoid over tests/windows_cases.sigmoid_family().  One JSON line; --out also writes a text report.

    python tools/bench_windows.py [--rounds 10] [--out profiles/windows.txt]
"""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import passt_amd  # noqa: E402
from passt_amd import ops  # noqa: E402

FRAMES, WINDOW, HOP = 60000, 998, 499


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527, s_patchout_t=0,
                                  s_patchout_f=0).to(dev).eval()
    net.precision = "bf16"
    x = (torch.rand(1, 1, 128, FRAMES, device=dev) * 2 - 1) * 1.5
    g = passt_amd.window_geometry([FRAMES], WINDOW, HOP, "align", 16, 10, 12)
    starts, M = g["win_t0"].tolist(), int(g["row_f"].size)
    assert len(starts) == 120 and M == 142800
    lengths = [WINDOW] * len(starts)

    def loop():
        return [net(x[:, :, :, s:s + WINDOW].contiguous()) for s in starts]

    def unfold():
        u = torch.stack([x[0, :, :, s:s + WINDOW] for s in starts])
        return net(u, lengths=lengths)

    def windows():
        return net.forward_windows(x, window=WINDOW, hop=HOP, pool=None)

    def windows_chunked():
        return net.forward_windows(x, window=WINDOW, hop=HOP, pool=None, max_tokens=32 * 1190)

    variants = {"loop": loop, "unfold": unfold, "windows": windows, "windows_chunked": windows_chunked}
    names = list(variants)
    times = {n: [] for n in names}
    out = {"metric": f"ms per recording of {FRAMES} frames ({len(starts)} windows of {WINDOW}, hop {HOP}, {M} tokens), eval forward passt_s bf16",
           "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # the same numbers first
        lo_b, fe_b = unfold()
        lo_c, fe_c, _ = windows()
        lo_d, _, _ = windows_chunked()
        lo_a = torch.cat([r[0] for r in loop()])
        scale = float(lo_b.abs().max())
        out["windows_equals_unfold_bitwise"] = bool(torch.equal(lo_b, lo_c) and torch.equal(fe_b, fe_c))
        out["chunked_vs_windows_rel"] = float((lo_d - lo_c).abs().max()) / scale
        out["loop_vs_windows_rel"] = float((lo_a - lo_c).abs().max()) / scale
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
    for n in names:
        t = sorted(times[n])
        out[n] = {"median_ms": round(t[len(t) // 2], 3), "min_ms": round(t[0], 3), "max_ms": round(t[-1], 3)}
    out["windows_over_unfold"] = round(out["windows"]["median_ms"] / out["unfold"]["median_ms"], 4)

    # the pool kernel's sigmoid against float64: one row per "recording", so the mean of one term is the sigmoid itself
    from tests import windows_cases as W
    z = W.sigmoid_family()
    got = ops.window_pool(z.view(-1, 1).to(dev), list(range(z.numel() + 1)), "mean", "sigmoid").view(-1).cpu()
    err = (got.double() - torch.sigmoid(z.double())).abs()
    out["sigmoid"] = {"logits": z.numel(), "largest_error": float(err.max()), "at_logit": float(z[err.argmax()]),
                      "allowance_in_tests": W.SIGMOID_ALLOWANCE}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(__doc__.split("\n\n    python")[0].strip() + "\n\n")
            f.write(f"device: {out['device']}; {a.rounds} rounds after {a.warmup} warm-up calls per variant, ABBA order, HIP events\n\n")
            for n in names:
                f.write(f"  {n:16s} median {out[n]['median_ms']:9.3f} ms   min {out[n]['min_ms']:9.3f}   max {out[n]['max_ms']:9.3f}\n")
            f.write(f"\n  windows / unfold (medians): {out['windows_over_unfold']}\n")
            f.write(f"  windows == unfold bit for bit: {out['windows_equals_unfold_bitwise']}\n")
            f.write(f"  chunked vs windows, largest logit difference / largest logit: {out['chunked_vs_windows_rel']:.3e}\n")
            f.write(f"  loop vs windows,    largest logit difference / largest logit: {out['loop_vs_windows_rel']:.3e}\n\n")
            s = out["sigmoid"]
            f.write(f"pa_window_pool's sigmoid against float64 torch.sigmoid over {s['logits']} logits (tests/windows_cases.sigmoid_family):\n"
                    f"  largest error {s['largest_error']:.4e} at logit {s['at_logit']:.6f}; the tests allow twice the measured figure per term: "
                    f"{s['allowance_in_tests']:.4e} (condition: below 1e-6)\n")


if __name__ == "__main__":
    main()

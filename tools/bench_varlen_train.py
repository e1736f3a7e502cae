#!/usr/bin/env python
"""Cost of Patchout training on a ragged batch (net.varlen_train), passt_s size (768 / 12 / 12, stride 10, 128 mel bands), bf16, one
GPU, a fixed mix of clip lengths (998/437/251/640/998/333/760/520 frames), structured Patchout 15 columns / 2 rows per clip.  One JSON
line per measurement.

  One training step = forward + backward through the autograd path (every parameter trainable, a BCE-shaped loss on the logits), one
  variant per process:
    packed   A: net(x, lengths=...) in training mode with net.varlen_train = True -- one packed kernel sequence over the kept tokens
    padded   B: the same clips padded to the longest, one uniform batch through the fixed path (what a user had to do before; it
                computes other numbers -- the padding is attended to -- and is the baseline, from the parent checkout: --root / --against)
  --against DIR: A from this checkout and B from DIR in fresh child processes, alternating ABAB... --reps times; medians, all values and
  the ratio A / B.  Without --against: the one variant named by --variant, in this process.

    python tools/bench_varlen_train.py --against ../parent_checkout --out profiles/varlen_train.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [998, 437, 251, 640, 998, 333, 760, 520]
S_PATCHOUT_T, S_PATCHOUT_F = 15, 2


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
    return ms


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def run_child(a):
    import torch
    sys.path.insert(0, a.root)
    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527, s_patchout_t=S_PATCHOUT_T,
                                  s_patchout_f=S_PATCHOUT_F).cuda().train()
    net.precision = "bf16"
    B, T = len(LENGTHS), max(LENGTHS)
    x = (torch.rand(B, 1, 128, T, device="cuda") * 2 - 1) * 1.5
    for i, n in enumerate(LENGTHS):
        x[i, :, :, n:] = 0.0                            # the padded variant reads the padding
    y = (torch.rand(B, 527, device="cuda") < 0.05).float()
    if a.variant == "packed":
        net.varlen_train = True

        def step():
            net.zero_grad(set_to_none=True)
            logits, _ = net(x, lengths=LENGTHS)
            torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()
    else:
        def step():
            net.zero_grad(set_to_none=True)
            logits, _ = net(x)
            torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ms = timed(step, a.warmup, a.iters)
    print(json.dumps({"variant": a.variant, "root": os.path.abspath(a.root), "ms_median": round(statistics.median(ms), 3),
                      "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}), flush=True)


def run_driver(a):
    def child(root, variant):
        cmd = [sys.executable, os.path.abspath(__file__), "--variant", variant, "--root", root, "--warmup", str(a.warmup),
               "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"{variant} step in {root} failed with exit status {r.returncode}")
        return json.loads(r.stdout.strip().splitlines()[-1])["ms_median"]

    A, Bv = [], []
    for r in range(a.reps):
        order = [(a.root, "packed", A), (a.against, "padded", Bv)]
        for root, variant, sink in (order if r % 2 == 0 else order[::-1]):
            sink.append(child(root, variant))
    mA, mB = statistics.median(A), statistics.median(Bv)
    kept = [2 + (12 - S_PATCHOUT_F) * ((n - 16) // 10 + 1 - S_PATCHOUT_T) for n in LENGTHS]
    emit(a, {"bench": "varlen_train_step", "precision": "bf16", "lengths": LENGTHS, "s_patchout_t": S_PATCHOUT_T, "s_patchout_f": S_PATCHOUT_F,
             "packed_tokens": sum(kept), "padded_tokens": len(LENGTHS) * max(kept), "iters_per_rep": a.iters, "A_packed_ms": mA, "A_per_rep": A,
             "B_padded_other_checkout_ms": mB, "B_per_rep": Bv, "ratio_A_over_B": round(mA / mB, 4), "speedup_B_over_A": round(mB / mA, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="packed", choices=["packed", "padded"])
    ap.add_argument("--root", default=HERE, help="checkout to import passt_amd from")
    ap.add_argument("--against", default="", help="another checkout whose padded step is measured alternately with this one's packed step")
    ap.add_argument("--out", default="", help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.against:
        run_driver(a)
    else:
        run_child(a)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Cost of the gradient w.r.t. the input spectrogram, passt_s size (768 / 12 / 12, stride 10, 128 x 998, no Patchout), bf16, one GPU.
One JSON line per configuration.

  fold   the fold kernel alone (pa_patch_input_bwd) at B = 64 on bf16 dcols: median time and the bandwidth it reaches on the bytes
         it has to move (B * Np * 256 * 2 read + B * F * T * 4 written) over bench_kernels.py's HBM peak
  step   forward + backward of one batch in eval mode, one of two variants:
           lossnet     every parameter frozen, x.requires_grad: no weight gradient, input gradient computed
           train_nodx  parameters trainable, x without gradient: every weight gradient, no input gradient (all an older checkout
                       can do: run this file with --root <that checkout>)
         --against DIR: both variants in child processes, this checkout's lossnet and DIR's train_nodx alternating --reps times
         (ABAB..., a fresh process each, so neither inherits the other's warm caches); reports both medians and their ratio

    python tools/bench_input_grad.py fold
    python tools/bench_input_grad.py step --batch 64 --against ../parent_checkout
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0           # bench_kernels.py HBM_PEAK
INNER = 20                      # fold: calls per timed bracket (a call is two short launches)


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


def run_fold(a):
    import torch
    sys.path.insert(0, a.root)
    from passt_amd import ops
    B, F, T, P, s = a.batch, 128, 998, 16, 10
    Fg, Tg = (F - P) // s + 1, (T - P) // s + 1
    Np = Fg * Tg
    idx = torch.arange(Np, dtype=torch.int32)
    pf, pt = (idx // Tg).cuda(), (idx % Tg).cuda()
    dcols = (torch.rand(B * Np, P * P, device="cuda") * 2 - 1).bfloat16()
    out = torch.empty(B, 1, F, T, device="cuda")
    reps = []
    for _ in range(a.reps):
        reps.append(statistics.median(timed(lambda: [ops.patch_input_bwd(dcols, pf, pt, B, F, T, P, s, s, out=out) for _ in range(INNER)],
                                            a.warmup, a.iters)) / INNER)
    ms = statistics.median(reps)
    bytes_ = B * Np * P * P * 2 + B * F * T * 4
    print(json.dumps({"bench": "patch_input_bwd", "B": B, "F": F, "T": T, "stride": s, "Np": Np, "dcols": "bf16",
                      "includes": "the grid -> slot table launch and the fold kernel",
                      "ms_median": round(ms, 4), "ms_per_rep": [round(v, 4) for v in reps], "bytes": bytes_,
                      "gb_per_s": round(bytes_ / ms / 1e6, 1), "frac_hbm_peak": round(bytes_ / ms / 1e6 / HBM_PEAK_GBS, 4)}), flush=True)


def run_step_child(a):
    import torch
    sys.path.insert(0, a.root)
    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527, s_patchout_t=0,
                                  s_patchout_f=0).cuda().eval()
    net.precision = "bf16"
    lossnet = a.variant == "lossnet"
    net.requires_grad_(not lossnet)
    x = ((torch.rand(a.batch, 1, 128, 998, device="cuda") * 2 - 1) * 1.5).requires_grad_(lossnet)
    w, v = torch.rand(a.batch, 768, device="cuda"), torch.rand(a.batch, 527, device="cuda")

    def step():
        x.grad = None
        for p in net.parameters():
            p.grad = None
        logits, feat = net(x)
        ((feat * w).sum() + (logits * v).sum()).backward()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ms = timed(step, a.warmup, a.iters)
    print(json.dumps({"variant": a.variant, "root": os.path.abspath(a.root), "B": a.batch, "ms_median": round(statistics.median(ms), 3),
                      "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}),
          flush=True)


def run_step_driver(a):
    def child(root, variant):
        cmd = [sys.executable, os.path.abspath(__file__), "step", "--batch", str(a.batch), "--variant", variant, "--root", root,
               "--warmup", str(a.warmup), "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"{variant} step in {root} failed with exit status {r.returncode}")
        return json.loads(r.stdout.strip().splitlines()[-1])

    new, old = [], []
    for r in range(a.reps):
        order = [(a.root, "lossnet", new), (a.against, "train_nodx", old)]
        for root, variant, sink in (order if r % 2 == 0 else order[::-1]):
            sink.append(child(root, variant))
    m_new, m_old = statistics.median(v["ms_median"] for v in new), statistics.median(v["ms_median"] for v in old)
    print(json.dumps({"bench": "loss_network_step", "B": a.batch, "precision": "bf16", "tokens": 1190,
                      "lossnet_ms": m_new, "lossnet_ms_per_rep": [v["ms_median"] for v in new],
                      "train_nodx_other_checkout_ms": m_old, "train_nodx_ms_per_rep": [v["ms_median"] for v in old],
                      "ratio_lossnet_over_train_nodx": round(m_new / m_old, 4),
                      "peak_mem_gb": {"lossnet": new[0]["peak_mem_gb"], "train_nodx": old[0]["peak_mem_gb"]}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["fold", "step"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--variant", default="lossnet", choices=["lossnet", "train_nodx"])
    ap.add_argument("--root", default=HERE, help="checkout to import passt_amd from")
    ap.add_argument("--against", default="", help="step: another checkout whose train_nodx step is measured alternately")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.what == "fold":
        run_fold(a)
    elif a.against:
        run_step_driver(a)
    else:
        run_step_child(a)


if __name__ == "__main__":
    main()

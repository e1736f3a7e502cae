#!/usr/bin/env python
"""Cost of gradients through the ragged-batch forward (net.varlen_grad), passt_s size (768 / 12 / 12, stride 10, 128 mel bands), bf16,
one GPU, the clip mix of tools/bench_varlen_eval.py (998/437/1203/16/251/640/998/33 frames).  One JSON line per measurement.

  step   forward + backward to x.grad of a frozen network (a loss network), one variant per process:
           packed   A: net(x, lengths=...) with net.varlen_grad = True -- one packed kernel sequence
           loop     B: eight batch-1 forward + backward calls on the cropped clips (all an older checkout can do for ragged clips: run
                       with --root <that checkout>)
           padded   C: one uniform batch padded to the longest clip (computes other numbers: context only)
         --against DIR: A from this checkout and B, C from DIR in fresh child processes, alternating ABAB... --reps times; medians, all
         values and the ratio A / B
  attn   the packed attention backward alone for the mix at H = 12: microseconds, TF/s on the executed FLOPs (10 * 64 * H * sum N_b^2),
         how many of the launched workgroups have work; beside it the fixed-length kernel pair at (8, 12, 474) through both entry points

    python tools/bench_varlen_grad.py step --against ../parent_checkout --out profiles/varlen_grad.txt
    python tools/bench_varlen_grad.py attn --out profiles/varlen_grad.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [998, 437, 1203, 16, 251, 640, 998, 33]


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


def run_step_child(a):
    import torch
    sys.path.insert(0, a.root)
    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, n_classes=527, s_patchout_t=0, s_patchout_f=0).cuda().eval()
    net.precision = "bf16"
    net.requires_grad_(False)
    B, T = len(LENGTHS), max(LENGTHS)
    x = ((torch.rand(B, 1, 128, T, device="cuda") * 2 - 1) * 1.5)
    w, v = torch.rand(B, 768, device="cuda"), torch.rand(B, 527, device="cuda")
    if a.variant == "packed":
        net.varlen_grad = True
        xg = x.requires_grad_()

        def step():
            xg.grad = None
            logits, feat = net(xg, lengths=LENGTHS)
            ((feat * w).sum() + (logits * v).sum()).backward()
    elif a.variant == "loop":
        clips = [x[i:i + 1, :, :, :n].contiguous().requires_grad_() for i, n in enumerate(LENGTHS)]

        def step():
            for i, c in enumerate(clips):
                c.grad = None
                logits, feat = net(c)
                ((feat * w[i:i + 1]).sum() + (logits * v[i:i + 1]).sum()).backward()
    else:
        xg = x.requires_grad_()

        def step():
            xg.grad = None
            logits, feat = net(xg)
            ((feat * w).sum() + (logits * v).sum()).backward()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ms = timed(step, a.warmup, a.iters)
    print(json.dumps({"variant": a.variant, "root": os.path.abspath(a.root), "ms_median": round(statistics.median(ms), 3),
                      "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}), flush=True)


def run_step_driver(a):
    def child(root, variant):
        cmd = [sys.executable, os.path.abspath(__file__), "step", "--variant", variant, "--root", root, "--warmup", str(a.warmup),
               "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
        if r.returncode:
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"{variant} step in {root} failed with exit status {r.returncode}")
        return json.loads(r.stdout.strip().splitlines()[-1])["ms_median"]

    A, Bv, Cv = [], [], []
    for r in range(a.reps):
        order = [(a.root, "packed", A), (a.against, "loop", Bv)]
        for root, variant, sink in (order if r % 2 == 0 else order[::-1]):
            sink.append(child(root, variant))
        Cv.append(child(a.against, "padded"))
    mA, mB, mC = (statistics.median(v) for v in (A, Bv, Cv))
    emit(a, {"bench": "varlen_loss_network_step", "precision": "bf16", "lengths": LENGTHS, "iters_per_rep": a.iters,
             "A_packed_ms": mA, "A_per_rep": A, "B_loop_other_checkout_ms": mB, "B_per_rep": Bv, "C_padded_other_checkout_ms": mC,
             "C_per_rep": Cv, "ratio_A_over_B": round(mA / mB, 4), "speedup_B_over_A": round(mB / mA, 3)})


def run_attn(a):
    import numpy as np
    import torch
    sys.path.insert(0, a.root)
    from passt_amd import ops
    H, D, scale = 12, 768, 0.125
    P, s, Fg, Tpe = 16, 10, 12, 99
    lens = [2 + Fg * min((n - P) // s + 1, Tpe) for n in LENGTHS]
    B, total, max_N = len(lens), sum(lens), max(lens)
    cu = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device="cuda")
    flags = ops.ATTN_Q_PRESCALED

    def case(total_rows):
        qkv = ((torch.rand(total_rows, 3 * D, device="cuda") * 2 - 1) * 1.5).bfloat16()
        d_o = (torch.rand(total_rows, D, device="cuda") * 2 - 1).bfloat16()
        return qkv, d_o

    qkv, d_o = case(total)
    o, lse = ops.attention_fwd_varlen(qkv, cu, B, H, max_N, scale, flags=flags)
    reps = [statistics.median(timed(lambda: ops.attention_bwd_varlen(qkv, o, d_o, lse, cu, B, H, max_N, scale, flags=flags), a.warmup, a.iters))
            for _ in range(a.reps)]
    ms = statistics.median(reps)
    flops = 10.0 * 64 * H * sum(n * n for n in lens)
    nblk = -(-max_N // 128)
    emit(a, {"bench": "attention_bwd_varlen", "tokens": lens, "H": H, "dtype": "bf16", "us_median": round(ms * 1e3, 1),
             "us_per_rep": [round(v * 1e3, 1) for v in reps], "executed_tflops": round(flops / ms / 1e9, 1),
             "workgroups_per_kernel": nblk * 8 * ((B * H + 7) // 8), "workgroups_with_work": H * sum(-(-n // 128) for n in lens)})
    # the fixed-length pair through both entry points (bit-identical results)
    Bf, N = 8, 474
    qkv, d_o = case(Bf * N)
    o, lse = ops.attention_fwd(qkv, Bf, H, N, scale, flags=flags)
    lse_p = lse.view(Bf, H, N).permute(1, 0, 2).reshape(H, Bf * N).contiguous()
    cuf = torch.arange(Bf + 1, dtype=torch.int32, device="cuda") * N
    fx, pk = [], []
    for _ in range(a.reps):
        fx.append(statistics.median(timed(lambda: ops.attention_bwd(qkv, o, d_o, lse, Bf, H, N, scale, flags=flags | ops.ATTN_BWD_TWO_PASS),
                                          a.warmup, a.iters)))
        pk.append(statistics.median(timed(lambda: ops.attention_bwd_varlen(qkv, o, d_o, lse_p, cuf, Bf, H, N, scale, flags=flags), a.warmup, a.iters)))
    emit(a, {"bench": "attention_bwd_pair_equal_lengths", "B": Bf, "H": H, "N": N, "dtype": "bf16",
             "fixed_entry_us": [round(v * 1e3, 1) for v in fx], "packed_entry_us": [round(v * 1e3, 1) for v in pk],
             "fixed_entry_us_median": round(statistics.median(fx) * 1e3, 1), "packed_entry_us_median": round(statistics.median(pk) * 1e3, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["step", "attn"])
    ap.add_argument("--variant", default="packed", choices=["packed", "loop", "padded"])
    ap.add_argument("--root", default=HERE, help="checkout to import passt_amd from")
    ap.add_argument("--against", default="", help="step: another checkout whose loop / padded steps are measured alternately")
    ap.add_argument("--out", default="", help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.what == "attn":
        run_attn(a)
    elif a.against:
        run_step_driver(a)
    else:
        run_step_child(a)


if __name__ == "__main__":
    main()

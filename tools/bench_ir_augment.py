#!/usr/bin/env python
"""Cost of the device-impulse-response convolution (pa_wave_ir_convolve), one GPU: B = 64 clips of 10 s (L = 320 000), banks of 10 IRs
of 256 / 2048 / 8192 taps, an IR drawn for every clip (hit rate 1.0) or for every other one (0.5).  Two variants, each in fresh child
processes, alternating, --reps times; medians of HIP-event brackets:

  kernel    ops.wave_ir_convolve (spectra prepared once, outside the timed region, as IRBank does)
  torchfft  the yardstick: the same convolution as torch ops on the same GPU -- rfft of the hit clips at 2^19 points, product with the
            (prepared) rfft of their IRs, irfft, cut to L; rows without an IR are copied

Per case: time, the bytes the convolution has to move (x read once, out written once: 2 B L 4; the spectra and tables are small and
re-read from the caches) over time as a fraction of bench_kernels.py's HBM peak, and yardstick / kernel.  One JSON line per case, and a
table (to --out as well, e.g. profiles/ir_augment.txt).

    python tools/bench_ir_augment.py run --out profiles/ir_augment.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0           # bench_kernels.py HBM_PEAK
L10S, N_IR = 320000, 10
TAPS, HITS = (256, 2048, 8192), (1.0, 0.5)
YARD_N = 1 << 19                # >= L + 8192 - 1


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


def child(a):
    import torch
    sys.path.insert(0, HERE)
    from passt_amd import ops
    torch.manual_seed(0)
    B, L = a.batch, L10S
    x = (torch.rand(B, L, device="cuda") * 2 - 1) * 0.3
    for taps in TAPS:
        irs = torch.randn(N_IR, taps, device="cuda") * torch.exp(-6.9 * torch.arange(taps, device="cuda") / taps)
        for hit in HITS:
            idx = torch.arange(B, device="cuda", dtype=torch.int32) % N_IR
            if hit < 1.0:
                idx[1::2] = -1
            if a.variant == "kernel":
                bank = ops.ir_bank_prepare(irs)
                fn = lambda: ops.wave_ir_convolve(x, L, None, idx, bank)                                        # noqa: E731
            else:
                Hf = torch.fft.rfft(irs, YARD_N)
                rows = torch.nonzero(idx >= 0).flatten()
                sel = idx[rows].long()

                def fn():
                    out = x.clone() if hit < 1.0 else torch.empty_like(x)
                    out[rows] = torch.fft.irfft(torch.fft.rfft(x[rows], YARD_N) * Hf[sel], YARD_N)[:, :L]
                    return out
            ms = timed(fn, a.warmup, a.iters)
            print(json.dumps({"variant": a.variant, "taps": taps, "hit": hit, "batch": B, "median_ms": statistics.median(ms), "min_ms": min(ms)}),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "child"])
    ap.add_argument("--variant")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "child":
        return child(a)
    res = {}
    for _ in range(a.reps):
        for v in ("kernel", "torchfft"):                   # ABAB..., a fresh process each
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--variant", v, "--batch", str(a.batch), "--warmup",
                                str(a.warmup), "--iters", str(a.iters)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                sys.exit(r.returncode)                     # nothing more is started on the GPU after a failure
            for line in r.stdout.strip().splitlines():
                d = json.loads(line)
                res.setdefault((d["taps"], d["hit"], v), []).append(d["median_ms"])
    import torch
    lines = [f"# tools/bench_ir_augment.py run: {torch.cuda.get_device_name(0)}, B = {a.batch}, L = {L10S}, {N_IR} IRs per bank, "
             f"{a.reps} fresh processes per variant (alternating), {a.iters} timed calls each, medians",
             f"# bytes = 2 B L 4 = {2 * a.batch * L10S * 4 / 1e6:.1f} MB; HBM peak {HBM_PEAK_GBS:.0f} GB/s (bench_kernels.py)",
             f"{'taps':>5} {'hit':>4} {'kernel us':>10} {'GB/s':>7} {'of peak':>8} {'torch.fft us':>13} {'yardstick/kernel':>17}"]
    nbytes = 2.0 * a.batch * L10S * 4
    for taps in TAPS:
        for hit in HITS:
            k, y = statistics.median(res[(taps, hit, "kernel")]), statistics.median(res[(taps, hit, "torchfft")])
            gbs = nbytes / (k * 1e-3) / 1e9
            print(json.dumps({"taps": taps, "hit": hit, "batch": a.batch, "kernel_ms": k, "kernel_runs": res[(taps, hit, "kernel")],
                              "torchfft_ms": y, "torchfft_runs": res[(taps, hit, "torchfft")], "bytes": nbytes,
                              "fraction_of_hbm_peak": gbs / HBM_PEAK_GBS, "ratio_torchfft_over_kernel": y / k}))
            lines.append(f"{taps:>5} {hit:>4} {k * 1e3:>10.1f} {gbs:>7.0f} {gbs / HBM_PEAK_GBS:>8.3f} {y * 1e3:>13.1f} {y / k:>17.2f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

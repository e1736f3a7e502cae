#!/usr/bin/env python
"""Cost of the gradient w.r.t. the waveform through the fused front end, one GPU.  One JSON line per measurement; every mode runs
its variants in fresh child processes, alternating, --reps times each, and reports medians (HIP-event brackets).

  kernel    pa_mel_frontend_bwd alone at B x 10 s next to pa_mel_frontend_fwd: time, bytes it has to move (wave read + dout read +
            dwave written), fraction of bench_kernels.py's HBM peak
  pair      forward + backward of the front end, loss (mel * g).sum(): the fused pair against the yardstick -- what a user had to
            write before this gradient existed, a torch-op composition on the same GPU (conv1d pre-emphasis, torch.stft, dense
            filterbank matmul, log; autograd)
  lossnet   wave -> mel -> frozen passt_s-size network (bf16, 998 frames, 1190 tokens) -> backward, once to wave.grad and once
            stopping at spec.grad (the spectrogram as the leaf)

    python tools/bench_wave_grad.py kernel --batch 64
    python tools/bench_wave_grad.py pair --batch 64
    python tools/bench_wave_grad.py lossnet --batch 64
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
L10S = 320000


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


def front_end():
    import passt_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return passt_amd.AugmentMelSTFT(fmin_aug_range=10, fmax_aug_range=2000, freqm=0, timem=0).cuda().eval()


def torch_front_end(mel):
    """The yardstick: the reference's chain as torch ops on the GPU, dense filterbank from the oracle."""
    import torch
    from oracle import passt_oracle as O
    basis, _ = O.kaldi_get_mel_banks(128, 1024, 32000, 0.0, 15000, 100.0, -500.0, 1.0)
    basis = torch.nn.functional.pad(basis, (0, 1), value=0.0).float().cuda()
    window = mel.window
    pre = mel.preemphasis_coefficient

    def fwd(x):
        y = torch.nn.functional.conv1d(x.unsqueeze(1), pre).squeeze(1)
        s = torch.stft(y, 1024, hop_length=320, win_length=800, center=True, normalized=False, window=window, return_complex=True)
        p = s.real ** 2 + s.imag ** 2
        return (torch.log(torch.matmul(basis, p) + 0.00001) + 4.5) / 5.0
    return fwd


def child(a):
    import torch
    sys.path.insert(0, HERE)
    from passt_amd import ops
    from passt_amd._lib import MelParams
    torch.manual_seed(0)
    mel = front_end()
    B = a.batch
    wave = (torch.rand(B, L10S, device="cuda") * 2 - 1) * 0.3
    T = 1 + (L10S - 1) // 320
    if a.variant in ("k_fwd", "k_bwd"):
        import math
        p = MelParams()
        p.n_fft, p.hop, p.n_mels, p.n_frames, p.preemph = 1024, 320, 128, T, 0.97
        lo, hi = 0.0, 1127.0 * math.log(1.0 + 15000 / 700.0)
        p.mel_low, p.inv_mel_delta = lo, 129 / (hi - lo)
        p.log_eps, p.out_add, p.out_scale = 0.00001, 4.5, 0.2
        g = torch.rand(B, 128, T, device="cuda") * 2 - 1
        if a.variant == "k_fwd":
            fn = lambda: ops.mel_frontend(wave, mel._window_padded, mel._bin_mel, mel._twiddle, p)                # noqa: E731
        else:
            fn = lambda: ops.mel_frontend_bwd(wave, mel._window_padded, mel._bin_mel, mel._twiddle, p, g)        # noqa: E731
    elif a.variant in ("pair_fused", "pair_torch"):
        g = torch.rand(B, 128, T, device="cuda") * 2 - 1
        f = mel if a.variant == "pair_fused" else torch_front_end(mel)
        w = wave.clone().requires_grad_()

        def fn():
            w.grad = None
            (f(w) * g).sum().backward()
    else:
        import passt_amd
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = passt_amd.PaSST(img_size=(128, 998), stride=10, num_classes=527, embed_dim=768, depth=12, num_heads=12,
                                  distilled=True, u_patchout=0, s_patchout_t=0, s_patchout_f=0).cuda().eval()
        net.precision = "bf16"
        net.requires_grad_(False)
        wv = wave[:, :998 * 320].contiguous()
        to_wave = a.variant == "ln_wave"
        w = wv.clone().requires_grad_(to_wave)

        def fn():
            w.grad = None
            spec = mel(w)
            if not to_wave:
                spec = spec.detach().requires_grad_()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                logits, feat = net(spec[:, None])
            (logits.sum() + feat.sum()).backward()
    ms = timed(fn, a.warmup, a.iters)
    print(json.dumps({"variant": a.variant, "batch": B, "median_ms": statistics.median(ms), "min_ms": min(ms)}))


MODES = {"kernel": ("k_fwd", "k_bwd"), "pair": ("pair_fused", "pair_torch"), "lossnet": ("ln_wave", "ln_spec")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=list(MODES) + ["child"])
    ap.add_argument("--variant")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.mode == "child":
        return child(a)
    va, vb = MODES[a.mode]
    res = {va: [], vb: []}
    for _ in range(a.reps):
        for v in (va, vb):                                 # ABAB..., a fresh process each
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--variant", v, "--batch", str(a.batch), "--warmup",
                                str(a.warmup), "--iters", str(a.iters)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                sys.exit(r.returncode)                     # nothing more is started on the GPU after a failure
            res[v].append(json.loads(r.stdout.strip().splitlines()[-1])["median_ms"])
    ma, mb = statistics.median(res[va]), statistics.median(res[vb])
    out = {"mode": a.mode, "batch": a.batch, va + "_ms": ma, vb + "_ms": mb, va + "_runs": res[va], vb + "_runs": res[vb], "ratio_" + vb + "_over_" + va: mb / ma}
    if a.mode == "kernel":
        T = 1 + (L10S - 1) // 320
        nbytes = 4.0 * a.batch * (2 * L10S + 128 * T)
        out["bwd_bytes"] = nbytes
        out["bwd_fraction_of_hbm_peak"] = nbytes / (mb * 1e-3) / (HBM_PEAK_GBS * 1e9)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

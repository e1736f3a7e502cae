"""What gradient clipping and gradient accumulation cost in the fused training step (profiles/grad_clip.txt).

    python tools/bench_grad_clip.py [--configs c2,c5] [--cases clip,...] [--repeats 2] [--ab-lib OTHER.so]

BASELINE configs #2 (passt_s, batch 64, BCE) and #5 (ESC-50 fine-tune, batch 12, CE) as bench.py builds them; cases: off, clip,
accumulate 4, both -- eager, and with the captured graph on c5 (off, clip).  Every case is timed against the SAME build with the
feature off in ABBA order (off, case, case, off: one block = --steps step() calls behind a warm-up, device-synchronised, host clock), so
a drift of the machine between blocks cancels; the spread of the feature-off blocks is printed next to every difference.  With
accumulation a step() is a micro-step (same batch), so the figures are per micro-batch.

--ab-lib: a second build of the library whose norm pass reads the gradients the other way (the shipped one reads them non-temporally;
-DPA_GRADNORM_PLAIN builds plain loads); the pair pa_grad_accum_sumsq + pa_adamw_clip over a passt_s-sized buffer is timed with both,
ABBA, in this process (the question is whether the optimizer's second read of the same bytes is served from the Infinity Cache).  The
same question inside the step: run this tool with PASST_AMD_LIB pointing at either build, alternating."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import passt_amd  # noqa: E402
from passt_amd import _lib  # noqa: E402
from passt_amd.train import TrainStep  # noqa: E402

DEV = torch.device("cuda", 0)
CASES = {"off": {}, "clip": dict(clip_grad_norm=1.0), "accumulate4": dict(accumulate=4), "clip+accumulate4": dict(clip_grad_norm=1.0, accumulate=4),
         "graph_off": dict(graph=True), "graph_clip": dict(graph=True, clip_grad_norm=1.0)}


def make_step(cfgd, mel, **kw):
    with warnings.catch_warnings(), contextlib.redirect_stdout(sys.stderr):
        warnings.simplefilter("ignore")
        torch.manual_seed(1234)
        net = passt_amd.get_model(arch=cfgd["arch"], pretrained=False, n_classes=cfgd["n_classes"], **cfgd["net_kw"]).to(DEV).train()
    net.precision = "bf16"
    return TrainStep(net, mel, lr=2e-5, weight_decay=1e-4, mixup_alpha=0.3, use_mixup=True, loss=cfgd["loss"], **kw)


def block(ts, x, y, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ts.step(x, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def run_config(name, steps, repeats, only=None):
    cfgd = bench.CONFIGS[name]
    with warnings.catch_warnings(), contextlib.redirect_stdout(sys.stderr):
        warnings.simplefilter("ignore")
        mel = passt_amd.AugmentMelSTFT(n_mels=128, sr=32000, win_length=800, hopsize=320, n_fft=1024, fmin=0.0, fmax=None,
                                       fmin_aug_range=10, fmax_aug_range=2000, **cfgd["mel_kw"]).to(DEV).train()
    B = cfgd["batch"]
    x = (torch.rand(B, 1, cfgd["clip"], device=DEV) * 2 - 1) * 0.1
    y = (torch.rand(B, cfgd["n_classes"], device=DEV) < 2.7 / 527).float() if cfgd["loss"] == "bce" else torch.randint(0, cfgd["n_classes"], (B,), device=DEV)
    names = [n for n in CASES if not n.startswith("graph") or name == "c5"]
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for case in names:
            if case in ("off", "graph_off") or (only and case not in only):
                continue
            base = "graph_off" if case.startswith("graph") else "off"
            a, b = make_step(cfgd, mel, **CASES[base]), make_step(cfgd, mel, **CASES[case])
            for ts in (a, b):
                block(ts, x, y, 8)                      # warm-up: code objects, staged copies, the graph's capture (after 3 steps)
            off, on = [], []
            for _ in range(repeats):
                off.append(block(a, x, y, steps))
                on.append(block(b, x, y, steps))
                on.append(block(b, x, y, steps))
                off.append(block(a, x, y, steps))
            norm = None if b.grad_norm is None else float(b.grad_norm)
            rec = dict(config=name, batch=B, case=case, against=base, steps_per_block=steps, off_ms=[round(v, 4) for v in off],
                       on_ms=[round(v, 4) for v in on], off_mean_ms=round(float(np.mean(off)), 4), on_mean_ms=round(float(np.mean(on)), 4),
                       delta_ms=round(float(np.mean(on) - np.mean(off)), 4), off_spread_ms=round(float(max(off) - min(off)), 4),
                       delta_pct=round(float((np.mean(on) / np.mean(off) - 1) * 100), 3), last_grad_norm=norm)
            print(json.dumps(rec), flush=True)
            out.append(rec)
            a.close(), b.close()
            del a, b
            torch.cuda.empty_cache()
    return out


def run_lib_ab(path, repeats, n=85_000_000):
    """pa_grad_accum_sumsq (norm pass) + pa_adamw_clip (the second reader of the gradients) with the shipped library and with the
    other build: ms per pair, ABBA"""
    libs = {"shipped": _lib.load(), "other": C.CDLL(path)}
    for lib in libs.values():
        lib.pa_grad_norm_partials.restype, lib.pa_grad_norm_partials.argtypes = C.c_int64, [C.c_int64]
        lib.pa_grad_accum_sumsq.argtypes = _lib.SIGNATURES["pa_grad_accum_sumsq"][1]
        lib.pa_clip_coef.argtypes = _lib.SIGNATURES["pa_clip_coef"][1]
        lib.pa_adamw_clip.argtypes = _lib.SIGNATURES["pa_adamw_clip"][1]
    p, g, m, v = (torch.randn(n, device=DEV) * 0.01 for _ in range(4))
    v.abs_()
    part = torch.zeros(int(libs["shipped"].pa_grad_norm_partials(n)), device=DEV)
    out = torch.zeros(2, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def pair(lib, reps=20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            assert lib.pa_grad_accum_sumsq(g.data_ptr(), None, 0, n, part.data_ptr(), st) == 0
            assert lib.pa_clip_coef(part.data_ptr(), part.numel(), 1e30, out.data_ptr(), st) == 0
            assert lib.pa_adamw_clip(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 2e-5, 0.9, 0.999, 1e-8, 1e-4, 1, None,
                                     out.data_ptr() + 4, st) == 0
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    def norm_only(lib, reps=20):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            assert lib.pa_grad_accum_sumsq(g.data_ptr(), None, 0, n, part.data_ptr(), st) == 0
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    for lib in libs.values():
        pair(lib, 3)
    res = {"shipped": [], "other": [], "shipped_norm_only": [], "other_norm_only": []}
    for _ in range(repeats):
        for k in ("shipped", "other", "other", "shipped"):
            res[k].append(round(pair(libs[k]), 4))
            res[k + "_norm_only"].append(round(norm_only(libs[k]), 4))
    rec = dict(lib_ab=path, elements=n, gradient_MB=round(n * 4 / 1e6, 1), ms_per_pair=res,
               norm_pass_GBps={k: round(n * 4 / 1e6 / float(np.mean(res[k + "_norm_only"])), 1) for k in ("shipped", "other")})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--cases", default="", help="comma-separated subset of the cases (default: all)")
    ap.add_argument("--ab-lib", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip.py measures on the GPU; there is none")
    torch.cuda.set_device(DEV)
    for name in args.configs.split(","):
        run_config(name, args.steps * (2 if name == "c5" else 1), args.repeats, set(args.cases.split(",")) if args.cases else None)
    if args.ab_lib:
        run_lib_ab(args.ab_lib, args.repeats)


if __name__ == "__main__":
    main()

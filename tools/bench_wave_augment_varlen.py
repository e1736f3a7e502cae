#!/usr/bin/env python
"""Cost of the waveform augmentation on a ragged batch (pa_wave_augment_varlen), one GPU, no impulse responses: B = 64 clips whose
lengths are drawn uniformly between 2 s and 10 s at 32 kHz (the length set of tools/bench_varlen_step.py), parameters drawn by
WaveAugment.draw under a fixed seed (gain, roll, waveform mixup at rate 0.5).  Four variants through the C ABI on buffers allocated
once, in ONE process, in alternating blocks (a b c d a b c d ...), --reps blocks each; a block is --warmup calls, then device events
around --iters calls:

  a  padded      pa_wave_augment on the clips padded to 320 000 samples: what a ragged batch costs without this entry
  b  ragged      pa_wave_augment_varlen on the same clips, every row at its own length, L = the longest
  c  full        pa_wave_augment_varlen with all 64 lengths equal to 320 000
  d  fixed_full  pa_wave_augment on those 64 full clips: the same work as c through the fixed entry

Per variant: the median over the blocks, their spread (min .. max), and the bytes the variant has to move (valid samples read by the
mean pass and by the mix pass, rows written; computed from the lengths) per second.  The spread of a variant's own blocks is the noise
a difference has to exceed.  One JSON line per variant and a table (to --out as well, e.g. profiles/wave_augment_varlen.txt).

    python tools/bench_wave_augment_varlen.py --out profiles/wave_augment_varlen.txt
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B, SR, L10S, SEED = 64, 32000, 320000, 20


def lengths():
    """samples per clip: durations uniform in [2 s, 10 s) under the seed of tools/bench_varlen_step.py"""
    import numpy as np
    return [int(s * SR) for s in np.random.RandomState(SEED).uniform(2.0, 10.0, B)]


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


def traffic(lens, olen, partner, L, ragged):
    """bytes a variant has to move: (mean pass reads, mix pass reads, writes) * 4.  The fixed entry averages every clip once over
    min(len, L); the ragged one averages the two operands of every mixed row over min(len, n_b)."""
    mixed = [(b, p) for b, p in enumerate(partner) if p >= 0]
    if ragged:
        mean = sum(min(lens[b], olen[b]) + min(lens[p], olen[b]) for b, p in mixed)
    else:
        mean = sum(min(n, L) for n in lens) if mixed else 0
    mix = sum(min(lens[b], olen[b]) for b in range(len(lens))) + sum(min(lens[p], olen[b]) for b, p in mixed)
    return 4 * mean, 4 * mix, 4 * len(lens) * L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    import numpy as np
    import torch

    from passt_amd import _lib
    from passt_amd.augment import WaveAugment
    if not torch.cuda.is_available():
        sys.exit("bench_wave_augment_varlen: no GPU; a timing needs one")
    lib = _lib.load()
    dev = "cuda"
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    gain_db, shift, partner, lam = WaveAugment(clip_samples=L10S).draw(B)
    lens = lengths()
    full = [L10S] * B
    Lr = max(lens)
    x = (torch.rand(B, L10S, device=dev) * 2 - 1) * 0.3

    def i32(v):
        return torch.tensor(np.asarray(v, np.int32)).to(dev)

    amp = torch.from_numpy((10.0 ** (np.asarray(gain_db, np.float64) / 20.0)).astype(np.float32)).to(dev)
    sh, pt, lm = i32(shift), i32(partner), torch.from_numpy(np.asarray(lam, np.float32)).to(dev)
    len_r, len_f = i32(lens), i32(full)
    out, ws = torch.empty(B, L10S, device=dev), torch.empty(2 * B, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()                                                                                          # noqa: E731

    def fixed(ln):
        return lambda: lib.pa_wave_augment(P(x), B, L10S, P(ln), P(amp), P(sh), P(pt), P(lm), P(ws), P(out), L10S, st)

    def varlen(ln, L):
        return lambda: lib.pa_wave_augment_varlen(P(x), B, L10S, P(ln), P(ln), P(amp), P(sh), P(pt), P(lm), P(ws), P(out), L, L, st)

    fns = dict(a_padded=fixed(len_r), b_ragged=varlen(len_r, Lr), c_full=varlen(len_f, L10S), d_fixed_full=fixed(len_f))
    moved = dict(a_padded=traffic(lens, full, partner, L10S, False), b_ragged=traffic(lens, lens, partner, Lr, True),
                 c_full=traffic(full, full, partner, L10S, True), d_fixed_full=traffic(full, full, partner, L10S, False))
    for name, fn in fns.items():
        assert fn() == 0, name
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(a.reps):
        for name, fn in fns.items():
            runs[name].append(timed(fn, a.warmup, a.iters))
    mixed = int((np.asarray(partner) >= 0).sum())
    lines = [f"# tools/bench_wave_augment_varlen.py: {torch.cuda.get_device_name(0)}, B = {B}, lengths {min(lens)} .. {max(lens)} samples "
             f"(sum {sum(lens)} = {sum(lens) / (B * L10S):.3f} of {B} x {L10S}), {mixed} of {B} rows mixed, {a.reps} alternating blocks of "
             f"{a.iters} calls per variant",
             f"{'variant':>13} {'median us':>10} {'min us':>8} {'max us':>8} {'MB moved':>9} {'GB/s':>7}"]
    for name in fns:
        med, lo, hi = statistics.median(runs[name]), min(runs[name]), max(runs[name])
        nbytes = sum(moved[name])
        rec = dict(variant=name, median_ms=med, min_ms=lo, max_ms=hi, runs_ms=runs[name], bytes_mean_read=moved[name][0],
                   bytes_mix_read=moved[name][1], bytes_written=moved[name][2], gb_per_s=nbytes / (med * 1e-3) / 1e9)
        print(json.dumps(rec), flush=True)
        lines.append(f"{name:>13} {med * 1e3:>10.1f} {lo * 1e3:>8.1f} {hi * 1e3:>8.1f} {nbytes / 1e6:>9.1f} {rec['gb_per_s']:>7.0f}")
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread_a = max(runs["a_padded"]) - min(runs["a_padded"])
    lines += [f"# b / a: time {med['b_ragged'] / med['a_padded']:.3f}, bytes {sum(moved['b_ragged']) / sum(moved['a_padded']):.3f}, "
              f"samples {sum(lens) / (B * L10S):.3f}",
              f"# c - a: {(med['c_full'] - med['a_padded']) * 1e3:+.1f} us; spread of a's own blocks {spread_a * 1e3:.1f} us; "
              f"c / d (same work, fixed entry): {med['c_full'] / med['d_fixed_full']:.3f}"]
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Times the validation metrics on the device (passt_amd.metrics.EvalAccumulator) next to the reference's host path
and writes profiles/eval_metrics.txt.

    python tools/bench_eval_metrics.py [--out profiles/eval_metrics.txt] [--reps 7] [--ref-reps 3]

Synthetic validation sets of the callers' sizes.  Per case, each figure is a median over repetitions that alternate between the
figures (so that drift of the box hits all of them alike):
  (a) update() per batch of 20 and of 64   device events around a whole epoch of updates / number of batches
  (b) compute() to a host scalar           host clock around compute() + the two .item() calls (ends in a device sync)
  (c) the reference's path                 per batch out.cpu() / target.cpu(), torch.cat, average_precision_score and
                                           roc_auc_score(average=None) (one column at a time with sample_weight for a mask);
                                           needs scikit-learn, else it is reported as absent
Also: the worst difference between (b)'s per-class values and (c)'s at the timed size, and the f32 sigmoid's error figures
(torch on the CPU and the kernel against the float64 sigmoid, in ulp, on the sweep of tests/eval_metrics_cases.py).
Needs a GPU: there is no CPU path to time."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from passt_amd import _lib, ops  # noqa: E402
from passt_amd.metrics import EvalAccumulator  # noqa: E402
from tests import eval_metrics_cases as K  # noqa: E402

EPOCH_S = 34.0          # 100 000 drawn clips (audioset/dataset.py:295) at the headline 2 900 clips/s
CASES = (("AudioSet eval 20371 x 527, ~8 labels per clip", 20371, 527, 8.0 / 527, None),
         ("FSD50K eval 10231 x 200, ~5 labels per clip", 10231, 200, 5.0 / 200, None),
         ("OpenMIC test 5085 x 20, 60 % mask", 5085, 20, 0.3, 0.6),
         ("worst case 20371 x 527, 30 % positives", 20371, 527, 0.3, None))


def make_case(n, C, p_pos, p_mask, dev):
    g = torch.Generator(device="cpu").manual_seed(n * 1000 + C)
    logits = (torch.randn(n, C, generator=g) * 3).to(dev)
    target = (torch.rand(n, C, generator=g) < p_pos).float().to(dev)
    mask = None if p_mask is None else (torch.rand(n, C, generator=g) < p_mask).float().to(dev)
    return logits, target, mask


def fill(acc, logits, target, mask, B):
    acc.reset()
    for b0 in range(0, logits.shape[0], B):
        acc.update(logits[b0:b0 + B], target[b0:b0 + B], None if mask is None else mask[b0:b0 + B])


def time_updates(acc, logits, target, mask, B):
    """ms per update(): events around one epoch of them"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fill(acc, logits, target, mask, B)
    e1.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3
    nb = -(-logits.shape[0] // B)
    return e0.elapsed_time(e1) / nb, host / nb


def time_compute(acc):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = acc.compute()
    m_ap, m_auc = res["mAP"].item(), res["mAUC"].item()
    return (time.perf_counter() - t0) * 1e3, res, (m_ap, m_auc)


def reference_path(logits, target, mask, B, metrics):
    """validation_step's copies + validation_epoch_end's two calls (ex_audioset.py:238-262, ex_openmic.py:221-248) -> ms, ap, auc"""
    import warnings
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs, tgts, msks = [], [], []
    for b0 in range(0, logits.shape[0], B):
        outs.append(torch.sigmoid(logits[b0:b0 + B]).cpu())
        tgts.append(target[b0:b0 + B].cpu())
        if mask is not None:
            msks.append(mask[b0:b0 + B].cpu())
    out, tgt = torch.cat(outs).float().numpy(), torch.cat(tgts).float().numpy()
    t1 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if mask is None:
            ap = metrics.average_precision_score(tgt, out, average=None)
            auc = metrics.roc_auc_score(tgt, out, average=None)
        else:
            msk = torch.cat(msks).float().numpy()
            ap = np.array([metrics.average_precision_score(tgt[:, i], out[:, i], sample_weight=msk[:, i]) for i in range(tgt.shape[1])])
            auc = np.array([metrics.roc_auc_score(tgt[:, i], out[:, i], sample_weight=msk[:, i]) for i in range(tgt.shape[1])])
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3, np.atleast_1d(ap), np.atleast_1d(auc)


def sigmoid_figures(dev):
    z = K.sigmoid_sweep()
    n = len(z)
    keys = torch.zeros((1, n), device=dev, dtype=torch.int32)
    state = torch.zeros((1, n), device=dev, dtype=torch.uint8)
    zt = torch.from_numpy(z.reshape(n, 1)).to(dev)
    ops.eval_append(zt, torch.zeros_like(zt), keys, state, 0, mode=_lib.EVAL_SIGMOID)
    got = K.key_score(keys.cpu().numpy().view(np.uint32)[0])
    ref = torch.sigmoid(torch.from_numpy(z)).numpy()
    normal = 1.0 / (1.0 + np.exp(-z.astype(np.float64))) >= float(np.finfo(np.float32).tiny)
    e_ref, e_got = K.ulp_error(ref, z), K.ulp_error(got, z)
    return [f"f32 sigmoid against the float64 sigmoid, {n} sorted logits over [-103, 103] (tests/eval_metrics_cases.py sigmoid_sweep), in ulp:",
            f"  torch.sigmoid on CPU f32   worst {e_ref.max():.3f} (whole sweep)   {e_ref[normal].max():.3f} (where the exact value is a normal f32)",
            f"  pa_eval_append, sigmoid    worst {e_got.max():.3f} (whole sweep)   {e_got[normal].max():.3f} (normal range)",
            f"  bound of tests/test_gpu_eval_metrics.py = 2 x torch's + 1: {2 * e_ref.max() + 1:.3f} / {2 * e_ref[normal].max() + 1:.3f};"
            f" elements where the two differ: {int((ref != got).sum())} of {n}",
            "  (the whole-sweep figure comes from z < -87.3: the exact value is an f32 denormal, exp(-z) overflows, both return 0)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-reps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_metrics.py needs a GPU: nothing here has a CPU path")
    dev = torch.device("cuda", 0)
    try:
        from sklearn import metrics
        import sklearn
        ref_note = f"scikit-learn {sklearn.__version__} on this box"
    except ImportError:
        metrics, ref_note = None, "scikit-learn is not installed on this box: (c) not measured here"
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "unknown CPU") \
        if os.path.exists("/proc/cpuinfo") else "unknown CPU"
    lines = ["Validation metrics on the device: passt_amd.metrics.EvalAccumulator (pa_eval_append / pa_eval_rank) against the reference's host path",
             f"made by tools/bench_eval_metrics.py --reps {args.reps} --ref-reps {args.ref_reps};  GPU: {torch.cuda.get_device_name(0)};  host CPU: {cpu}",
             f"(c): {ref_note}", "medians over repetitions that alternate between the figures; [min .. max] behind each",
             "|(b) - (c)| is not an error of either: (c) ranks torch's f32 sigmoid computed on the device, (b) the kernel's; where the two differ",
             "in the last bit, ties between samples form or break.  The line behind it judges (b) on its own stored scores.", ""]
    for name, n, C, p_pos, p_mask in CASES:
        logits, target, mask = make_case(n, C, p_pos, p_mask, dev)
        acc = EvalAccumulator(C, capacity=32768)
        fill(acc, logits, target, mask, 64)                      # warm-up of every launch shape: both batch sizes, compute
        fill(acc, logits, target, mask, 20)
        time_compute(acc)
        t = {"a20": [], "a20h": [], "a64": [], "a64h": [], "b": [], "c": [], "c_copy": []}
        res = ref = None
        for rep in range(args.reps):
            d, h = time_updates(acc, logits, target, mask, 64)
            t["a64"].append(d), t["a64h"].append(h)
            d, h = time_updates(acc, logits, target, mask, 20)
            t["a20"].append(d), t["a20h"].append(h)
            ms, res, means = time_compute(acc)
            t["b"].append(ms)
            if metrics is not None and rep < args.ref_reps:
                ms, copy_ms, r_ap, r_auc = reference_path(logits, target, mask, 20, metrics)
                t["c"].append(ms), t["c_copy"].append(copy_ms)
                ref = (r_ap, r_auc)

        def med(k, unit="ms", scale=1.0):
            v = [x * scale for x in t[k]]
            return f"{statistics.median(v):9.3f} {unit} [{min(v):.3f} .. {max(v):.3f}]"
        n_pos = res["n_pos"].sum().item()
        lines += [f"== {name}: {n_pos} valid positives in all, sum_c P_c * N_c = {float((res['n_pos'] * (res['n_pos'] + res['n_neg'])).sum()):.3g} comparisons",
                  f"  (a) update(), batch 20   {med('a20', 'us', 1e3)} on the device per batch;  host wall per batch {med('a20h', 'us', 1e3)}",
                  f"  (a) update(), batch 64   {med('a64', 'us', 1e3)} on the device per batch;  host wall per batch {med('a64h', 'us', 1e3)}",
                  f"  (b) compute() -> mAP, mAUC on the host   {med('b')}   = {statistics.median(t['b']) / 1e3 / EPOCH_S * 100:.4f} % of a {EPOCH_S:.0f} s epoch"]
        if ref is not None:
            c_med = statistics.median(t["c"])
            err = max(float(np.nanmax(np.abs(res[k].cpu().numpy() - r))) for k, r in zip(("ap", "auc"), ref))
            same_nan = all(np.array_equal(np.isnan(res[k].cpu().numpy()), np.isnan(r)) for k, r in zip(("ap", "auc"), ref))
            lines += [f"  (c) reference path, batch 20             {med('c')}   of which copies + cat {med('c_copy')}   = {c_med / 1e3 / EPOCH_S * 100:.2f} % of the epoch",
                      f"      (b) is {c_med / statistics.median(t['b']):.0f} x faster than (c);  per-class |ap, auc (b) - (c)| <= {err:.2e}, NaN classes equal: {same_nan}"]
        else:
            lines += ["  (c) not measured on this box"]
        # faster and different is not faster: the timed result against the NumPy restatement of the arithmetic on the stored keys
        sig = K.key_score(acc._keys[:, :n].cpu().numpy().view(np.uint32)).T
        r = K.restate(sig, target.cpu().numpy(), None if mask is None else mask.cpu().numpy())
        exact = all(np.array_equal(res[k].cpu().numpy(), r[k]) for k in ("n_pos", "n_neg", "auc_num"))
        err = max(float(np.nanmax(np.abs(res[k].cpu().numpy() - r[k]))) for k in ("ap", "auc"))
        lines += [f"  at this size against tests/eval_metrics_cases.py restate(): n_pos, n_neg, auc_num equal: {exact};  |ap, auc| <= {err:.2e}"]
        lines.append("")
        del acc, logits, target, mask
    lines += sigmoid_figures(dev)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

"""Fixture of Patchout training on ragged batches: tests/golden/varlen_train.npz, from the real reference implementation
(kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_varlen_grad_golden.py does; none of its text is here).

The contract of ``net.train(); net.varlen_train = True; net(x, lengths=...)`` is that every clip gets what it would get alone at batch
size 1 in training mode, the Patchout draws being made clip after clip.  So the reference ``PaSST.train()`` runs ONE CLIP AT A TIME,
cropped to its length, under ONE ``torch.manual_seed`` per case, with make_varlen_grad_golden's loss ``(logits * a).sum() + (features *
b).sum()``, every parameter and the input requiring a gradient, and for every case of CASES this records

    <case>.logits (B, n_classes)   <case>.features (B, D)     row i = clip i alone
    <case>.dx.<i>                  pin_sample(dx of clip i (1, 1, n_mels, lengths[i]), SAMPLE)   .stats = (L2 norm, largest magnitude)
    <case>.dx.<i>.nonzero          number of non-zero entries of that dx (= the pixels some kept patch covers)
    <case>.grad.<parameter>        the same for the gradients of param_grads() summed over the clips
    <case>.rng                     the CPU generator's state after the last clip
    <case>.row_f / row_t / row_tpos / cu_tok / toff     the index part: the packed token rows the draws imply (varlen_geometry_train's
                                   layout), rebuilt from the values the reference's own torch.randint / torch.randperm calls RETURNED
                                   (recorded while it ran), not from this project's draw order

Weights and inputs are oracle/detgen.py streams, so the tests regenerate them instead of storing them.

    python tests/golden/make_varlen_train_golden.py        (CPU, about a minute)
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import detgen, ref_import  # noqa: E402
from oracle import passt_oracle as O   # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_grad_golden as VG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = 4096
# depth 2, 768 / 12 heads, stride 10, a 256-frame model: Tpe = 25 time positions, Fg = 12 frequency rows
MODEL = dict(embed_dim=768, depth=2, num_heads=12, img_size=(128, 256))
CASES = {
    # 16 frames = 1 patch column, 12 patches, 5 kept; the 300-frame clip (29 columns) is cut to 25 and draws no offset
    "a": dict(cfg=O.make_cfg(**MODEL, u_patchout=7), lengths=(16, 56, 106, 300), seed=51, torch_seed=2024),
    "b": dict(cfg=O.make_cfg(**MODEL, s_patchout_t=2, s_patchout_f=3), lengths=(56, 106, 250), seed=52, torch_seed=2025),
    "c": dict(cfg=O.make_cfg(**MODEL, s_patchout_t=2, s_patchout_f=3, u_patchout=7), lengths=(106, 250), seed=53, torch_seed=2026),
}
INDEX_KEYS = ("row_f", "row_t", "row_tpos", "cu_tok", "toff")
param_grads = VG.param_grads
loss_of = VG.loss_of


def inputs(case):
    """(x (B, 1, n_mels, longest clip), a (B, n_classes), b (B, D)): clip i is the first lengths[i] frames of x[i]."""
    cfg, B = case["cfg"], len(case["lengths"])
    x = detgen.uniform(case["seed"], "x", (B, 1, cfg["img_size"][0], max(case["lengths"])), -1.5, 1.5)
    a = detgen.uniform(case["seed"], "a", (B, cfg["num_classes"]), -1.0, 1.0)
    b = detgen.uniform(case["seed"], "b", (B, cfg["embed_dim"]), -1.0, 1.0)
    return x, a, b


def grid_of(cfg, n):
    """(frequency rows, patch columns before the time cut) of an n-frame clip"""
    P, (fs, ts) = cfg["patch"], cfg["stride"]
    return (cfg["img_size"][0] - P) // fs + 1, (n - P) // ts + 1


def covered(cfg, n, row_f, row_t):
    """bool (n_mels, n): the pixels of an n-frame clip that the patches at grid positions (row_f, row_t) cover"""
    P, (fs, ts) = cfg["patch"], cfg["stride"]
    m = np.zeros((cfg["img_size"][0], n), dtype=bool)
    for f, t in zip(row_f, row_t):
        m[f * fs:f * fs + P, t * ts:t * ts + P] = True
    return m


class _Draws:
    """Records what torch.randint / torch.randperm return while the reference runs (they are called through, untouched)."""

    def __enter__(self):
        self.log, self._saved = [], (torch.randint, torch.randperm)

        def spy(name, fn):
            def call(*a, **k):
                out = fn(*a, **k)
                self.log.append((name, int(a[0]), out.clone().numpy()))
                return out
            return call
        torch.randint, torch.randperm = spy("randint", torch.randint), spy("randperm", torch.randperm)
        return self

    def __exit__(self, *exc):
        torch.randint, torch.randperm = self._saved


def rows_from_draws(cfg, lengths, logs):
    """The packed token rows of the batch from the recorded return values, clip after clip: cls, dist, then the kept patches in sequence
    order (frequency-major flatten of the kept columns x kept rows, then the unstructured selection)."""
    Tpe = cfg["grid"][1]
    row_f, row_t, row_tpos, cu, toffs = [], [], [], [0], []
    for n, log in zip(lengths, logs):
        log = list(log)
        F_dim, T_dim = grid_of(cfg, n)
        toff = 0
        if T_dim < Tpe:
            name, hi, v = log.pop(0)
            assert name == "randint" and hi == 1 + Tpe - T_dim
            toff = int(v[0])
        ts, fs = np.arange(min(T_dim, Tpe)), np.arange(F_dim)
        if cfg["s_patchout_t"]:
            name, hi, v = log.pop(0)
            assert name == "randperm" and hi == T_dim
            ts = np.sort(v[:T_dim - cfg["s_patchout_t"]])
        if cfg["s_patchout_f"]:
            name, hi, v = log.pop(0)
            assert name == "randperm" and hi == F_dim
            fs = np.sort(v[:F_dim - cfg["s_patchout_f"]])
        pf, pt = np.repeat(fs, ts.size), np.tile(ts, fs.size)
        if cfg["u_patchout"]:
            name, hi, v = log.pop(0)
            assert name == "randperm" and hi == pf.size
            keep = np.sort(v[:pf.size - cfg["u_patchout"]])
            pf, pt = pf[keep], pt[keep]
        assert not log
        row_f += [-1, -1] + pf.tolist()
        row_t += [0, 1] + pt.tolist()
        row_tpos += [0, 1] + (pt + toff).tolist()
        cu.append(len(row_f))
        toffs.append(toff)
    return dict(row_f=np.array(row_f, np.int32), row_t=np.array(row_t, np.int32), row_tpos=np.array(row_tpos, np.int32),
                cu_tok=np.array(cu, np.int32), toff=np.array(toffs, np.int32))


def run_case(case):
    cfg, lengths = case["cfg"], case["lengths"]
    m = ref_import.build_reference_passt(cfg, detgen.passt_state_dict(cfg, case["seed"]))
    m.train()
    x, a, b = inputs(case)
    out, lo, fe, logs = {}, [], [], []
    torch.manual_seed(case["torch_seed"])
    for i, n in enumerate(lengths):
        xt = torch.from_numpy(np.ascontiguousarray(x[i:i + 1, :, :, :n])).requires_grad_()
        with warnings.catch_warnings(), _Draws() as d:
            warnings.simplefilter("ignore")
            logits, feat = ref_import.run_silently(m, xt)[:2]
        logs.append(d.log)
        loss_of(logits, feat, torch.from_numpy(a[i:i + 1]), torch.from_numpy(b[i:i + 1])).backward()
        lo.append(logits.detach().numpy()[0])
        fe.append(feat.detach().numpy()[0])
        G._pinned_into(out, f"dx.{i}", xt.grad.numpy(), SAMPLE)
        out[f"dx.{i}.nonzero"] = np.array(int(np.count_nonzero(xt.grad.numpy())), np.int64)
    out["rng"] = torch.get_rng_state().numpy().copy()
    out["logits"], out["features"] = np.stack(lo), np.stack(fe)
    params = dict(m.named_parameters())
    for k in param_grads(cfg):
        G._pinned_into(out, f"grad.{k}", params[k].grad.numpy(), SAMPLE)
    out.update(rows_from_draws(cfg, lengths, logs))
    return out


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        res = run_case(case)
        out.update({f"{name}.{k}": v for k, v in res.items()})
        print(name, "tokens per clip", np.diff(res["cu_tok"]).tolist(), "toff", res["toff"].tolist(),
              "max|dx| per clip", [float(res[f"dx.{i}.stats"][1]) for i in range(len(case["lengths"]))])
    np.savez_compressed(os.path.join(HERE, "varlen_train.npz"), **out)


if __name__ == "__main__":
    main()

"""Generate tests/golden/ir_augment.npz by running the REAL reference bodies of pydub_augment (with its impulse-response branch),
pad_or_truncate, get_roll_func and MixupDataset from audioset/dataset.py, extracted with ast the way make_golden.py produces
wave_augment.npz (the module needs av, h5py, librosa to import).

    python tests/golden/make_golden_ir.py

``convolve`` is scipy.signal.convolve as in the reference's import, ``get_ir_sample`` returns the case's IR, the draws are pinned to
tests.ir_cases.IR_AUG_CASE.  Only arrays are stored: the reference's outputs and mixed targets, and ``ref_err`` [B], the largest
distance of each output row from the same pipeline evaluated in float64 (the reference's own error; the test adds it to its cap).
Inputs are regenerated bit-exactly by tests.ir_cases.ir_aug_inputs."""
import ast
import contextlib
import io
import os
import sys

import numpy as np
import scipy.signal
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from tests import ir_cases as IC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def float64_pipeline(c, raws, irs):
    """the same per-item pipeline and mixing in float64 on the float32 operands"""
    L, items = c["L"], []
    for b, raw in enumerate(raws):
        w = raw.astype(np.float64)
        if c["ir_idx"][b] >= 0:
            w = np.convolve(w, irs[c["ir_idx"][b]].astype(np.float64))
        w = w * 10.0 ** (c["gain_db"][b] / 20.0)
        w = np.concatenate([w, np.zeros(max(L - len(w), 0))])[:L]
        items.append(np.roll(w, c["shift"][b]))
    out = []
    for b in range(len(raws)):
        if c["partner"][b] < 0:
            out.append(items[b])
            continue
        lam = max(c["lam"][b], 1.0 - c["lam"][b])
        x1, x2 = items[b] - items[b].mean(), items[c["partner"][b]] - items[c["partner"][b]].mean()
        x = x1 * lam + x2 * (1.0 - lam)
        out.append(x - x.mean())
    return np.stack(out)


def gen_ir_case():
    src = open(os.path.join(ref_import.REFERENCE_ROOT, "audioset", "dataset.py")).read()
    keep = []
    for node in ast.parse(src).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in ("pad_or_truncate", "pydub_augment", "get_roll_func",
                                                                              "MixupDataset"):
            node.decorator_list = []
            keep.append(node)
    c = IC.IR_AUG_CASE
    raws, irs = IC.ir_aug_inputs(c)
    current = {}
    ns = {"np": np, "torch": torch, "TorchDataset": object, "convolve": scipy.signal.convolve,
          "get_ir_sample": lambda: irs[c["ir_idx"][current["item"]]]}
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(ast.Module(body=keep, type_ignores=[]), "<reference audioset/dataset.py>", "exec"), ns)

    class Items:                                      # what AudioSetDataset.__getitem__ + roll_func hand over
        def __len__(self):
            return len(raws)

        def __getitem__(self, i):
            current["item"] = i
            s_rand, s_randint = torch.rand, torch.randint
            torch.rand = lambda *a, **k: torch.tensor([0.0 if c["ir_idx"][i] >= 0 else 1.0])       # the IR decision, ir_augment = 0.5
            torch.randint = lambda *a, **k: torch.tensor([c["gain_db"][i] + 7])
            try:
                w = ns["pydub_augment"](raws[i], gain_augment=7, ir_augment=0.5)
            finally:
                torch.rand, torch.randint = s_rand, s_randint
            w = ns["pad_or_truncate"](np.asarray(w, np.float32), c["L"]).reshape(1, -1)
            with contextlib.redirect_stdout(io.StringIO()):
                x, _, y = ns["get_roll_func"](axis=1, shift=c["shift"][i])((w, f"clip{i}", np.eye(len(raws), dtype=np.float32)[i]))
            return x, f"clip{i}", torch.as_tensor(y)

    with contextlib.redirect_stdout(io.StringIO()):
        mix = ns["MixupDataset"](Items(), beta=2, rate=0.5)
    out, tgt = [], []
    for b in range(len(raws)):
        s_rand, s_randint, s_beta = torch.rand, torch.randint, np.random.beta
        torch.rand = lambda *a, **k: torch.tensor([0.0 if c["partner"][b] >= 0 else 1.0])
        torch.randint = lambda *a, **k: torch.tensor([max(c["partner"][b], 0)])
        np.random.beta = lambda *a, **k: c["lam"][b]
        try:
            x, _, y = mix[b]
        finally:
            torch.rand, torch.randint, np.random.beta = s_rand, s_randint, s_beta
        out.append(np.asarray(x, np.float32).reshape(-1))
        tgt.append(np.asarray(y, np.float32))
    out = np.stack(out)
    ref_err = np.abs(out.astype(np.float64) - float64_pipeline(c, raws, irs)).max(axis=1)
    np.savez_compressed(os.path.join(HERE, "ir_augment.npz"), out=out, target=np.stack(tgt), ref_err=ref_err)
    print("ir_augment", out.shape, float(np.abs(out).max()), "reference error per clip", ref_err)


if __name__ == "__main__":
    gen_ir_case()

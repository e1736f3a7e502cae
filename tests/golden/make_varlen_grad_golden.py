"""Fixture of the gradients through the ragged-batch forward: tests/golden/varlen_grad.npz, from the real reference implementation
(kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_varlen_golden.py does; none of its text is here).

The reference's answer to clips of different lengths is batch size 1 (ex_fsd50k.py:53-56), and there ``x.requires_grad_()`` is plain
autograd.  So the reference ``PaSST.eval()`` runs ONE CLIP AT A TIME on make_varlen_golden's MODELS and LENGTHS with the
input-gradient fixture's loss ``(logits * a).sum() + (features * b).sum()`` (detgen rows ``a``, ``b`` per clip), in two variants --
parameters frozen and parameters trainable -- and records

    <model>.<variant>.dx.<i>             pin_sample(dx of clip i (1, 1, n_mels, LENGTHS[i]), DX_SAMPLE)   .stats = (L2 norm, largest magnitude)
    <model>.trainable.grad.<parameter>   the same for the gradients of PARAM_GRADS summed over the clips

Weights and inputs are oracle/detgen.py streams, so the tests regenerate them instead of storing them.

    python tests/golden/make_varlen_grad_golden.py        (CPU, about a minute)
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import detgen, ref_import  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_golden as V  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DX_SAMPLE = 4096
VARIANTS = ("frozen", "trainable")
MODELS, LENGTHS = V.MODELS, V.LENGTHS


def param_grads(cfg):
    last = cfg["depth"] - 1
    return ("time_new_pos_embed", "freq_new_pos_embed", "cls_token", "dist_token", "new_pos_embed", "patch_embed.proj.weight",
            "patch_embed.proj.bias", "blocks.0.attn.qkv.weight", f"blocks.{last}.mlp.fc1.weight", "norm.weight", "head.1.weight")


def inputs(case):
    """(x (B, 1, n_mels, max LENGTHS), a (B, n_classes), b (B, D)): clip i is the first LENGTHS[i] frames of x[i]."""
    cfg, B = case["cfg"], len(LENGTHS)
    a = detgen.uniform(case["seed"], "a", (B, cfg["num_classes"]), -1.0, 1.0)
    b = detgen.uniform(case["seed"], "b", (B, cfg["embed_dim"]), -1.0, 1.0)
    return V.model_input(case), a, b


def loss_of(logits, feat, a, b):
    return (logits * a).sum() + (feat * b).sum()


def per_clip(case, trainable, forward, params):
    """Run ``forward(x_clip) -> (logits, features)`` one clip at a time under the fixture's loss.  ``params``: {name: leaf tensor} whose
    .grad accumulates over the clips.  Returns ([dx of clip i], {name: summed gradient})."""
    x, a, b = inputs(case)
    dxs = []
    for i, n in enumerate(LENGTHS):
        xt = torch.from_numpy(np.ascontiguousarray(x[i:i + 1, :, :, :n])).requires_grad_()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat = forward(xt)
        loss_of(logits, feat, torch.from_numpy(a[i:i + 1]), torch.from_numpy(b[i:i + 1])).backward()
        dxs.append(xt.grad.numpy())
    grads = {k: params[k].grad.numpy() for k in param_grads(case["cfg"])} if trainable else {}
    return dxs, grads


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in MODELS.items():
        for variant in VARIANTS:
            m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
            m.eval()
            m.requires_grad_(variant == "trainable")
            dxs, grads = per_clip(case, variant == "trainable", lambda xt: ref_import.run_silently(m, xt)[:2], dict(m.named_parameters()))
            for i, dx in enumerate(dxs):
                G._pinned_into(out, f"{name}.{variant}.dx.{i}", dx, DX_SAMPLE)
            for k, v in grads.items():
                G._pinned_into(out, f"{name}.{variant}.grad.{k}", v, DX_SAMPLE)
            print(name, variant, "max|dx| per clip", [float(out[f"{name}.{variant}.dx.{i}.stats"][1]) for i in range(len(LENGTHS))])
    np.savez_compressed(os.path.join(HERE, "varlen_grad.npz"), **out)


if __name__ == "__main__":
    main()

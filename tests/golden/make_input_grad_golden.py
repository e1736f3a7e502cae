"""Fixture of the gradient w.r.t. the input spectrogram: tests/golden/input_grad.npz, from the real reference implementation
(kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_golden.py does; none of its text is here).

In the reference ``x.requires_grad_()`` is plain autograd.  Every case runs the reference ``PaSST`` on a detgen spectrogram that
requires a gradient, with the loss ``(logits * a).sum() + (features * b).sum()`` (detgen ``a``, ``b``, a different row per clip,
so both outputs feed the gradient), and records

    <case>.logits  <case>.features
    <case>.dx                 pin_sample(dx, DX_SAMPLE)         <case>.dx.stats = (L2 norm, largest magnitude) of the whole dx
    <case>.grad.<parameter>   the same for PARAM_GRADS, where the case's parameters are trainable

Weights and inputs are oracle/detgen.py streams, so the tests regenerate them instead of storing them.

    python tests/golden/make_input_grad_golden.py        (CPU, about a minute)
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

HERE = os.path.dirname(os.path.abspath(__file__))
DX_SAMPLE = 8192
PARAM_GRADS = ("patch_embed.proj.weight", "blocks.0.attn.qkv.weight")

CASES = {
    # the loss-network case: eval, stride 10, 998 frames (1190 tokens, every inner pixel under four patches), all parameters frozen
    "frozen_eval": dict(cfg=O.make_cfg(embed_dim=768, depth=2, num_heads=12), B=2, T=998, training=False, frozen=True, seed=51),
    # train mode, structured + unstructured Patchout (model_small_train's geometry and seeding), parameters trainable
    "patchout_train": dict(cfg=O.make_cfg(**G.SMALL, s_patchout_t=6, s_patchout_f=3, u_patchout=5), B=3, T=250, training=True,
                           frozen=False, seed=52, torch_seed=1234),
    # stride 16: no overlap; mixed strides
    "stride16": dict(cfg=O.make_cfg(**dict(G.SMALL, img_size=(128, 320), stride=(16, 16))), B=2, T=320, training=False, frozen=False,
                     seed=53),
    "stride10x16": dict(cfg=O.make_cfg(**dict(G.SMALL, img_size=(128, 320), stride=(10, 16))), B=2, T=320, training=False,
                        frozen=False, seed=54),
    # input longer than the model (the reference's "x will be cut" warning): 32 patch columns into a 25-column time embedding
    "time_cut": dict(cfg=O.make_cfg(**G.SMALL), B=2, T=330, training=False, frozen=True, seed=55),
    # a larger batch, a different (a, b) row per clip
    "batch4": dict(cfg=O.make_cfg(**G.SMALL), B=4, T=250, training=False, frozen=False, seed=56),
}


def inputs(case):
    """(x (B, 1, n_mels, T), a (B, n_classes), b (B, D)) of a case."""
    cfg, B = case["cfg"], case["B"]
    x = detgen.uniform(case["seed"], "x", (B, 1, cfg["img_size"][0], case["T"]), -1.5, 1.5)
    a = detgen.uniform(case["seed"], "a", (B, cfg["num_classes"]), -1.0, 1.0)
    b = detgen.uniform(case["seed"], "b", (B, cfg["embed_dim"]), -1.0, 1.0)
    return x, a, b


def loss_of(logits, feat, a, b):
    return (logits * a).sum() + (feat * b).sum()


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.train(case["training"])
        m.requires_grad_(not case["frozen"])
        x, a, b = inputs(case)
        xt = torch.from_numpy(x).requires_grad_()
        if "torch_seed" in case:
            torch.manual_seed(case["torch_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat = ref_import.run_silently(m, xt)
        loss_of(logits, feat, torch.from_numpy(a), torch.from_numpy(b)).backward()
        out[name + ".logits"], out[name + ".features"] = logits.detach().numpy(), feat.detach().numpy()
        G._pinned_into(out, name + ".dx", xt.grad.numpy(), DX_SAMPLE)
        params = dict(m.named_parameters())
        for k in PARAM_GRADS:
            if case["frozen"]:
                assert params[k].grad is None
            else:
                G._pinned_into(out, f"{name}.grad.{k}", params[k].grad.numpy(), DX_SAMPLE)
        print(name, "dx", tuple(xt.grad.shape), "norm / absmax", out[name + ".dx.stats"])
    np.savez_compressed(os.path.join(HERE, "input_grad.npz"), **out)


if __name__ == "__main__":
    main()

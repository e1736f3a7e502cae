"""Fixture of the attention maps' gradients: tests/golden/attn_grad.npz, from the real reference implementation (kkoutini/PaSST,
imported read-only through oracle/ref_import.py exactly as make_attn_golden.py does; none of its text is here).

In the reference the attention probabilities of a block are the INPUT of ``blocks[i].attn.attn_drop``; a forward hook there that calls
``retain_grad()`` on it leaves, after ``loss.backward()``, the gradient of the loss with respect to the probabilities in its ``.grad``.
Every case of make_attn_golden (same configurations, seeds, inputs and hooked blocks) runs the reference ``PaSST`` with such hooks and
make_hidden_golden's loss

    (logits * a).sum() + (features * b).sum()            (detgen ``a``, ``b``)

and records, for every hooked block l,

    <case>.grad.b<l>.<v>          pin_sample of the (B, H, N, N) gradient, v in GRAD_VARIANTS (all rows / the cls and dist query rows)
    <case>.cam.b<l>.<v>           pin_sample of relu(map * gradient) in fp64, v in make_attn_golden.VARIANTS ("mean": its mean over heads)
    <key>.stats                   (L2 norm, largest magnitude) of the whole tensor
    <key>.shape                   its shape

The ragged case is the reference's own way with clips of different lengths: ONE CLIP AT A TIME at batch size 1, cropped to its
length (``ragged.<i>.*`` per clip, ``a`` / ``b`` rows i).  Weights and inputs are oracle/detgen.py streams, so the tests regenerate
them instead of storing them.

    python tests/golden/make_attn_grad_golden.py        (CPU, about a minute)
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import detgen, ref_import  # noqa: E402
from tests.golden import make_attn_golden as AG  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = AG.SAMPLE
CASES, RAGGED, VARIANTS = AG.CASES, AG.RAGGED, AG.VARIANTS
GRAD_VARIANTS = ("all.each", "prefix.each")          # the network forms no mean over heads: there is no gradient w.r.t. one


def loss_weights(case, B=None):
    """(a (B, n_classes), b (B, D)) of the loss."""
    cfg, B = case["cfg"], case["B"] if B is None else B
    return (detgen.uniform(case["seed"], "a", (B, cfg["num_classes"]), -1.0, 1.0),
            detgen.uniform(case["seed"], "b", (B, cfg["embed_dim"]), -1.0, 1.0))


def ragged_loss_weights():
    return loss_weights(RAGGED, len(RAGGED["lengths"]))


def run_reference(m, x, a, b, attn):
    """[(map, its gradient) as (B, H, N, N) arrays per entry of ``attn``] after the backward of the loss."""
    seen, hooks = {}, []

    def hook(_m, inp, _o, key):
        inp[0].retain_grad()
        seen[key] = inp[0]

    for k in attn:
        hooks.append(m.blocks[k].attn.attn_drop.register_forward_hook(lambda _m, inp, _o, k=k: hook(_m, inp, _o, k)))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat = ref_import.run_silently(m, torch.from_numpy(np.ascontiguousarray(x)))
    finally:
        for hk in hooks:
            hk.remove()
    ((logits * torch.from_numpy(a)).sum() + (feat * torch.from_numpy(b)).sum()).backward()
    return [(seen[k].detach().numpy(), seen[k].grad.numpy()) for k in attn]


def _into(out, prefix, case, pairs):
    depth = case["cfg"]["depth"]
    for k, (p, g) in zip(case["attn"], pairs):
        blk = AG.block_of(k, depth)
        cam = np.maximum(p.astype(np.float64) * g.astype(np.float64), 0.0)
        for kind, full, variants in (("grad", g, GRAD_VARIANTS), ("cam", cam, VARIANTS)):
            for v in variants:
                key = f"{prefix}.{kind}.b{blk}.{v}"
                t = AG.variant_of(full, v)
                G._pinned_into(out, key, t, SAMPLE)
                out[key + ".shape"] = np.array(t.shape, np.int64)


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.train(case["training"])
        if "torch_seed" in case:
            torch.manual_seed(case["torch_seed"])
        pairs = run_reference(m, AG.inputs(case), *loss_weights(case), case["attn"])
        _into(out, name, case, pairs)
        print(name, [g.shape for _, g in pairs], [float(np.abs(g).max()) for _, g in pairs])
    case = RAGGED
    m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
    m.eval()
    x = AG.ragged_inputs()
    a, b = ragged_loss_weights()
    for i, n in enumerate(case["lengths"]):
        m.zero_grad()
        pairs = run_reference(m, x[i:i + 1, :, :, :n], a[i:i + 1], b[i:i + 1], case["attn"])
        _into(out, f"ragged.{i}", case, pairs)
        print("ragged", i, n, [g.shape for _, g in pairs])
    np.savez_compressed(os.path.join(HERE, "attn_grad.npz"), **out)


if __name__ == "__main__":
    main()

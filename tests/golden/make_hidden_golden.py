"""Fixture of the per-layer token outputs and the gradients of a loss on them: tests/golden/hidden.npz, from the real reference
implementation (kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_golden.py does; none of its text
is here).

In the reference the token sequence at a depth is what a forward hook on ``blocks[i]`` (or on ``norm``) sees.  Every case runs the
reference ``PaSST`` with such hooks on a detgen spectrogram that requires a gradient, with the loss

    (logits * a).sum() + (features * b).sum() + sum_l (h_l * c_l).sum()

(detgen ``a``, ``b``, ``c_l``; a case with ``hidden_only`` drops the first two terms) and records

    <case>.logits  <case>.features
    <case>.hidden.<l>         pin_sample(h_l, SAMPLE)           <case>.hidden.<l>.stats = (L2 norm, largest magnitude) of all of h_l
    <case>.hidden.<l>.shape   h_l's shape
    <case>.dx                 pin_sample(dx, SAMPLE)            <case>.dx.stats likewise
    <case>.grad.<parameter>   the same for PARAM_GRADS, where the case's parameters are trainable

The ragged case is the reference's own way with clips of different lengths: ONE CLIP AT A TIME at batch size 1, cropped to its
length (``ragged.<i>.*`` per clip; ``ragged.grad.*`` is the sum over the clips, which is what a packed batch accumulates).
Weights and inputs are oracle/detgen.py streams, so the tests regenerate them instead of storing them.

    python tests/golden/make_hidden_golden.py        (CPU, a few minutes)
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
SAMPLE = 4096
PARAM_GRADS = ("patch_embed.proj.weight", "blocks.0.attn.qkv.weight")

CASES = {
    # the perceptual-loss case: eval, stride 10, 998 frames (1190 tokens), depth 2 at full width, all parameters frozen
    "frozen_eval": dict(cfg=O.make_cfg(embed_dim=768, depth=2, num_heads=12), B=2, T=998, training=False, frozen=True, seed=61,
                        hidden=(0, -1, "norm")),
    # train mode, structured + unstructured Patchout (model_small_train's geometry and seeding), parameters trainable
    "patchout_train": dict(cfg=O.make_cfg(**G.SMALL, s_patchout_t=6, s_patchout_f=3, u_patchout=5), B=3, T=250, training=True,
                           frozen=False, seed=62, torch_seed=1234, hidden=(0, "norm", -1)),
    # the loss reads token outputs only: logits and features stay unused
    "hidden_only": dict(cfg=O.make_cfg(**G.SMALL), B=2, T=250, training=False, frozen=False, seed=63, hidden=(0, "norm"),
                        hidden_only=True),
    # an intermediate layer only (prefix-only tail), three blocks deep
    "intermediate": dict(cfg=O.make_cfg(**dict(G.SMALL, depth=3)), B=2, T=250, training=False, frozen=False, seed=64, hidden=(1, 0)),
}
# the ragged path: clips of three different lengths, each alone at batch size 1 (998 = the model's length, 33 = two patch columns)
RAGGED = dict(cfg=O.make_cfg(**dict(G.SMALL, img_size=(128, 998))), seed=65, lengths=[998, 437, 33], hidden=(0, -1, "norm"))


def key_of(h):
    """fixture / detgen name of a requested entry"""
    return "norm" if h == "norm" else f"b{h}"


def inputs(case):
    """(x (B, 1, n_mels, T), a (B, n_classes), b (B, D)) of a case."""
    cfg, B = case["cfg"], case["B"]
    x = detgen.uniform(case["seed"], "x", (B, 1, cfg["img_size"][0], case["T"]), -1.5, 1.5)
    a = detgen.uniform(case["seed"], "a", (B, cfg["num_classes"]), -1.0, 1.0)
    b = detgen.uniform(case["seed"], "b", (B, cfg["embed_dim"]), -1.0, 1.0)
    return x, a, b


def hidden_weights(seed, h, shape, clip=None):
    """c_l of the loss for a token output of ``shape`` (..., Ntok, D): detgen, scaled by 1 / Ntok so that a layer's term weighs
    about what the pooled outputs' terms weigh.  ``clip``: the ragged case's own stream per clip."""
    name = "c." + key_of(h) + ("" if clip is None else f".{clip}")
    return detgen.uniform(seed, name, shape, -1.0, 1.0) / np.float32(shape[-2])


def loss_of(logits, feat, hs, a, b, cs, hidden_only=False):
    loss = sum((h * c).sum() for h, c in zip(hs, cs))
    return loss if hidden_only else loss + (logits * a).sum() + (feat * b).sum()


def run_reference(m, x, hidden):
    """(logits, features, [token output per entry of ``hidden``]) of the reference model ``m`` through forward hooks."""
    seen, hooks = {}, []
    for h in hidden:
        mod = m.norm if h == "norm" else m.blocks[h]
        hooks.append(mod.register_forward_hook(lambda _m, _i, out, h=h: seen.__setitem__(h, out)))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat = ref_import.run_silently(m, x)
    finally:
        for hk in hooks:
            hk.remove()
    return logits, feat, [seen[h] for h in hidden]


def reference_step(m, case, x, a, b, clip=None):
    xt = torch.from_numpy(np.ascontiguousarray(x)).requires_grad_()
    logits, feat, hs = run_reference(m, xt, case["hidden"])
    cs = [torch.from_numpy(hidden_weights(case["seed"], h, tuple(t.shape), clip)) for h, t in zip(case["hidden"], hs)]
    loss_of(logits, feat, hs, torch.from_numpy(a), torch.from_numpy(b), cs, case.get("hidden_only", False)).backward()
    return logits.detach().numpy(), feat.detach().numpy(), [t.detach().numpy() for t in hs], xt.grad.numpy()


def _hidden_into(out, prefix, hidden, hs):
    for h, t in zip(hidden, hs):
        G._pinned_into(out, f"{prefix}.hidden.{key_of(h)}", t, SAMPLE)
        out[f"{prefix}.hidden.{key_of(h)}.shape"] = np.array(t.shape, np.int64)


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.train(case["training"])
        m.requires_grad_(not case["frozen"])
        x, a, b = inputs(case)
        if "torch_seed" in case:
            torch.manual_seed(case["torch_seed"])
        logits, feat, hs, dx = reference_step(m, case, x, a, b)
        out[name + ".logits"], out[name + ".features"] = logits, feat
        _hidden_into(out, name, case["hidden"], hs)
        G._pinned_into(out, name + ".dx", dx, SAMPLE)
        params = dict(m.named_parameters())
        for k in PARAM_GRADS:
            if case["frozen"]:
                assert params[k].grad is None
            else:
                G._pinned_into(out, f"{name}.grad.{k}", params[k].grad.numpy(), SAMPLE)
        print(name, [tuple(t.shape) for t in hs], "dx norm / absmax", out[name + ".dx.stats"])
    # ragged: every clip alone, cropped to its length; the parameter gradients add up over the clips
    case = RAGGED
    m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
    m.eval()
    x, a, b = ragged_inputs()
    for i, n in enumerate(case["lengths"]):
        logits, feat, hs, dx = reference_step(m, case, x[i:i + 1, :, :, :n], a[i:i + 1], b[i:i + 1], clip=i)
        out[f"ragged.{i}.logits"], out[f"ragged.{i}.features"] = logits, feat
        _hidden_into(out, f"ragged.{i}", case["hidden"], hs)
        G._pinned_into(out, f"ragged.{i}.dx", dx, SAMPLE)
        print("ragged", i, n, [tuple(t.shape) for t in hs])
    params = dict(m.named_parameters())
    for k in PARAM_GRADS:
        G._pinned_into(out, f"ragged.grad.{k}", params[k].grad.numpy(), SAMPLE)
    np.savez_compressed(os.path.join(HERE, "hidden.npz"), **out)


def ragged_inputs():
    """(x (B, 1, n_mels, max length), a, b) of the ragged case: clip i is its first lengths[i] frames."""
    return inputs(dict(RAGGED, B=len(RAGGED["lengths"]), T=max(RAGGED["lengths"])))


if __name__ == "__main__":
    main()

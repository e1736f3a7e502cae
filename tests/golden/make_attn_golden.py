"""Fixture of the attention maps: tests/golden/attn.npz, from the real reference implementation (kkoutini/PaSST, imported read-only
through oracle/ref_import.py exactly as make_golden.py does; none of its text is here).

In the reference the attention probabilities softmax(q k^T * scale) of a block are what a forward hook on
``blocks[i].attn.attn_drop`` sees as its INPUT (the plus-one variant of the softmax is switched off there).  Every case runs the
reference ``PaSST`` with such hooks on a detgen spectrogram and records, for every hooked block l and every variant v of
VARIANTS (derived here from the hooked (B, H, N, N) map: the mean over heads, the cls / dist query rows),

    <case>.logits  <case>.features
    <case>.attn.b<l>.<v>          pin_sample(map, SAMPLE)
    <case>.attn.b<l>.<v>.stats    (L2 norm, largest magnitude) of the whole map
    <case>.attn.b<l>.<v>.l1       the sum of the whole map in fp64: a softmax row sums to 1, so this is its number of rows
    <case>.attn.b<l>.<v>.shape    the map's shape

The ragged case is the reference's own way with clips of different lengths: ONE CLIP AT A TIME at batch size 1, cropped to its
length (``ragged.<i>.*`` per clip, shapes (1, H, Nq, N) / (1, Nq, N)).  Weights and inputs are oracle/detgen.py streams, so the tests
regenerate them instead of storing them.

    python tests/golden/make_attn_golden.py        (CPU, about a minute)
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
from tests.golden import make_hidden_golden as HG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = 4096
# variant name -> (attn_rows, attn_heads) of PaSST.forward
VARIANTS = {"all.each": ("all", "each"), "all.mean": ("all", "mean"), "prefix.each": ("prefix", "each"), "prefix.mean": ("prefix", "mean")}

CASES = {
    # eval, the small net: the first and the last block (the last one is the prefix-only tail's)
    "eval": dict(cfg=O.make_cfg(**G.SMALL), B=2, T=250, training=False, seed=71, attn=(0, -1)),
    # train mode, structured + unstructured Patchout (patchout_train's geometry and seeding)
    "patchout_train": dict(cfg=HG.CASES["patchout_train"]["cfg"], B=3, T=250, training=True, seed=72, torch_seed=1234, attn=(0,)),
    # an intermediate block of a three-block net
    "three_blocks": dict(cfg=O.make_cfg(**dict(G.SMALL, depth=3)), B=2, T=250, training=False, seed=73, attn=(1,)),
}
# the ragged path: make_hidden_golden.RAGGED's clips (998, 437, 33 frames), each alone at batch size 1
RAGGED = dict(cfg=HG.RAGGED["cfg"], seed=75, lengths=list(HG.RAGGED["lengths"]), attn=(0, -1))


def inputs(case):
    cfg = case["cfg"]
    return detgen.uniform(case["seed"], "x", (case["B"], 1, cfg["img_size"][0], case["T"]), -1.5, 1.5)


def ragged_inputs():
    """x (B, 1, n_mels, max length) of the ragged case: clip i is its first lengths[i] frames."""
    return inputs(dict(RAGGED, B=len(RAGGED["lengths"]), T=max(RAGGED["lengths"])))


def block_of(a, depth):
    return a % depth


def variant_of(full, v):
    """The map PaSST.forward hands out for VARIANTS[v], from the full (B, H, N, N) one (fp64 in between)."""
    rows, heads = VARIANTS[v]
    m = full.astype(np.float64)
    if rows == "prefix":
        m = m[:, :, :2]
    if heads == "mean":
        m = m.mean(1)
    return m


def run_reference(m, x, attn):
    """(logits, features, [the (B, H, N, N) input of blocks[l].attn.attn_drop per entry of ``attn``])."""
    seen, hooks = {}, []
    for a in attn:
        hooks.append(m.blocks[a].attn.attn_drop.register_forward_hook(lambda _m, inp, _o, a=a: seen.__setitem__(a, inp[0].detach())))
    try:
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            logits, feat = ref_import.run_silently(m, torch.from_numpy(np.ascontiguousarray(x)))
    finally:
        for hk in hooks:
            hk.remove()
    return logits.numpy(), feat.numpy(), [seen[a].numpy() for a in attn]


def _maps_into(out, prefix, case, maps):
    depth = case["cfg"]["depth"]
    for a, full in zip(case["attn"], maps):
        for v in VARIANTS:
            k = f"{prefix}.attn.b{block_of(a, depth)}.{v}"
            m = variant_of(full, v)
            G._pinned_into(out, k, m, SAMPLE)
            out[k + ".l1"] = np.array(m.sum())
            out[k + ".shape"] = np.array(m.shape, np.int64)


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.train(case["training"])
        if "torch_seed" in case:
            torch.manual_seed(case["torch_seed"])
        logits, feat, maps = run_reference(m, inputs(case), case["attn"])
        out[name + ".logits"], out[name + ".features"] = logits, feat
        _maps_into(out, name, case, maps)
        print(name, [t.shape for t in maps])
    case = RAGGED
    m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
    m.eval()
    x = ragged_inputs()
    for i, n in enumerate(case["lengths"]):
        logits, feat, maps = run_reference(m, x[i:i + 1, :, :, :n], case["attn"])
        out[f"ragged.{i}.logits"], out[f"ragged.{i}.features"] = logits, feat
        _maps_into(out, f"ragged.{i}", case, maps)
        print("ragged", i, n, [t.shape for t in maps])
    np.savez_compressed(os.path.join(HERE, "attn.npz"), **out)


if __name__ == "__main__":
    main()

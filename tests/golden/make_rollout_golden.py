"""Fixture of the attention rollouts: tests/golden/rollout.npz, from the real reference implementation (kkoutini/PaSST, imported
read-only through oracle/ref_import.py exactly as make_attn_grad_golden.py does; none of its text is here).

Every case of make_attn_golden (same configurations, seeds, inputs) runs the reference ``PaSST`` with make_attn_grad_golden's hooks
on EVERY block and its loss, and the two recipes of INTEGRATION.md section 1.6 are evaluated in fp64 on the hooked (map, gradient)
pairs, blocks first to last, ``roll`` starting from the identity:

    attn:  a = 0.5 * mean_h A_l + 0.5 * I;   roll = (a / a.sum(-1)) @ roll                (attention rollout, Abnar & Zuidema)
    cam:   roll = roll + mean_h relu(A_l * dA_l) @ roll                                   (gradient-weighted rollout, Chefer et al.)

and the cls and dist rows ``roll[:, :2]`` are recorded whole, as fp64:

    <case>.<attn|cam>.from<k>           (B, 2, N): the product over blocks k .. depth-1  (k = 0; for three_blocks also k = 1)
    <case>.<attn|cam>.from<k>.shape     its shape

The ragged case is the reference's own way with clips of different lengths: ONE CLIP AT A TIME at batch size 1, cropped to its
length (``ragged.<i>.*`` per clip, loss rows i).  Weights and inputs are oracle/detgen.py streams, so the tests regenerate them
instead of storing them.

    python tests/golden/make_rollout_golden.py        (CPU, about a minute)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import detgen, ref_import  # noqa: E402
from tests.golden import make_attn_golden as AG  # noqa: E402
from tests.golden import make_attn_grad_golden as GG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CASES, RAGGED = AG.CASES, AG.RAGGED
FROM = {"three_blocks": (0, 1)}                    # case -> the first blocks recorded (default: block 0 only)


def first_blocks(name):
    return FROM.get(name, (0,))


def recipe_attn(maps, first=0):
    """Section 1.6's attention rollout in fp64 on the head-mean maps [(B, N, N) per block]: the (B, 2, N) cls / dist rows."""
    n = maps[0].shape[-1]
    eye = np.eye(n)
    roll = np.broadcast_to(eye, maps[0].shape).astype(np.float64)
    for a in maps[first:]:
        a = 0.5 * a.astype(np.float64) + 0.5 * eye
        roll = (a / a.sum(-1, keepdims=True)) @ roll
    return np.ascontiguousarray(roll[:, :2])


def recipe_cam(cams, first=0):
    """Section 1.6's gradient-weighted rollout in fp64 on [mean_h relu(A * dA) (B, N, N) per block]: the (B, 2, N) cls / dist rows."""
    roll = np.broadcast_to(np.eye(cams[0].shape[-1]), cams[0].shape).astype(np.float64)
    for c in cams[first:]:
        roll = roll + c.astype(np.float64) @ roll
    return np.ascontiguousarray(roll[:, :2])


def _into(out, prefix, firsts, pairs):
    maps = [p.astype(np.float64).mean(1) for p, _ in pairs]
    cams = [np.maximum(p.astype(np.float64) * g.astype(np.float64), 0.0).mean(1) for p, g in pairs]
    for k in firsts:
        for kind, r in (("attn", recipe_attn(maps, k)), ("cam", recipe_cam(cams, k))):
            out[f"{prefix}.{kind}.from{k}"] = r
            out[f"{prefix}.{kind}.from{k}.shape"] = np.array(r.shape, np.int64)


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.train(case["training"])
        if "torch_seed" in case:
            torch.manual_seed(case["torch_seed"])
        pairs = GG.run_reference(m, AG.inputs(case), *GG.loss_weights(case), range(case["cfg"]["depth"]))
        _into(out, name, first_blocks(name), pairs)
        print(name, [p.shape for p, _ in pairs])
    case = RAGGED
    m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
    m.eval()
    x = AG.ragged_inputs()
    a, b = GG.ragged_loss_weights()
    for i, n in enumerate(case["lengths"]):
        m.zero_grad()
        pairs = GG.run_reference(m, x[i:i + 1, :, :, :n], a[i:i + 1], b[i:i + 1], range(case["cfg"]["depth"]))
        _into(out, f"ragged.{i}", (0,), pairs)
        print("ragged", i, n, [p.shape for p, _ in pairs])
    np.savez_compressed(os.path.join(HERE, "rollout.npz"), **out)


if __name__ == "__main__":
    main()

"""Fixture of stochastic depth (drop_path_rate > 0): tests/golden/drop_path.npz, from the real reference implementation
(kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_golden.py does; none of its text is here).

The reference ``PaSST`` is built here with ``drop_path_rate`` (oracle.ref_import.build_reference_passt has no such argument): the
model is make_golden.SMALL three blocks deep at rate 0.5, so block 0 has no DropPath (linspace starts at 0), block 1 (p = 0.25) runs
on all rows and block 2 (p = 0.5) is the prefix-only tail of the kernel path.  Two cases at B = 6, train mode, on the CPU:

    plain      T = 250, no Patchout
    patchout   structured and unstructured Patchout: the Patchout draws and the mask draws interleave on ONE generator (the CPU's)

The masks are recorded with a forward hook on every ``DropPath`` (a clip's branch was kept <=> the module's output for it is
non-zero), one (B,) row per call, in call order: blocks ascending, attention branch then MLP branch.  The generator asserts that every
call keeps at least one clip and drops at least one, and that some clip is dropped in a block's attention branch and kept in its MLP
branch; the torch seeds below were chosen so that the reference's own draws satisfy this.  The loss is make_hidden_golden's,
``(logits * a).sum() + (features * b).sum()``, and a case records

    <case>.masks              (depth, 2, B) keep flags (rows of blocks without a DropPath are 1)
    <case>.logits  <case>.features
    <case>.dx                 pin_sample(dx, SAMPLE)            <case>.dx.stats = (L2 norm, largest magnitude) of all of dx
    <case>.grad.<parameter>   the same for PARAM_GRADS
    <case>.hidden.b1          pin_sample of the output of blocks[1] (what ``hidden=(1,)`` returns), with .stats and .shape

Weights and inputs are oracle/detgen.py streams, so the tests regenerate them instead of storing them.

    python tests/golden/make_drop_path_golden.py        (CPU, well under a minute)
"""
import contextlib
import io
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
SAMPLE = 2048
RATE, DEPTH, B = 0.5, 3, 6
HIDDEN = 1
PARAM_GRADS = ("patch_embed.proj.weight", "blocks.1.attn.qkv.weight", "blocks.1.attn.proj.bias", "blocks.1.mlp.fc2.bias",
               "blocks.2.attn.proj.bias", "blocks.2.mlp.fc2.bias", "blocks.1.norm2.weight")

CASES = {
    "plain": dict(cfg=O.make_cfg(**dict(G.SMALL, depth=DEPTH)), B=B, T=250, seed=81, torch_seed=5),
    "patchout": dict(cfg=O.make_cfg(**dict(G.SMALL, depth=DEPTH), s_patchout_t=6, s_patchout_f=3, u_patchout=5), B=B, T=250, seed=82,
                     torch_seed=3),
}


def build_reference(cfg, state_dict, rate=RATE):
    """The reference ``PaSST`` (models/passt.py:383) with ``drop_path_rate``, weights loaded."""
    ref_passt, _ = ref_import.load_reference()
    with contextlib.redirect_stdout(io.StringIO()):
        m = ref_passt.PaSST(u_patchout=cfg.get("u_patchout", 0), s_patchout_t=cfg.get("s_patchout_t", 0),
                            s_patchout_f=cfg.get("s_patchout_f", 0), img_size=tuple(cfg["img_size"]), patch_size=cfg.get("patch", 16),
                            stride=tuple(cfg["stride"]), in_chans=1, num_classes=cfg["num_classes"], embed_dim=cfg["embed_dim"],
                            depth=cfg["depth"], num_heads=cfg["num_heads"], distilled=True, drop_path_rate=rate)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state_dict.items()}, strict=True)
    return m


def active_blocks(m):
    """indices of the blocks whose drop_path is a DropPath with a rate (not nn.Identity)"""
    return [i for i, blk in enumerate(m.blocks) if getattr(blk.drop_path, "drop_prob", 0.0)]


def reference_step(m, case):
    """One train-mode forward + backward of the reference under the case's torch seed.  Returns (masks (depth, 2, B), logits, features,
    block-HIDDEN output, dx), numpy."""
    x, a, b = HG.inputs(case)
    calls, seen, hooks = [], {}, []
    for i in active_blocks(m):
        hooks.append(m.blocks[i].drop_path.register_forward_hook(
            lambda _m, _i, out, i=i: calls.append((i, (out.detach().reshape(out.shape[0], -1) != 0).any(1).numpy()))))
    hooks.append(m.blocks[HIDDEN].register_forward_hook(lambda _m, _i, out: seen.__setitem__("h", out.detach().numpy().copy())))
    xt = torch.from_numpy(np.ascontiguousarray(x)).requires_grad_()
    torch.manual_seed(case["torch_seed"])
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat = ref_import.run_silently(m, xt)
    finally:
        for hk in hooks:
            hk.remove()
    ((logits * torch.from_numpy(a)).sum() + (feat * torch.from_numpy(b)).sum()).backward()
    masks = np.ones((len(m.blocks), 2, case["B"]), np.float32)
    nth = {}
    for i, kept in calls:                   # call order within a block: attention branch, then MLP branch
        j = nth.get(i, 0)
        masks[i, j] = kept
        nth[i] = j + 1
    assert all(v == 2 for v in nth.values()) and sorted(nth) == active_blocks(m), nth
    return masks, logits.detach().numpy(), feat.detach().numpy(), seen["h"], xt.grad.numpy()


def masks_are_telling(masks, active):
    """every active call keeps a clip and drops one; some clip is dropped in a block's attention branch and kept in its MLP branch"""
    mixed = all(0 < masks[i, j].sum() < masks.shape[2] for i in active for j in range(2))
    crossed = any(((masks[i, 0] == 0) & (masks[i, 1] == 1)).any() for i in active)
    return bool(mixed and crossed)


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = build_reference(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.train()
        assert active_blocks(m) == [1, 2], active_blocks(m)
        masks, logits, feat, h, dx = reference_step(m, case)
        assert masks_are_telling(masks, active_blocks(m)), (name, masks)
        out[name + ".masks"] = masks
        out[name + ".logits"], out[name + ".features"] = logits, feat
        G._pinned_into(out, name + ".dx", dx, SAMPLE)
        G._pinned_into(out, f"{name}.hidden.b{HIDDEN}", h, SAMPLE)
        out[f"{name}.hidden.b{HIDDEN}.shape"] = np.array(h.shape, np.int64)
        params = dict(m.named_parameters())
        for k in PARAM_GRADS:
            G._pinned_into(out, f"{name}.grad.{k}", params[k].grad.numpy(), SAMPLE)
        print(name, "masks", masks[1:].astype(int).tolist(), "dx norm / absmax", out[name + ".dx.stats"])
    np.savez_compressed(os.path.join(HERE, "drop_path.npz"), **out)


if __name__ == "__main__":
    main()

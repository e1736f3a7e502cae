"""Fixture of attention dropout: tests/golden/attn_dropout.npz, from the real reference implementation (kkoutini/PaSST, imported
read-only through oracle/ref_import.py exactly as make_golden.py does; none of its text is here).

The reference puts an ``nn.Dropout`` on the attention probabilities (``attn = attn.softmax(-1); attn = self.attn_drop(attn)``).  Its
element-wise draws cannot be reproduced on the device, so the mask is a pure function of a seed and the element's position
(include/passt_amd.h, "attention dropout").  Here every ``blocks[i].attn.attn_drop`` of the reference ``PaSST`` is REPLACED by a
module that multiplies the probabilities by ``passt_amd.attn_drop_mask(SEED, i, B, H, N, N, p) / keep`` -- the host restatement of the
rule, keep = 1 - round(256 p) / 256 -- and the reference's own forward and backward do the rest.  The model is make_golden.SMALL three
blocks deep, train mode, on the CPU: block 0 inactive (p = 0), block 1 p = 0.25 (t = 64), block 2 -- the prefix-only tail of the
kernel path, which computes the cls / dist query rows only; the mask of a row does not depend on how many rows are computed --
p = 0.5 (t = 128).  Two cases at B = 3:

    plain      T = 250, no Patchout
    patchout   structured and unstructured Patchout (the token count is the draws')

The loss is make_hidden_golden's, ``(logits * a).sum() + (features * b).sum()``, and a case records

    <case>.logits  <case>.features
    <case>.dx                 pin_sample(dx, SAMPLE)            <case>.dx.stats = (L2 norm, largest magnitude) of all of dx
    <case>.grad.<parameter>   the same for PARAM_GRADS
    <case>.kept               per active block: the kept fraction of its mask (the generator asserts it lies within 5 sigma of keep)

Weights and inputs are oracle/detgen.py streams, so the tests regenerate them instead of storing them.

    python tests/golden/make_attn_dropout_golden.py        (CPU, needs the built library for the host mask; well under a minute)
"""
import math
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
DEPTH, B = 3, 3
SEED = (0x1234ABCD, 0x9F1E2D3C)
RATES = (0.0, 0.25, 0.5)                # blocks[i].attn.attn_drop.p: t = 0, 64, 128
PARAM_GRADS = ("patch_embed.proj.weight", "blocks.0.mlp.fc2.bias", "blocks.1.attn.qkv.weight", "blocks.1.attn.qkv.bias", "blocks.1.attn.proj.weight",
               "blocks.2.attn.qkv.weight", "blocks.2.attn.proj.bias", "blocks.1.norm1.weight")

CASES = {
    "plain": dict(cfg=O.make_cfg(**dict(G.SMALL, depth=DEPTH)), B=B, T=250, seed=91, torch_seed=5),
    "patchout": dict(cfg=O.make_cfg(**dict(G.SMALL, depth=DEPTH), s_patchout_t=6, s_patchout_f=3, u_patchout=5), B=B, T=250, seed=92,
                     torch_seed=3),
}


class RuleDropout(torch.nn.Module):
    """stands in for a block's ``attn_drop``: probabilities (B, H, N, N) times mask / keep, the mask from the host entry"""

    def __init__(self, site, p, seen):
        super().__init__()
        self.site, self.p, self.seen = site, p, seen

    def forward(self, attn):
        from passt_amd import ops
        Bc, H, nq, N = attn.shape
        t = ops.attn_drop_t(self.p)
        mask = ops.attn_drop_mask(SEED, self.site, Bc, H, nq, N, self.p)
        self.seen[self.site] = (float(mask.float().mean()), mask.numel(), t)
        return attn * (mask.to(attn.dtype) / (1.0 - t / 256.0))


def reference_step(m, case):
    """One train-mode forward + backward of the reference with the rule's masks.  Returns (logits, features, dx, kept), numpy."""
    x, a, b = HG.inputs(case)
    seen = {}
    for i, blk in enumerate(m.blocks):
        if RATES[i] > 0:
            blk.attn.attn_drop = RuleDropout(i, RATES[i], seen)
    xt = torch.from_numpy(np.ascontiguousarray(x)).requires_grad_()
    torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, feat = ref_import.run_silently(m, xt)
    ((logits * torch.from_numpy(a)).sum() + (feat * torch.from_numpy(b)).sum()).backward()
    return logits.detach().numpy(), feat.detach().numpy(), xt.grad.numpy(), seen


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.train()
        logits, feat, dx, seen = reference_step(m, case)
        assert sorted(seen) == [1, 2], seen
        for i, (frac, n, t) in seen.items():
            keep = 1.0 - t / 256.0
            assert abs(frac - keep) <= 5 * math.sqrt(keep * (1 - keep) / n), (name, i, frac, keep)
        out[name + ".kept"] = np.array([seen[i][0] for i in (1, 2)])
        out[name + ".logits"], out[name + ".features"] = logits, feat
        G._pinned_into(out, name + ".dx", dx, SAMPLE)
        params = dict(m.named_parameters())
        for k in PARAM_GRADS:
            G._pinned_into(out, f"{name}.grad.{k}", params[k].grad.numpy(), SAMPLE)
        print(name, "kept", out[name + ".kept"], "dx norm / absmax", out[name + ".dx.stats"])
    np.savez_compressed(os.path.join(HERE, "attn_dropout.npz"), **out)


if __name__ == "__main__":
    main()

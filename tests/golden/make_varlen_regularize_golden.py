"""Fixture of stochastic depth and attention dropout on ragged training batches: tests/golden/varlen_regularize.npz, from the real
reference implementation (kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_varlen_train_golden.py
does; none of its text is here).

The contract of ``net.varlen_regularize = True`` is that a ragged batch of B clips is regularised as the fixed path regularises a batch
of B clips: clip b gets entry b of the (depth, 2, B) drop-path factors on all of its rows, and the attention mask of sequence b -- the
rule of include/passt_amd.h at s = b*H + h, with q and k the positions inside the clip.  Patchout keeps its clip-after-clip draws.  So,
combining make_varlen_train_golden.py and make_attn_dropout_golden.py, the reference ``PaSST.train()`` runs ONE CLIP AT A TIME, cropped
to its length, under ONE ``torch.manual_seed`` per case, with

    every active ``blocks[i].attn.attn_drop`` REPLACED by a module that multiplies the probabilities of clip b by
        ``passt_amd.attn_drop_mask(SEED, i, b + 1, H, N, N, p)[b] / keep``            (keep = 1 - round(256 p) / 256)
    every active ``blocks[i].drop_path``      REPLACED by a module that multiplies a branch of clip b by
        ``FLAGS[i, branch, b] / keep``                                               (keep = 1 - the block's drop-path rate)

neither of which draws, so the generator sees the Patchout draws only.  The model is make_varlen_train_golden.MODEL three blocks deep
with ``drop_path_rate = 0.5`` (linspace: 0, 0.25, 0.5): block 0 inactive, block 1 attention p = 0.25 (t = 64), block 2 -- the prefix-only
tail of the kernel path -- attention p = 0.5 (t = 128).  The flags are chosen by hand (CASES) so that every active (block, branch) keeps
a clip and drops one and every clip is dropped at least once and kept at least once; main() asserts both, and per clip and active block
that the mask holds kept and dropped elements with a kept fraction within 5 sigma of keep.

The loss is make_varlen_grad_golden's, ``(logits * a).sum() + (features * b).sum()``, every parameter and the input requiring a
gradient, and a case records make_varlen_train_golden's keys (logits, features, dx.<i> pinned per clip, grad.<parameter> pinned and
summed over the clips, rng, the index part) plus

    <case>.flags        (depth, 2, B) keep flags: what ``drop_path_masks=`` takes
    <case>.kept         (clips, 2): the kept fraction of the masks of blocks 1 and 2

``attn_drop_seed=SEED`` replays the masks.  Weights and inputs are oracle/detgen.py streams, so the tests regenerate them.

    python tests/golden/make_varlen_regularize_golden.py        (CPU, needs the built library for the host mask; about a minute)
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
from tests.golden import make_drop_path_golden as DG  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_train_golden as VT  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = VT.SAMPLE
SEED = (0x51F15E3D, 0x0BADC0DE)
DEPTH = 3
DROP_PATH_RATE = 0.5                    # the constructor's linspace gives the blocks 0, 0.25, 0.5
ATTN_RATES = (0.0, 0.25, 0.5)           # blocks[i].attn.attn_drop.p: t = 0, 64, 128
ACTIVE = (1, 2)
MODEL = dict(VT.MODEL, depth=DEPTH)


def _flags(b1_attn, b1_mlp, b2_attn, b2_mlp):
    B = len(b1_attn)
    return np.array([[[1] * B, [1] * B], [b1_attn, b1_mlp], [b2_attn, b2_mlp]], np.float32)


CASES = {
    "a": dict(cfg=O.make_cfg(**MODEL, u_patchout=7), lengths=(16, 56, 106, 300), seed=61, torch_seed=2027,
              flags=_flags([1, 0, 1, 1], [0, 1, 1, 0], [1, 1, 0, 1], [1, 1, 1, 0])),
    "b": dict(cfg=O.make_cfg(**MODEL, s_patchout_t=2, s_patchout_f=3), lengths=(56, 106, 250), seed=62, torch_seed=2028,
              flags=_flags([0, 1, 1], [1, 0, 1], [1, 1, 0], [1, 0, 1])),
}
inputs = VT.inputs
loss_of = VT.loss_of


def param_grads(cfg):
    return VT.param_grads(cfg) + ("blocks.1.attn.qkv.weight", "blocks.1.attn.proj.weight", "blocks.1.mlp.fc2.weight", "blocks.1.mlp.fc2.bias",
                                  "blocks.2.attn.qkv.weight", "blocks.2.attn.proj.bias", "blocks.1.norm2.weight")


def flags_are_telling(flags):
    """every active (block, branch) keeps a clip and drops one; every clip is dropped at least once and kept at least once"""
    act = flags[list(ACTIVE)]
    B = flags.shape[2]
    mixed = all(0 < act[i, j].sum() < B for i in range(len(ACTIVE)) for j in range(2))
    per_clip = act.reshape(-1, B)
    return bool(mixed and (per_clip.min(0) == 0).all() and (per_clip.max(0) == 1).all())


class _Clip:
    """which clip of the batch the reference is running (the stand-in modules read it)"""
    b = 0


class RuleDropout(torch.nn.Module):
    """stands in for a block's ``attn_drop``: the probabilities (1, H, N, N) of clip b times mask / keep, the mask that of sequence b"""

    def __init__(self, site, p, clip, seen):
        super().__init__()
        self.site, self.p, self.clip, self.seen = site, p, clip, seen

    def forward(self, attn):
        from passt_amd import ops
        one, H, nq, N = attn.shape
        assert one == 1
        t = ops.attn_drop_t(self.p)
        mask = ops.attn_drop_mask(SEED, self.site, self.clip.b + 1, H, nq, N, self.p)[self.clip.b]
        self.seen[(self.clip.b, self.site)] = (float(mask.float().mean()), mask.numel(), t, bool(mask.any()), bool((~mask).any()))
        return attn * (mask.to(attn.dtype) / (1.0 - t / 256.0)).unsqueeze(0)


class FlagDropPath(torch.nn.Module):
    """stands in for a block's ``drop_path`` (one module, called for the attention branch and then for the MLP branch)"""

    def __init__(self, flags_i, keep, clip):
        super().__init__()
        self.flags_i, self.keep, self.clip, self.calls = flags_i, keep, clip, 0

    def forward(self, x):
        branch = self.calls % 2
        self.calls += 1
        return x * (float(self.flags_i[branch, self.clip.b]) / self.keep)


def run_case(case):
    cfg, lengths, flags = case["cfg"], case["lengths"], case["flags"]
    m = DG.build_reference(cfg, detgen.passt_state_dict(cfg, case["seed"]), rate=DROP_PATH_RATE)
    m.train()
    assert DG.active_blocks(m) == list(ACTIVE)
    clip, seen, paths = _Clip(), {}, {}
    for i in ACTIVE:
        blk = m.blocks[i]
        paths[i] = blk.drop_path = FlagDropPath(flags[i], 1.0 - float(blk.drop_path.drop_prob), clip)
        blk.attn.attn_drop = RuleDropout(i, ATTN_RATES[i], clip, seen)
    x, a, b = inputs(case)
    out, lo, fe, logs = {}, [], [], []
    torch.manual_seed(case["torch_seed"])
    for i, n in enumerate(lengths):
        clip.b = i
        xt = torch.from_numpy(np.ascontiguousarray(x[i:i + 1, :, :, :n])).requires_grad_()
        with warnings.catch_warnings(), VT._Draws() as d:
            warnings.simplefilter("ignore")
            logits, feat = ref_import.run_silently(m, xt)[:2]
        logs.append(d.log)
        loss_of(logits, feat, torch.from_numpy(a[i:i + 1]), torch.from_numpy(b[i:i + 1])).backward()
        lo.append(logits.detach().numpy()[0])
        fe.append(feat.detach().numpy()[0])
        G._pinned_into(out, f"dx.{i}", xt.grad.numpy(), SAMPLE)
        out[f"dx.{i}.nonzero"] = np.array(int(np.count_nonzero(xt.grad.numpy())), np.int64)
    assert all(p.calls == 2 * len(lengths) for p in paths.values())
    out["rng"] = torch.get_rng_state().numpy().copy()
    out["logits"], out["features"] = np.stack(lo), np.stack(fe)
    params = dict(m.named_parameters())
    for k in param_grads(cfg):
        G._pinned_into(out, f"grad.{k}", params[k].grad.numpy(), SAMPLE)
    out.update(VT.rows_from_draws(cfg, lengths, logs))
    out["flags"] = flags
    kept = np.zeros((len(lengths), len(ACTIVE)))
    for (bi, site), (frac, n, t, any_kept, any_dropped) in seen.items():
        keep = 1.0 - t / 256.0
        assert any_kept and any_dropped, (bi, site)
        assert abs(frac - keep) <= 5 * math.sqrt(keep * (1 - keep) / n), (bi, site, frac, keep, n)
        kept[bi, ACTIVE.index(site)] = frac
    assert len(seen) == len(lengths) * len(ACTIVE)
    out["kept"] = kept
    return out


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        assert flags_are_telling(case["flags"]), name
        res = run_case(case)
        out.update({f"{name}.{k}": v for k, v in res.items()})
        print(name, "tokens per clip", np.diff(res["cu_tok"]).tolist(), "kept", res["kept"].round(3).tolist(),
              "max|dx| per clip", [float(res[f"dx.{i}.stats"][1]) for i in range(len(case["lengths"]))])
    np.savez_compressed(os.path.join(HERE, "varlen_regularize.npz"), **out)


if __name__ == "__main__":
    main()

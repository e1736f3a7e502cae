"""GPU tests of stochastic depth and attention dropout on ragged training batches (``net.varlen_regularize = True``), the model on top of
pa_attention_fwd_varlen_dropout / pa_attention_bwd_varlen_dropout (tests/test_gpu_attention_varlen_dropout.py has the kernels).

Contract: a ragged batch of B clips is regularised as the fixed path regularises a batch of B clips -- clip b gets entry b of the (depth,
2, B) drop-path factors on all of its rows and the attention mask of sequence b.  Reference values: tests/golden/varlen_regularize.npz
(the real reference in training mode, one clip at a time under one seed, the masks put in by stand-in modules,
tests/golden/make_varlen_regularize_golden.py).  Errors are taken per clip as tests/test_gpu_varlen_train.py takes them, and the bounds
are that file's: 1e-3 in fp32, BF16_LOGITS / BF16_GRADS of tests/test_gpu_model.py in bf16; the TrainStep comparison has the bounds of
tests/test_gpu_varlen_step.py::test_ragged_step_matches_the_autograd_path (loss 1e-5, parameters 2e-4).  Every figure is printed and
recorded (record(...)) before it is asserted.

Measured on MI355X: fp32 logits / features 1.1e-6, dx 1.9e-6, parameter gradients <= 2.1e-6; bf16 logits 3.6e-3, features 4.5e-3, dx
6.9e-3, parameter gradients <= 5.1e-3; the step against the drop-in path: loss difference 6.0e-8, parameters identical.

Every test fails on the parent commit at the NotImplementedError of a ragged batch with an active regulariser."""
import functools
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
import passt_amd.optim  # noqa: E402
from oracle import detgen  # noqa: E402
from passt_amd import passt as P  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_regularize_golden as VR  # noqa: E402
from tests.golden import make_varlen_train_golden as VT  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, BF16_LOGITS, record, rel  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "varlen_regularize.npz")


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(GOLDEN))


def _net(case, precision):
    """the fixture's model: drop_path_rate at construction, attention dropout set on the modules; training mode, both switches on"""
    cfg = case["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.PaSST(u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"], s_patchout_f=cfg["s_patchout_f"],
                            img_size=cfg["img_size"], patch_size=cfg["patch"], stride=cfg["stride"], num_classes=cfg["num_classes"],
                            embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], distilled=True,
                            drop_path_rate=VR.DROP_PATH_RATE)
    sd = detgen.passt_state_dict(cfg, case["seed"])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    for blk, p in zip(m.blocks, VR.ATTN_RATES):
        blk.attn.attn_drop.p = p
    m.precision = precision
    m = m.to(DEV).train()
    m.varlen_train = m.varlen_regularize = True
    assert P.drop_path_rates(m) == [0.0, 0.25, 0.5] and P.attn_drop_rates(m) == [0, 64, 128]
    return m


def _io(case):
    """x with NaN behind every clip's length, and the loss rows"""
    x, a, b = VR.inputs(case)
    x = torch.from_numpy(x)
    for i, n in enumerate(case["lengths"]):
        x[i, :, :, n:] = float("nan")
    return x.to(DEV), torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)


def _replay(case, seed=VR.SEED):
    return dict(drop_path_masks=torch.from_numpy(case["flags"]), attn_drop_seed=seed)


def _step(m, case, x, a, b, route="autograd", rows=None, **kw):
    """one forward + backward under the case's torch seed.  Returns (logits, features, dx, {name: gradient})."""
    lengths = list(case["lengths"])
    if rows is not None:                        # loss weights of the other clips zero
        keep = torch.zeros(len(lengths), 1, device=DEV)
        keep[rows] = 1.0
        a, b = a * keep, b * keep
    torch.manual_seed(case["torch_seed"])
    m.zero_grad()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if route == "autograd":
            xg = x.clone().requires_grad_()
            logits, feat = m(xg, lengths=lengths, **kw)
            VT.loss_of(logits, feat, a, b).backward()
            return logits.detach(), feat.detach(), xg.grad, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        logits, feat, ctx = P.passt_forward_varlen_replay(m, x, lengths, save=True, **kw)
        grads = {k: torch.full_like(p, float("nan")) for k, p in m.named_parameters() if not k.startswith("head_dist.")}
        dx = P.passt_backward_varlen(m, ctx, a.contiguous(), b.contiguous(), grads, want_dx=True)
        return logits, feat, dx, grads


# ---- 1. against the fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["autograd", "direct"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(VR.CASES))
def test_model_vs_reference(name, precision, route):
    """Both cases, both precisions, through ``net(x, lengths=)`` + autograd and through passt_forward_varlen_replay / passt_backward_varlen, with
    drop_path_masks= and attn_drop_seed= set to the fixture's: logits, features and dx per clip, the parameter gradients summed over the
    clips, the CPU generator's final state (the Patchout draws only)."""
    gold, case = _gold(), VR.CASES[name]
    cfg, lengths = case["cfg"], case["lengths"]
    m = _net(case, precision)
    x, a, b = _io(case)
    logits, feat, dx, grads = _step(m, case, x, a, b, route, **_replay(case))
    torch.cuda.synchronize()
    dev_state = torch.cuda.get_rng_state()
    assert np.array_equal(torch.get_rng_state().numpy(), gold[f"{name}.rng"])        # the Patchout draws of the clip-by-clip loop only
    assert torch.equal(dev_state, _seeded_device_state(case["torch_seed"]))          # a replay draws nothing on the device
    assert dx is not None and dx.shape == x.shape and dx.dtype == torch.float32
    assert torch.isfinite(logits).all() and torch.isfinite(feat).all() and torch.isfinite(dx).all()     # the NaN behind the lengths is never read
    w = dict(logits=0.0, features=0.0, dx=0.0, dx_norm=0.0)
    cu = gold[f"{name}.cu_tok"]
    for i, n in enumerate(lengths):
        key = f"{name}.dx.{i}"
        nrm, scale = (float(v) for v in gold[key + ".stats"])
        got = dx[i:i + 1, :, :, :n].cpu().numpy()
        e = dict(logits=rel(logits[i].cpu(), gold[f"{name}.logits"][i]), features=rel(feat[i].cpu(), gold[f"{name}.features"][i]),
                 dx=float(np.abs(G.pin_sample(got, VR.SAMPLE) - gold[key]).max()) / scale,
                 dx_norm=abs(float(np.linalg.norm(got.astype(np.float64))) - nrm) / nrm)
        print(f"varlen_regularize.{name}[{precision},{route}] clip {i} len {n}: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
        for k, v in e.items():
            w[k] = max(w[k], v)
        rows = slice(int(cu[i]) + 2, int(cu[i + 1]))
        mask = torch.from_numpy(VT.covered(cfg, n, gold[f"{name}.row_f"][rows], gold[f"{name}.row_t"][rows])).to(DEV)
        assert float(dx[i, :, :, n:].abs().max() if n < dx.shape[-1] else 0.0) == 0.0, i
        assert float(dx[i, 0, :, :n][~mask].abs().max() if not bool(mask.all()) else 0.0) == 0.0, i
    for k in VR.param_grads(cfg):
        key = f"{name}.grad.{k}"
        w["grad." + k] = float(np.abs(G.pin_sample(grads[k].cpu().numpy(), VR.SAMPLE) - gold[key]).max()) / float(gold[key + ".stats"][1])
    record(f"varlen_regularize.{name}[{precision},{route}]", **w)
    print(f"varlen_regularize.{name}[{precision},{route}]", w)
    lim_out, lim_g = (1e-3, 1e-3) if precision == "fp32" else (BF16_LOGITS, BF16_GRADS)
    for k, v in w.items():
        assert v < (lim_out if k in ("logits", "features") else lim_g), (k, v, w)


def _seeded_device_state(seed):
    torch.manual_seed(seed)
    return torch.cuda.get_rng_state()


# ---- 2. replay, the draws, eval mode ----------------------------------------------------------------------------------------------------
def _bits_equal(r1, r2):
    return (torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and torch.equal(r1[2], r2[2]) and set(r1[3]) == set(r2[3])
            and all(torch.equal(r1[3][k], r2[3][k]) for k in r1[3]))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_replay_is_bit_identical_and_the_seed_matters(precision):
    case = VR.CASES["b"]
    m = _net(case, precision)
    x, a, b = _io(case)

    def run(**kw):
        lo, fe, dx, g = _step(m, case, x, a, b, **kw)
        return lo.clone(), fe.clone(), dx.clone(), {k: v.clone() for k, v in g.items()}
    r1, r2 = run(**_replay(case)), run(**_replay(case))
    assert _bits_equal(r1, r2)
    r3 = run(**_replay(case, seed=(VR.SEED[0] ^ 1, VR.SEED[1])))
    assert not torch.equal(r1[0], r3[0]) and not torch.equal(r1[2], r3[2])
    flipped = case["flags"].copy()
    flipped[1, 1] = 1 - flipped[1, 1]
    r4 = run(drop_path_masks=torch.from_numpy(flipped), attn_drop_seed=VR.SEED)
    assert not torch.equal(r1[0], r4[0])
    # drawn, not replayed: after one seed the device generator ends where a fixed forward of the same B leaves it, and the factors
    # and the seed are those of drop_path_draws / attn_drop_draw in that order
    B, T = len(case["lengths"]), max(case["lengths"])
    run()
    ragged_state = torch.cuda.get_rng_state()
    torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        m(torch.nan_to_num(x[:, :, :, :T]))
    assert torch.equal(torch.cuda.get_rng_state(), ragged_state)
    torch.manual_seed(case["torch_seed"])
    scales = P.drop_path_draws(m, B, x.device)
    seed = P.attn_drop_draw(x.device)
    assert torch.equal(torch.cuda.get_rng_state(), ragged_state)
    r5, r6 = run(), run(drop_path_masks=(scales > 0).float(), attn_drop_seed=seed)
    assert _bits_equal(r5, r6)


def test_eval_mode_does_not_see_the_switch():
    case = VR.CASES["a"]
    m = _net(case, "bf16").eval()
    x, _, _ = _io(case)
    lengths = list(case["lengths"])
    state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo1, fe1 = m(x, lengths=lengths)
        lo2, fe2 = m(x, lengths=lengths, **_replay(case))              # the keywords are ignored without an active rate
        m.varlen_regularize = False
        lo0, fe0 = m(x, lengths=lengths)
    assert torch.equal(lo0, lo1) and torch.equal(fe0, fe1) and torch.equal(lo0, lo2) and torch.equal(fe0, fe2)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(torch.cuda.get_rng_state(), dev_state)
    # and the switch off in training mode is the refusal
    m.train()
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        m(x, lengths=lengths)
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(torch.cuda.get_rng_state(), dev_state)


# ---- 3. a dropped branch gets no gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dropped_branch_has_exactly_zero_weight_gradient(precision):
    """Clip 0 of case "a": the MLP branch of block 1 dropped, its attention branch kept.  With the other clips' loss weights zero, the
    gradient of blocks.1.mlp.* is exactly 0, and that of blocks.1.attn.proj.weight is not."""
    case = VR.CASES["a"]
    assert case["flags"][1, 1, 0] == 0 and case["flags"][1, 0, 0] == 1
    m = _net(case, precision)
    x, a, b = _io(case)
    for route in ("autograd", "direct"):
        _, _, dx, g = _step(m, case, x, a, b, route, rows=[0], **_replay(case))
        for k in ("blocks.1.mlp.fc2.weight", "blocks.1.mlp.fc1.weight", "blocks.1.mlp.fc1.bias", "blocks.1.norm2.weight"):
            assert float(g[k].abs().max()) == 0.0, (route, k)
        assert float(g["blocks.1.attn.proj.weight"].abs().max()) > 0 and float(g["blocks.2.mlp.fc2.weight"].abs().max()) > 0
        assert float(dx[1:].abs().max()) == 0.0 and float(dx[0].abs().max()) > 0


# ---- 4. the training step ----------------------------------------------------------------------------------------------------------------
def test_train_step_with_both_regularisers_matches_the_drop_in_path():
    """One ragged step, fp32, drawn regularisers, clipping that bites, block 0 frozen: TrainStep.step(x, y, lengths=) against
    net(x, lengths=) + BCE + loss.backward() + passt_amd.optim.AdamW(max_grad_norm=c).step() under the same seeds."""
    from passt_amd.train import TrainStep
    case = VR.CASES["a"]
    lengths, cfg = list(case["lengths"]), case["cfg"]
    lr, wd, seed = 1e-3, 1e-2, 50
    m1, m2 = _net(case, "fp32"), _net(case, "fp32")
    for m in (m1, m2):
        m.blocks[0].requires_grad_(False)
    x, _, _ = _io(case)
    y = torch.from_numpy((detgen.uniform(case["seed"], "y", (len(lengths), cfg["num_classes"]), 0.0, 1.0) < 0.1).astype(np.float32)).to(DEV)
    named = [(n, p) for n, p in m1.named_parameters() if p.requires_grad and not n.startswith("head_dist.")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(seed)
        lg, _ = m1(x, lengths=lengths)
        loss1 = torch.nn.functional.binary_cross_entropy_with_logits(lg, y, reduction="none").mean()
        loss1.backward()
        state, dev_state = torch.get_rng_state(), torch.cuda.get_rng_state()
        norm1 = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for _, p in named))
        c = 0.5 * norm1
        opt = passt_amd.optim.AdamW([p for _, p in named], lr=lr, weight_decay=wd, max_grad_norm=c)
        opt.step()
        ts = TrainStep(m2, None, lr=lr, weight_decay=wd, use_mixup=False, clip_grad_norm=c)
        assert [n for n, _ in ts.named] == [n for n, _ in named]
        torch.manual_seed(seed)
        loss2 = ts.step(x, y, lengths=lengths)
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), state) and torch.equal(torch.cuda.get_rng_state(), dev_state)      # the same draws
    d, norm2, coef2 = abs(loss1.item() - loss2.item()), float(ts.grad_norm), float(ts._clip_out[1])
    wp = max(rel(p2.detach().cpu(), p1.detach().cpu()) for (_, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()))
    record("varlen_regularize.step_vs_drop_in[fp32]", loss=d, params=wp, norm_rel=abs(norm2 - norm1) / norm1, factor=coef2)
    print(f"varlen_regularize.step: losses {loss1.item():.7f} {loss2.item():.7f} diff {d:.2e}, norm {norm1:.6e} / {norm2:.6e}, factor {coef2:.4f}, "
          f"worst parameter rel {wp:.2e}")
    assert math.isfinite(loss2.item()) and ts.t == 1
    assert coef2 < 1.0                                                  # the clipping bites
    assert d < 1e-5 and wp < 2e-4, (d, wp)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    assert all(torch.equal(sd1[k], sd2[k]) for k in sd1 if k.startswith("blocks.0."))      # frozen: never written
    ts.close()

"""GPU tests of Patchout training on ragged batches (``net.train(); net.varlen_train = True; net(x, lengths=...)``): the two slot-table
kernels of the packed patch-stage backward, and the model on top.

Contract: every clip gets what it would get alone at batch size 1 in training mode, the Patchout draws being made clip after clip with
the reference's RNG calls.  Reference values: tests/golden/varlen_train.npz (the real reference in training mode, one clip at a time
under one seed, tests/golden/make_varlen_train_golden.py).  Errors in dx are taken per clip, relative to that clip's own largest entry.
Bounds are the project's own: tests.test_gpu_kernels.tol for the kernels, 1e-3 (fp32) and BF16_LOGITS / BF16_GRADS of
tests/test_gpu_model.py for the model.  No MI355X figures yet: none could be taken when this was written; every test
prints and records (record(...)) what it measures before it asserts.
"""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib, ops  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_train_golden as VT  # noqa: E402
from tests.test_gpu_kernels import TD, rel_err, rnd, tol  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, BF16_LOGITS, build, record, rel  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "varlen_train.npz")


# ---- 1. the kernels against a numpy restatement -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout(stride):
    """B = 3 clips of 1 / 5 / 24 patch columns on a 64-bin spectrogram, P = 16: clip 0 keeps a single patch, clip 1 about two thirds, clip
    2 about two thirds with two whole columns and one whole frequency row gone.  Every clip has its own non-zero offset into a
    26-position time embedding.  Returns the host arrays and the numbers that go with them."""
    P, F, Tpe = 16, 64, 26
    Fg, cols = (F - P) // stride + 1, (1, 5, 24)
    T_max = (max(cols) - 1) * stride + P + 5            # 251 / 389: odd, so rows of dx straddle the four-element vectors
    gen = np.random.default_rng(7 + stride)
    slot = np.full((3, Fg, max(cols)), -1, np.int32)
    row_f, row_t, row_clip, cu = [], [], [], [0]
    for b, T in enumerate(cols):
        keep = gen.random((Fg, T)) < 0.66
        if b == 0:
            keep[:] = False
            keep[Fg - 2, 0] = True
        if b == 2:
            keep[:, [3, 17]] = False
            keep[1, :] = False
        f, t = np.nonzero(keep)                         # frequency-major, like the sequence order
        slot[b, f, t] = cu[-1] + 2 + np.arange(f.size)
        row_f += [-1, -1] + f.tolist()
        row_t += [0, 1] + t.tolist()
        row_clip += [b] * (2 + f.size)
        cu.append(len(row_f))
    return dict(P=P, F=F, Tpe=Tpe, Fg=Fg, Tg=max(cols), T_max=T_max, stride=stride, slot=slot, cu=np.array(cu, np.int32),
                toff=np.array([25, 4, 2], np.int32), row_f=np.array(row_f), row_t=np.array(row_t), row_clip=np.array(row_clip), M=cu[-1])


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("stride", [10, 16])
def test_patch_input_bwd_rows_vs_numpy(stride, dt):
    """stride 10: overlapping patches (several kept patches add into one pixel); stride 16: they tile.  dx is pre-filled with NaN, so an
    element the kernel does not write fails."""
    L = _layout(stride)
    P, F, T_max, M = L["P"], L["F"], L["T_max"], L["M"]
    dcols = rnd(M, P * P, seed=stride).to(TD[dt])
    want = np.zeros((3, F, T_max))
    mask = np.zeros((3, F, T_max), bool)
    src = dcols.double().numpy().reshape(M, P, P)
    for r in range(M):
        if L["row_f"][r] >= 0:
            b, f0, t0 = L["row_clip"][r], L["row_f"][r] * stride, L["row_t"][r] * stride
            want[b, f0:f0 + P, t0:t0 + P] += src[r]
            mask[b, f0:f0 + P, t0:t0 + P] = True
    slot = torch.from_numpy(L["slot"]).to(DEV)
    dx = torch.full((3, 1, F, T_max), float("nan"), device=DEV)
    assert ops.patch_input_bwd_rows(dcols.to(DEV), slot, F, T_max, P, stride, stride, out=dx) is dx
    torch.cuda.synchronize()
    got = dx[:, 0].double().cpu().numpy()
    assert np.isfinite(got).all()
    assert (got[~mask] == 0).all()                      # exactly 0 where no kept patch covers: dropped, behind the clip, the single-patch clip
    assert mask[0].sum() == P * P and (got[0][mask[0]] != 0).all()
    e = rel_err(torch.from_numpy(got), torch.from_numpy(want))
    record(f"patch_input_bwd_rows[s{stride},{'f32' if dt == PA_F32 else 'bf16'}]", err=e)
    print(f"patch_input_bwd_rows stride {stride} dtype {dt}: rel err {e:.3e}")
    assert e < tol(dt), e
    dx2 = ops.patch_input_bwd_rows(dcols.to(DEV), slot, F, T_max, P, stride, stride)
    torch.cuda.synchronize()
    assert dx2.shape == dx.shape and torch.equal(dx, dx2)       # two runs bit-identical
    with pytest.raises(_lib.PasstAmdError):
        ops.patch_input_bwd_rows(dcols.to(DEV), slot[:, :-1], F, T_max, P, stride, stride)      # the table's rows are the patch grid's


@pytest.mark.parametrize("stride", [10, 16])
def test_patch_bwd_rows_vs_numpy(stride):
    L = _layout(stride)
    Fg, Tpe, M, D = L["Fg"], L["Tpe"], L["M"], 72                # D is no multiple of the 16 channels of a workgroup
    dtok = rnd(M, D, seed=3 + stride)
    d64 = dtok.double().numpy()
    patch = L["row_f"] >= 0
    tpos_col = L["row_t"] + L["toff"][L["row_clip"]]
    assert tpos_col[patch].max() == Tpe - 1                     # the single-patch clip sits on the last time position
    want = dict(bias=d64[patch].sum(0), cls=d64[L["cu"][:-1]].sum(0), dist=d64[L["cu"][:-1] + 1].sum(0),
                tpos=np.zeros((Tpe, D)), fpos=np.zeros((Fg, D)))
    np.add.at(want["tpos"], tpos_col[patch], d64[patch])
    np.add.at(want["fpos"], L["row_f"][patch], d64[patch])
    want["tpos"], want["fpos"], want["npe"] = want["tpos"].T, want["fpos"].T, np.stack([want["cls"], want["dist"]])
    slot, cu, toff = (torch.from_numpy(L[k]).to(DEV) for k in ("slot", "cu", "toff"))

    def run(fill, accumulate=False):
        out = dict(cls=torch.full((1, 1, D), fill), dist=torch.full((1, 1, D), fill), npe=torch.full((1, 2, D), fill), bias=torch.full((D,), fill),
                   tpos=torch.full((1, D, 1, Tpe), fill), fpos=torch.full((1, D, Fg, 1), fill))
        out = {k: v.to(DEV) for k, v in out.items()}
        ops.patch_bwd_rows(dtok.to(DEV), slot, cu, toff, Tpe, Fg, out["cls"], out["dist"], out["npe"], out["bias"], out["tpos"], out["fpos"],
                           accumulate=accumulate)
        torch.cuda.synchronize()
        return out
    a, b = run(float("nan")), run(3.0)
    worst = 0.0
    for k, v in a.items():
        assert torch.isfinite(v).all() and torch.equal(v, b[k]), k                 # overwritten; two runs bit-identical
        worst = max(worst, rel_err(v.reshape(want[k].shape), torch.from_numpy(want[k])))
    record(f"patch_bwd_rows[s{stride}]", err=worst)
    print(f"patch_bwd_rows stride {stride}: rel err {worst:.3e}")
    assert worst < tol(PA_F32), worst
    # time positions no clip reaches stay exactly 0
    unused = np.setdiff1d(np.arange(Tpe), tpos_col[patch])
    assert unused.size and float(a["tpos"][0, :, 0, torch.from_numpy(unused)].abs().max()) == 0.0
    c = run(1.0, accumulate=True)
    for k, v in c.items():
        assert rel_err(v.reshape(want[k].shape), torch.from_numpy(want[k] + 1.0)) < tol(PA_F32), k
    # frozen mode: every output NULL is a no-op, a partial set is refused
    lib = _lib.load()
    d = dtok.to(DEV)
    args = (d.data_ptr(), M, D, slot.data_ptr(), cu.data_ptr(), toff.data_ptr(), 3, L["Tg"], Tpe, Fg)
    assert lib.pa_patch_bwd_rows(*args, None, None, None, None, None, None, 0, None) == 0
    assert lib.pa_patch_bwd_rows(*args, a["cls"].data_ptr(), None, None, None, None, None, 0, None) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(v, b[k]) for k, v in a.items())
    with pytest.raises(_lib.PasstAmdError):
        ops.patch_bwd_rows(d, slot, cu, toff[:2], Tpe, Fg, *(a[k] for k in ("cls", "dist", "npe", "bias", "tpos", "fpos")))


# ---- 2. the model against the reference fixture ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(GOLDEN))


def _io(case):
    """x with NaN behind every clip's length, and the loss rows"""
    x, a, b = VT.inputs(case)
    x = torch.from_numpy(x)
    for i, n in enumerate(case["lengths"]):
        x[i, :, :, n:] = float("nan")
    return x.to(DEV), torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)


def _net(case, precision, trainable):
    m = build(case, precision).train().requires_grad_(trainable)
    m.varlen_train = True
    return m


def _packed_step(m, case, x, a, b, **kw):
    xg = x.clone().requires_grad_()
    torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = m(xg, lengths=list(case["lengths"]), **kw)
    VT.loss_of(out[0], out[1], a, b).backward()
    return out, xg.grad


@pytest.mark.parametrize("variant", ["trainable", "frozen"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(VT.CASES))
def test_model_varlen_train_vs_reference(name, precision, variant):
    """Cases (a) - (c), both precisions, parameters trainable and frozen: logits, features and x.grad per clip, the parameter gradients
    summed over the clips, the generator's final state; every figure is printed and recorded before it is asserted."""
    gold, case, trainable = _gold(), VT.CASES[name], variant == "trainable"
    cfg, lengths = case["cfg"], case["lengths"]
    m = _net(case, precision, trainable)
    x, a, b = _io(case)
    (logits, feat), dx = _packed_step(m, case, x, a, b)
    torch.cuda.synchronize()
    assert np.array_equal(torch.get_rng_state().numpy(), gold[f"{name}.rng"])        # the draws of the clip-by-clip loop, no more, no less
    assert logits.grad_fn is not None and dx is not None and dx.shape == x.shape and dx.dtype == torch.float32
    assert torch.isfinite(logits).all() and torch.isfinite(feat).all() and torch.isfinite(dx).all()     # the NaN behind the lengths is never read
    w = dict(logits=0.0, features=0.0, dx=0.0, dx_norm=0.0)
    cu = gold[f"{name}.cu_tok"]
    for i, n in enumerate(lengths):
        key = f"{name}.dx.{i}"
        nrm, scale = (float(v) for v in gold[key + ".stats"])
        got = dx[i:i + 1, :, :, :n].cpu().numpy()
        e = dict(logits=rel(logits[i].detach().cpu(), gold[f"{name}.logits"][i]), features=rel(feat[i].detach().cpu(), gold[f"{name}.features"][i]),
                 dx=float(np.abs(G.pin_sample(got, VT.SAMPLE) - gold[key]).max()) / scale,
                 dx_norm=abs(float(np.linalg.norm(got.astype(np.float64))) - nrm) / nrm)
        print(f"varlen_train.{name}[{precision},{variant}] clip {i} len {n}: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
        for k, v in e.items():
            w[k] = max(w[k], v)
        # exactly 0 behind the clip's length and on the pixels that only dropped patches cover
        rows = slice(int(cu[i]) + 2, int(cu[i + 1]))
        mask = torch.from_numpy(VT.covered(cfg, n, gold[f"{name}.row_f"][rows], gold[f"{name}.row_t"][rows])).to(DEV)
        assert float(dx[i, :, :, n:].abs().max() if n < dx.shape[-1] else 0.0) == 0.0, i
        assert float(dx[i, 0, :, :n][~mask].abs().max() if not bool(mask.all()) else 0.0) == 0.0, i
        assert float(dx[i, 0, :, :n][mask].abs().max()) > 0, i
    params = dict(m.named_parameters())
    if trainable:
        for k in VT.param_grads(cfg):
            key = f"{name}.grad.{k}"
            got = params[k].grad.cpu().numpy()
            w["grad." + k] = float(np.abs(G.pin_sample(got, VT.SAMPLE) - gold[key]).max()) / float(gold[key + ".stats"][1])
        assert all((p.grad is None) == k.startswith("head_dist.") for k, p in params.items())
    else:
        assert all(p.grad is None for p in params.values())
    record(f"varlen_train.{name}[{precision},{variant}]", **w)
    print(f"varlen_train.{name}[{precision},{variant}]", w)
    lim_out, lim_g = (1e-3, 1e-3) if precision == "fp32" else (BF16_LOGITS, BF16_GRADS)
    for k, v in w.items():
        assert v < (lim_out if k in ("logits", "features") else lim_g), (k, v, w)


# ---- 3. against this library's own fixed path at batch size 1 -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VT.CASES))
def test_packed_training_step_is_the_batch_1_loop(name):
    """fp32: the packed call and the loop ``for i: net(x[i:i+1, :, :, :lengths[i]])`` under the same seed -- the same kept patches (the
    generator ends in the same state, the outputs and gradients agree within 1e-3)."""
    case = VT.CASES[name]
    x, a, b = _io(case)
    m = _net(case, "fp32", True)
    (logits, feat), dx = _packed_step(m, case, x, a, b)
    state = torch.get_rng_state()
    s = build(case, "fp32").train()
    s.input_grad = True
    torch.manual_seed(case["torch_seed"])
    w = dict(logits=0.0, features=0.0, dx=0.0, grads=0.0)
    for i, n in enumerate(case["lengths"]):
        xi = x[i:i + 1, :, :, :n].contiguous().requires_grad_()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lo, fe = s(xi)
        VT.loss_of(lo, fe, a[i:i + 1], b[i:i + 1]).backward()
        w["logits"] = max(w["logits"], rel(logits[i].detach().cpu(), lo[0].detach().cpu()))
        w["features"] = max(w["features"], rel(feat[i].detach().cpu(), fe[0].detach().cpu()))
        w["dx"] = max(w["dx"], rel(dx[i:i + 1, :, :, :n].cpu(), xi.grad.cpu()))
        assert torch.equal(dx[i:i + 1, :, :, :n] == 0, xi.grad == 0), i         # the same pixels are covered: the same kept patches
    assert torch.equal(torch.get_rng_state(), state)
    g1 = dict(s.named_parameters())
    for k, p in m.named_parameters():
        if p.grad is not None:
            w["grads"] = max(w["grads"], rel(p.grad.cpu(), g1[k].grad.cpu()))
    record(f"varlen_train.{name}.vs_single[fp32]", **w)
    print(f"varlen_train.{name}.vs_single", w)
    assert all(v < 1e-3 for v in w.values()), w


# ---- 4. token outputs and attention maps ---------------------------------------------------------------------------------------------
def test_hidden_and_attn_have_the_kept_tokens_per_clip():
    gold, case = _gold(), VT.CASES["a"]
    x, a, b = _io(case)
    m = _net(case, "fp32", True)
    (logits, feat, hs, maps, off), dx = _packed_step(m, case, x, a, b, hidden=(0, -1), attn=(0,))
    torch.cuda.synchronize()
    ntok = np.diff(gold["a.cu_tok"]).tolist()
    assert ntok == [7, 55, 115, 295]
    assert off.dtype == torch.int64 and off.tolist() == gold["a.cu_tok"].tolist()
    assert len(hs) == 2 and all(h.shape == (sum(ntok), 768) and h.grad_fn is not None and torch.isfinite(h).all() for h in hs)
    assert len(maps) == 1 and [tuple(t.shape) for t in maps[0]] == [(12, n, n) for n in ntok]
    for t in maps[0]:
        assert t.grad_fn is None and float((t.sum(-1) - 1).abs().max()) < 1e-5
    # the same draws, the same outputs as a call without them (the last block runs on all rows: to rounding)
    (lo2, fe2), dx2 = _packed_step(m, case, x, a, b)
    assert rel(logits.detach().cpu(), lo2.detach().cpu()) < 1e-3 and rel(dx.cpu(), dx2.cpu()) < 1e-3
    assert torch.equal(dx == 0, dx2 == 0)


# ---- 5. the switch ------------------------------------------------------------------------------------------------------------------
def test_switch_and_no_grad():
    case = VT.CASES["c"]
    x, a, b = _io(case)
    lengths = list(case["lengths"])
    m = build(case, "fp32").requires_grad_(False)
    assert m.varlen_train is False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.eval()
        lo0, fe0 = m(x, lengths=lengths)
        m.train()
        state = torch.get_rng_state()
        with pytest.raises(NotImplementedError, match="ragged"):
            m(x, lengths=lengths)
        assert torch.equal(torch.get_rng_state(), state)
        m.varlen_train = True
        m.eval()
        lo1, fe1 = m(x, lengths=lengths)
        assert torch.equal(lo0, lo1) and torch.equal(fe0, fe1) and lo1.grad_fn is None         # eval mode does not see the switch
        assert torch.equal(torch.get_rng_state(), state)
        m.train()
        # no_grad: a plain forward with Patchout, the outputs of the recorded call bit for bit
        (lo2, fe2), dx = _packed_step(m, case, x, a, b)
        torch.manual_seed(case["torch_seed"])
        with torch.no_grad():
            lo3, fe3 = m(x.clone().requires_grad_(), lengths=lengths)
        assert lo3.grad_fn is None and torch.equal(lo2, lo3) and torch.equal(fe2, fe3)
        assert not torch.equal(lo3, lo0)                                                        # Patchout happened
        # nothing requires a gradient: no node
        lo4, _ = m(x, lengths=lengths)
        assert lo4.grad_fn is None
        # a clip that cannot satisfy the counts is named, and nothing is drawn
        state = torch.get_rng_state()
        with pytest.raises(ValueError, match="clip 1:"):
            m(x, lengths=[106, 26])                                                             # 2 patch columns, s_patchout_t = 2
        assert torch.equal(torch.get_rng_state(), state)

"""``net(x, attn=...)`` on the HIP path: the pa_attention_probs kernel against the fp64 softmax of the same rounded inputs, the packed
form against the fixed one, the model against the real reference's fixture (tests/golden/attn.npz: forward hooks on
``blocks[i].attn.attn_drop``), and the invariants of the interface.

Kernel bound: a probability is exp(score - lse), so to first order its relative error is the score's absolute error plus lse's: the
sum of test_gpu_kernels.test_attention_fwd_bwd's two bounds (o, which carries the score error, plus lse), 4e-5 for f32 and 3.5e-2 for
bf16, on the probabilities and on the row sums.  With the fp64 lse handed in only the new kernel's own error is left: tol(dt).  Model
bounds: 1e-3 (fp32) and BF16_LOGITS of tests/test_gpu_model.py, relative to the largest reference entry.  Every measured value is
recorded through test_gpu_kernels.record() / test_gpu_model.record() ("attn_probs" / "attn." names, to be filed as
profiles/attn_parity_metrics.json: no MI355X run had been made when this was written).

Every test fails on the parent commit: the kernel tests on the missing ops, the others with a TypeError on the ``attn=`` keyword."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from passt_amd import ops  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32  # noqa: E402
from tests.golden import make_attn_golden as AG  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_hidden_golden as HG  # noqa: E402
from tests.test_gpu_kernels import TD, _attn_inputs, _attn_ref, rel_err, rnd, tol  # noqa: E402
from tests.test_gpu_kernels import record as record_kernel  # noqa: E402
from tests.test_gpu_model import BF16_LOGITS, DEV, build, rel  # noqa: E402
from tests.test_gpu_model import record as record_model  # noqa: E402

MODES = [(rows, mean) for rows in ("all", "prefix") for mean in (False, True)]


def record(name, **kw):
    (record_model if name.startswith("attn.") else record_kernel)(name, **kw)
    print(name, {k: float(v) for k, v in kw.items()})


def bound(dt):
    """test_attention_fwd_bwd's bound on o plus its bound on lse"""
    return tol(dt, 2e-5, 1.5e-2) + tol(dt, 2e-5, 2e-2)


def _softmax_ref(qref, B, H, N, scale):
    """fp64 (B, H, N, N) probabilities and (B, H, N) lse of the reference-side qkv"""
    t = qref.double().cpu().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (t[0] @ t[1].transpose(-2, -1)) * scale
    return s.softmax(-1), torch.logsumexp(s, -1)


def _variant(p, rows, mean):
    p = p[:, :, :2] if rows == "prefix" else p
    return p.mean(1, keepdim=True) if mean else p


def _check_all_modes(name, dt, x, B, H, N, pre):
    D = H * 64
    qkv, qref = _attn_inputs(x, dt, D, pre)
    ref, rlse = _softmax_ref(qref, B, H, N, 0.125)
    assert torch.allclose(rlse, _attn_ref(qref, B, H, N, 0.125)[1])          # the same reference the forward's tests use
    lse_dev = {"all": ops.attention_fwd(qkv, B, H, N, 0.125, flags=pre)[1], "prefix": ops.attention_fwd(qkv, B, H, N, 0.125, nq=2, flags=pre)[1]}
    lse_ref = {"all": rlse.float().reshape(-1).to(DEV), "prefix": rlse[:, :, :2].float().reshape(-1).to(DEV)}
    lim, lim_own = bound(dt), tol(dt)
    for rows, mean in MODES:
        nq = 2 if rows == "prefix" else N
        want = _variant(ref, rows, mean)
        p = ops.attention_probs(qkv, lse_dev[rows], B, H, N, 0.125, nq=nq, head_mean=mean, flags=pre)
        assert p.shape == (B, 1 if mean else H, nq, N) and p.dtype == torch.float32 and torch.isfinite(p).all()
        e = rel_err(p, want)
        e_sum = float((p.double().sum(-1) - 1).abs().max())
        p_own = ops.attention_probs(qkv, lse_ref[rows], B, H, N, 0.125, nq=nq, head_mean=mean, flags=pre)
        e_own = rel_err(p_own, want)
        record(f"attn_probs[{name},{dt},pre{pre},{rows},{'mean' if mean else 'each'}]", p=e, rowsum=e_sum, p_fp64_lse=e_own)
        assert e < lim and e_sum < lim, (rows, mean, e, e_sum)
        assert e_own < lim_own, (rows, mean, e_own)
        assert torch.equal(p, ops.attention_probs(qkv, lse_dev[rows], B, H, N, 0.125, nq=nq, head_mean=mean, flags=pre))     # bit-repeatable


# a one-tile sequence, exact tile multiples, tails of 1, 3 and 20 keys, multi-tile sequences
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("B,H,N", [(2, 2, 67), (3, 2, 64), (1, 1, 20), (1, 1, 33), (1, 3, 474), (2, 1, 500), (1, 2, 1190)])
def test_attention_probs_vs_fp64_softmax(dt, B, H, N, pre):
    D = H * 64
    x = rnd(B * N, 3 * D, seed=17, scale=1.5)
    if N > 70:                                                   # test_attention_fwd_bwd's spike
        x[N - 3, 0:64] *= 4.0
        x[69, D:D + 64] = x[N - 3, 0:64]
    _check_all_modes(f"{B},{H},{N}", dt, x, B, H, N, pre)


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("case", ["large", "tiny"])
def test_attention_probs_score_ranges(dt, case, pre):
    """test_attention_running_max_paths' uniformly large and uniformly tiny score ranges."""
    B, H, N = 2, 2, 300
    D = H * 64
    x = rnd(B * N, 3 * D, seed=91, scale=1.0)
    x[:, :2 * D] *= 5.0 if case == "large" else 1e-3
    _check_all_modes(case, dt, x, B, H, N, pre)


@pytest.mark.parametrize("N", [33, 67])
def test_attention_probs_strongly_negative_scores_with_keys_past_n(N):
    """test_attention_bwd_strongly_negative_scores_with_keys_past_n's construction (scores ~ -128, lse < -100): a key lane past N
    inside a live tile would see exp2(0 - lse * log2 e) = inf.  Every output is finite, every element of a NaN-filled buffer is
    overwritten, and the guard rows behind it stay as they were."""
    B, H = 2, 2
    D = H * 64
    x = rnd(B * N, 3 * D, seed=77, scale=1.5)
    x[:, D:2 * D] += 4.0
    x[:, :D] -= 4.0
    qkv, _ = _attn_inputs(x, PA_BF16, D, 1)
    for rows, mean in MODES:
        nq = 2 if rows == "prefix" else N
        lse = ops.attention_fwd(qkv, B, H, N, 0.125, nq=nq, flags=1)[1]
        assert float(lse.max()) < -100.0
        n = B * (1 if mean else H) * nq * N
        buf = torch.full((n + 4 * N,), float("nan"), device=DEV)
        p = ops.attention_probs(qkv, lse, B, H, N, 0.125, nq=nq, head_mean=mean, flags=1, out=buf[:n])
        torch.cuda.synchronize()
        assert torch.isfinite(buf[:n]).all() and torch.isnan(buf[n:]).all(), (rows, mean)
        assert float((p.sum(-1) - 1).abs().max()) < bound(PA_BF16)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("nq", [None, 2])
@pytest.mark.parametrize("mean", [False, True])
def test_attention_probs_packed_equals_fixed_per_clip(dt, nq, mean):
    """Packed sequences of 130, 20, 67 and 3 tokens: every clip's map is bit for bit what the fixed entry gives the clip alone at
    B = 1; the whole (NaN-filled) buffer is written and the guard behind it is not."""
    lens, H = [130, 20, 67, 3], 2
    D, B, total = H * 64, len(lens), sum(lens)
    x = rnd(total, 3 * D, seed=23, scale=1.5)
    qkv, _ = _attn_inputs(x, dt, D, 1)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu_dev = torch.from_numpy(cu).to(DEV)
    Ho = 1 if mean else H
    off, n = ops.attention_probs_offsets(lens, Ho, nq)
    lse = ops.attention_fwd_varlen(qkv, cu_dev, B, H, max(lens), 0.125, nq=nq, flags=1)[1]
    buf = torch.full((n + 512,), float("nan"), device=DEV)
    flat = ops.attention_probs_varlen(qkv, lse, cu_dev, torch.from_numpy(off).to(DEV), n, B, H, max(lens), 0.125, nq=nq, head_mean=mean,
                                      flags=1, out=buf[:n])
    torch.cuda.synchronize()
    assert torch.isfinite(buf[:n]).all() and torch.isnan(buf[n:]).all()
    for i, N in enumerate(lens):
        q1 = qkv[cu[i]:cu[i + 1]].contiguous()
        nq1 = N if nq is None else min(nq, N)
        lse1 = ops.attention_fwd(q1, 1, H, N, 0.125, nq=nq1, flags=1)[1]
        alone = ops.attention_probs(q1, lse1, 1, H, N, 0.125, nq=nq1, head_mean=mean, flags=1)
        got = flat[off[i]:off[i] + Ho * nq1 * N].view(1, Ho, nq1, N)
        assert torch.equal(got, alone), (i, N)


# ----------------------------------------------------------------------------------------------
# model against the reference's fixture
# ----------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lim(precision):
    return 1e-3 if precision == "fp32" else BF16_LOGITS


def _map_metrics(gold, key, t, metrics, tag):
    tn = t.detach().cpu().numpy()
    assert t.dtype == torch.float32 and t.grad_fn is None and tuple(tn.shape) == tuple(gold[key + ".shape"]), (key, tn.shape)
    metrics[tag] = rel(G.pin_sample(tn, AG.SAMPLE), gold[key])
    nrm = float(gold[key + ".stats"][0])
    metrics[tag + "_norm"] = abs(float(np.linalg.norm(tn.astype(np.float64))) - nrm) / nrm
    metrics[tag + "_rowsum"] = float(np.abs(tn.astype(np.float64).sum(-1) - 1).max())


@pytest.mark.parametrize("name", list(AG.CASES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_attn_vs_reference_fixture(golden_dir, name, precision):
    gold = dict(np.load(os.path.join(golden_dir, "attn.npz")))
    case = AG.CASES[name]
    m = build(case, precision)
    m.train(case["training"])
    x = _dev(AG.inputs(case))
    depth, lim = case["cfg"]["depth"], _lim(precision)
    for v, (rows, heads) in AG.VARIANTS.items():
        if "torch_seed" in case:
            torch.manual_seed(case["torch_seed"])
        with warnings.catch_warnings(), torch.no_grad():
            warnings.simplefilter("ignore")
            logits, feat, maps = m(x, attn=case["attn"], attn_rows=rows, attn_heads=heads)
        metrics = dict(logits=rel(logits.cpu(), gold[name + ".logits"]), features=rel(feat.cpu(), gold[name + ".features"]))
        assert len(maps) == len(case["attn"])
        for a, t in zip(case["attn"], maps):
            _map_metrics(gold, f"{name}.attn.b{a % depth}.{v}", t, metrics, f"b{a % depth}")
        record(f"attn.{name}[{precision},{v}]", **metrics)
        assert all(e < lim for e in metrics.values()), (v, metrics)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_attn_matches_every_clip_alone(golden_dir, precision):
    """The packed path: clip i's tensor against the reference run on clip i alone at batch size 1."""
    gold = dict(np.load(os.path.join(golden_dir, "attn.npz")))
    case, lengths = AG.RAGGED, AG.RAGGED["lengths"]
    m = build(case, precision).eval()
    x = _dev(AG.ragged_inputs())
    depth, H, lim = case["cfg"]["depth"], case["cfg"]["num_heads"], _lim(precision)
    for v, (rows, heads) in AG.VARIANTS.items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat, maps, tok = m(x, lengths=lengths, attn=case["attn"], attn_rows=rows, attn_heads=heads)
        assert tok.dtype == torch.int64 and tok.device.type == "cpu" and tok.shape == (len(lengths) + 1,)
        ntok = (tok[1:] - tok[:-1]).tolist()
        for i in range(len(lengths)):
            metrics = dict(logits=rel(logits[i:i + 1].cpu(), gold[f"ragged.{i}.logits"]), features=rel(feat[i:i + 1].cpu(), gold[f"ragged.{i}.features"]))
            for a, per_clip in zip(case["attn"], maps):
                assert isinstance(per_clip, list) and len(per_clip) == len(lengths)
                t = per_clip[i]
                nq = 2 if rows == "prefix" else ntok[i]
                assert t.shape == ((nq, ntok[i]) if heads == "mean" else (H, nq, ntok[i]))
                assert t.untyped_storage().data_ptr() == per_clip[0].untyped_storage().data_ptr()      # views of one buffer
                _map_metrics(gold, f"ragged.{i}.attn.b{a % depth}.{v}", t[None], metrics, f"b{a % depth}")
            record(f"attn.ragged.{i}[{precision},{v}]", **metrics)
            assert all(e < lim for e in metrics.values()), (i, v, metrics)


# ----------------------------------------------------------------------------------------------
# invariants, on the HIP path itself
# ----------------------------------------------------------------------------------------------
def _train_step(precision, **kw):
    case = HG.CASES["patchout_train"]
    m = build(case, precision).train()
    m.input_grad = True
    x, a, b = HG.inputs(case)
    xg = _dev(x).requires_grad_()
    torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = m(xg, **kw)
    ((out[0] * _dev(a)).sum() + (out[1] * _dev(b)).sum()).backward()
    return m, out, xg


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kw", [dict(attn=(0,)), dict(attn=(-1,), attn_rows="prefix"), dict(attn=(0, 1), attn_rows="prefix", attn_heads="mean")])
def test_maps_change_nothing_else(precision, kw):
    """A training-mode step (Patchout, same seed, same draws) with maps asked for: logits, features, x.grad and every parameter gradient
    are bit for bit those of the step without ``attn``; the maps carry no grad_fn."""
    m0, out0, x0 = _train_step(precision)
    m1, out1, x1 = _train_step(precision, **kw)
    assert len(out1) == 3 and len(out1[2]) == len(kw["attn"])
    assert all(t.grad_fn is None and not t.requires_grad and t.dtype == torch.float32 for t in out1[2])
    assert out1[0].grad_fn is not None
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1]) and torch.equal(x0.grad, x1.grad)
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        if n.startswith("head_dist."):
            assert p0.grad is None and p1.grad is None
        else:
            assert torch.equal(p0.grad, p1.grad), n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_modes_agree_and_return_order(precision):
    case = HG.CASES["intermediate"]                              # three blocks
    m = build(case, precision).eval()
    x = _dev(HG.inputs(case)[0])
    B, H, N = x.shape[0], case["cfg"]["num_heads"], 290
    with torch.no_grad():
        lo, fe = m(x)
        lo1, fe1, each = m(x, attn=(0, 1, -1))
        assert [tuple(t.shape) for t in each] == [(B, H, N, N)] * 3
        _, _, mean = m(x, attn=[0, 1, 2], attn_heads="mean")
        _, _, pre = m(x, attn=range(3), attn_rows="prefix")
        lo2, fe2, pre_mean = m(x, attn=(2, 0), attn_rows="prefix", attn_heads="mean")
        # the prefix rows of the last block come from the prefix-only tail as it is: nothing else changes
        assert torch.equal(lo, lo2) and torch.equal(fe, fe2)
        assert [tuple(t.shape) for t in pre_mean] == [(B, 2, N)] * 2
        for k in range(3):
            assert mean[k].shape == (B, N, N) and pre[k].shape == (B, H, 2, N)
            assert float((mean[k] - each[k].mean(1)).abs().max()) < 1e-6          # f32 rounding of H probabilities <= 1
            assert float((each[k].sum(-1) - 1).abs().max()) < _lim(precision)
        for k in range(2):                                       # below the last block "prefix" is the same arithmetic on the same lse
            assert torch.equal(pre[k], each[k][:, :, :2])
        assert torch.equal(pre_mean[1], m(x, attn=(0,), attn_rows="prefix", attn_heads="mean")[2][0])
        # all rows of the last block: the full tail, logits / features to rounding (as with hidden=(-1,))
        assert rel(lo1.cpu(), lo.cpu()) < _lim(precision) and rel(fe1.cpu(), fe.cpu()) < _lim(precision)
        # hidden= and attn= in one call: (logits, features, hidden, attn)
        lo3, fe3, hs, maps = m(x, hidden=(1, "norm"), attn=(1,))
        assert len(hs) == 2 and hs[0].shape == (B, N, 128) and len(maps) == 1 and torch.equal(maps[0], each[1])
        assert torch.equal(hs[0], m(x, hidden=(1, "norm"))[2][0])
    # with lengths: (logits, features, hidden, attn, tok_offsets) / (logits, features, attn, tok_offsets)
    rag = build(HG.RAGGED, precision).eval()
    xr = _dev(HG.ragged_inputs()[0])
    out = rag(xr, lengths=HG.RAGGED["lengths"], hidden=(0,), attn=(0,), attn_rows="prefix")
    assert len(out) == 5 and out[2][0].dim() == 2 and isinstance(out[3][0], list) and out[4].dtype == torch.int64
    out2 = rag(xr, lengths=HG.RAGGED["lengths"], attn=(0,), attn_rows="prefix")
    assert len(out2) == 4 and all(torch.equal(u, v) for u, v in zip(out[3][0], out2[2][0]))
    # gradients through the packed node with maps asked for
    rag.varlen_grad = True
    xg = xr.clone().requires_grad_()
    lo_g, fe_g, maps_g, _ = rag(xg, lengths=HG.RAGGED["lengths"], attn=(0,), attn_rows="prefix")
    assert lo_g.grad_fn is not None and all(t.grad_fn is None for t in maps_g[0])
    lo_g.sum().backward()
    assert xg.grad is not None and all(torch.equal(u, v) for u, v in zip(maps_g[0], out2[2][0]))


def test_bad_requests_raise_before_anything_is_drawn():
    case = HG.CASES["patchout_train"]
    m = build(case, "fp32").train()
    x = _dev(HG.inputs(case)[0])
    torch.manual_seed(5)
    state = torch.random.get_rng_state()
    for kw in (dict(attn=0), dict(attn=()), dict(attn="0"), dict(attn=(2,)), dict(attn=(-3,)), dict(attn=(0, -2)), dict(attn=(0, 0)),
               dict(attn=("norm",)), dict(attn=(True,)), dict(attn=(0,), attn_rows="cls"), dict(attn=(0,), attn_heads="sum"),
               dict(attn_rows="none"), dict(attn_heads=None)):
        with pytest.raises(ValueError):
            m(x, **kw)
    assert torch.equal(torch.random.get_rng_state(), state)
    ens = passt_amd.passt.EnsembelerModel([m])
    with pytest.raises(ValueError):
        ens(x, attn=(0,))

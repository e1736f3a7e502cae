"""``net(x, attn=..., attn_grad=...)`` on the HIP path: the pa_attention_probs_grad kernel against fp64 of the same rounded inputs, the
packed form against the fixed one, the model against the real reference's fixture (tests/golden/attn_grad.npz: ``retain_grad()`` in a
forward hook on ``blocks[i].attn.attn_drop``), and the invariants of the interface.

Kernel bounds.  g = d_o v^T is one 64-term product with f32 accumulation: tol(dt) of tests/test_gpu_kernels.py, relative to the largest
entry.  CAM is max(p * g, 0): to first order the error of p * g is p's plus g's, so bound(dt) of tests/test_gpu_attn.py (the
probabilities from the device lse) plus tol(dt); with the fp64 lse handed in p has only the probability kernel's own error tol(dt), so
2 * tol(dt).  CAM with each head is the f32 product of what pa_attention_probs and the GRAD mode write, one rounding: 2^-22 relative.
Model bounds: the project's gradient bounds, 1e-3 (fp32) and BF16_GRADS of tests/test_gpu_model.py, relative to the largest entry of
the reference tensor (a map gradient is a gradient that has passed through the same backward).  Every measured value is recorded
through test_gpu_kernels.record() / test_gpu_model.record() ("attn_probs_grad[...]" / "attn_grad." names, filed as
profiles/attn_grad_parity_metrics.json).

Every test fails on the parent commit: the kernel tests on the missing ops, the others with a TypeError on the ``attn_grad=`` keyword."""
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
from tests.golden import make_attn_grad_golden as GG  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_hidden_golden as HG  # noqa: E402
from tests.test_gpu_attn import _dev, _softmax_ref, _train_step, bound  # noqa: E402
from tests.test_gpu_kernels import TD, _attn_inputs, rel_err, rnd, tol  # noqa: E402
from tests.test_gpu_kernels import record as record_kernel  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, DEV, build  # noqa: E402
from tests.test_gpu_model import record as record_model  # noqa: E402

GRAD, CAM = ops.ATTN_PGRAD_GRAD, ops.ATTN_PGRAD_CAM


def record(name, **kw):
    (record_model if name.startswith("attn_grad.") else record_kernel)(name, **kw)
    print(name, {k: float(v) for k, v in kw.items()})


def _g_ref(qref, d_o, B, H, N):
    """fp64 (B, H, N, N): g[b, h, q, k] = sum_d d_o[b, q, h, d] * v[b, k, h, d]"""
    v = qref.double().cpu().view(B, N, 3, H, 64)[:, :, 2].permute(0, 2, 1, 3)
    do = d_o.double().cpu().view(B, N, H, 64).permute(0, 2, 1, 3)
    return do @ v.transpose(-2, -1)


def _compact(d_o, B, N, nq):
    """the prefix form [(b * nq + q)][D] of a token-row d_o"""
    return d_o.view(B, N, -1)[:, :nq].reshape(B * nq, -1).contiguous()


def _twice(fn):
    """fn() -- checked bit-repeatable"""
    a, b = fn(), fn()
    assert torch.equal(a, b)
    return a


# a one-tile sequence, exact tile multiples, tails of 1, 3 and 20 keys, multi-tile rows
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("B,H,N", [(2, 2, 67), (3, 2, 64), (1, 1, 20), (1, 1, 33), (1, 3, 474), (2, 1, 500)])
def test_attention_probs_grad_vs_fp64(dt, B, H, N, pre):
    D = H * 64
    x = rnd(B * N, 3 * D, seed=17, scale=1.5)
    if N > 70:                                                   # test_attention_fwd_bwd's spike
        x[N - 3, 0:64] *= 4.0
        x[69, D:D + 64] = x[N - 3, 0:64]
    qkv, qref = _attn_inputs(x, dt, D, pre)
    d_o = rnd(B * N, D, seed=29).to(TD[dt]).to(DEV)
    p_ref, rlse = _softmax_ref(qref, B, H, N, 0.125)
    g_ref = _g_ref(qref, d_o, B, H, N)
    cam_ref = (p_ref * g_ref).clamp_min(0)
    name = f"{B},{H},{N},{dt},pre{pre}"

    # ---- GRAD: all rows; the two prefix rows from the token-row d_o and from the compact one
    g_all = _twice(lambda: ops.attention_probs_grad(qkv, None, d_o, B, H, N, 0.125, flags=pre))
    g_tok = _twice(lambda: ops.attention_probs_grad(qkv, None, d_o, B, H, N, 0.125, nq=2, flags=pre))
    g_cmp = _twice(lambda: ops.attention_probs_grad(qkv, None, _compact(d_o, B, N, 2), B, H, N, 0.125, nq=2, do_compact=True, flags=pre))
    assert g_all.shape == (B, H, N, N) and g_tok.shape == (B, H, 2, N) and g_all.dtype == torch.float32
    e = dict(all=rel_err(g_all, g_ref), prefix_rows=rel_err(g_tok, g_ref[:, :, :2]), prefix_compact=rel_err(g_cmp, g_ref[:, :, :2]))
    record(f"attn_probs_grad[{name},grad]", **e)
    assert all(v < tol(dt) for v in e.values()), e
    assert torch.equal(g_tok, g_cmp) and torch.equal(g_tok, g_all[:, :, :2])          # the same tiles of the same products

    # ---- CAM: each head / head mean, all rows / prefix rows (compact d_o), device lse / fp64 lse
    lse_dev = {N: ops.attention_fwd(qkv, B, H, N, 0.125, flags=pre)[1], 2: ops.attention_fwd(qkv, B, H, N, 0.125, nq=2, flags=pre)[1]}
    lse_ref = {N: rlse.float().reshape(-1).to(DEV), 2: rlse[:, :, :2].float().reshape(-1).to(DEV)}
    for nq in (N, 2):
        d_in, compact = (d_o, False) if nq == N else (_compact(d_o, B, N, 2), True)
        for mean in (False, True):
            want = cam_ref[:, :, :nq]
            want = want.mean(1, keepdim=True) if mean else want
            args = dict(nq=nq, head_mean=mean, mode=CAM, do_compact=compact, flags=pre)
            c = _twice(lambda: ops.attention_probs_grad(qkv, lse_dev[nq], d_in, B, H, N, 0.125, **args))
            c_own = ops.attention_probs_grad(qkv, lse_ref[nq], d_in, B, H, N, 0.125, **args)
            assert c.shape == (B, 1 if mean else H, nq, N) and torch.isfinite(c).all() and float(c.min()) >= 0
            e, e_own = rel_err(c, want), rel_err(c_own, want)
            tag = f"attn_probs_grad[{name},cam,{'all' if nq == N else 'prefix'},{'mean' if mean else 'each'}]"
            if not mean:
                p = ops.attention_probs(qkv, lse_dev[nq], B, H, N, 0.125, nq=nq, flags=pre)
                e_prod = rel_err(c, torch.relu(p * (g_all if nq == N else g_cmp)))
                record(tag, cam=e, cam_fp64_lse=e_own, vs_probs_times_grad=e_prod)
                assert e_prod < 2.0 ** -22, e_prod
            else:
                record(tag, cam=e, cam_fp64_lse=e_own)
            assert e < bound(dt) + tol(dt), (nq, mean, e)
            assert e_own < 2 * tol(dt), (nq, mean, e_own)


@pytest.mark.parametrize("N", [33, 67])
def test_attention_probs_grad_strongly_negative_scores_with_keys_past_n(N):
    """test_attention_probs_strongly_negative_scores_with_keys_past_n's construction (scores ~ -128, lse < -100): a key lane past N
    inside a live tile would see exp2(0 - lse * log2 e) = inf, and inf * g or inf * 0 would reach the sum over heads.  In both modes
    every output is finite, every element of a NaN-filled buffer is overwritten, and the guard behind it stays as it was."""
    B, H = 2, 2
    D = H * 64
    x = rnd(B * N, 3 * D, seed=77, scale=1.5)
    x[:, D:2 * D] += 4.0
    x[:, :D] -= 4.0
    qkv, _ = _attn_inputs(x, PA_BF16, D, 1)
    d_o = rnd(B * N, D, seed=31).to(torch.bfloat16).to(DEV)
    for mode, mean in ((GRAD, False), (CAM, False), (CAM, True)):
        for nq in (N, 2):
            lse = ops.attention_fwd(qkv, B, H, N, 0.125, nq=nq, flags=1)[1]
            assert float(lse.max()) < -100.0
            n = B * (1 if mean else H) * nq * N
            for compact in ((False,) if nq == N else (False, True)):
                buf = torch.full((n + 4 * N,), float("nan"), device=DEV)
                ops.attention_probs_grad(qkv, lse if mode == CAM else None, _compact(d_o, B, N, 2) if compact else d_o, B, H, N, 0.125,
                                         nq=nq, head_mean=mean, mode=mode, do_compact=compact, flags=1, out=buf[:n])
                torch.cuda.synchronize()
                assert torch.isfinite(buf[:n]).all() and torch.isnan(buf[n:]).all(), (mode, mean, nq, compact)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("nq", [None, 2])
@pytest.mark.parametrize("mode,mean", [(GRAD, False), (CAM, False), (CAM, True)])
def test_attention_probs_grad_packed_equals_fixed_per_clip(dt, nq, mode, mean):
    """Packed sequences of 130, 20, 67 and 3 tokens: every clip's tensor is bit for bit what the fixed entry gives the clip alone at
    B = 1 (with nq = 2 from the token-row d_o and from the compact one); the whole (NaN-filled) buffer is written and the guard
    behind it is not."""
    lens, H = [130, 20, 67, 3], 2
    D, B, total = H * 64, len(lens), sum(lens)
    x = rnd(total, 3 * D, seed=23, scale=1.5)
    qkv, _ = _attn_inputs(x, dt, D, 1)
    d_tok = rnd(total, D, seed=37).to(TD[dt]).to(DEV)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu_dev = torch.from_numpy(cu).to(DEV)
    Ho = 1 if mean else H
    off, n = ops.attention_probs_offsets(lens, Ho, nq)
    off_dev = torch.from_numpy(off).to(DEV)
    lse = ops.attention_fwd_varlen(qkv, cu_dev, B, H, max(lens), 0.125, nq=nq, flags=1)[1] if mode == CAM else None
    forms = [(d_tok, False)]
    if nq is not None:
        forms.append((torch.cat([d_tok[cu[i]:cu[i] + nq] for i in range(B)]).contiguous(), True))
    for d_o, compact in forms:
        buf = torch.full((n + 512,), float("nan"), device=DEV)
        flat = ops.attention_probs_grad_varlen(qkv, lse, d_o, cu_dev, off_dev, n, B, H, max(lens), 0.125, nq=nq, head_mean=mean, mode=mode,
                                               do_compact=compact, flags=1, out=buf[:n])
        torch.cuda.synchronize()
        assert torch.isfinite(buf[:n]).all() and torch.isnan(buf[n:]).all()
        for i, N in enumerate(lens):
            q1 = qkv[cu[i]:cu[i + 1]].contiguous()
            nq1 = N if nq is None else min(nq, N)
            lse1 = ops.attention_fwd(q1, 1, H, N, 0.125, nq=nq1, flags=1)[1] if mode == CAM else None
            d1 = d_o[i * nq:i * nq + nq1].contiguous() if compact else d_tok[cu[i]:cu[i + 1]].contiguous()
            alone = ops.attention_probs_grad(q1, lse1, d1, 1, H, N, 0.125, nq=nq1, head_mean=mean, mode=mode, do_compact=compact, flags=1)
            got = flat[off[i]:off[i] + Ho * nq1 * N].view(1, Ho, nq1, N)
            assert torch.equal(got, alone), (i, N, compact)


# ----------------------------------------------------------------------------------------------
# model against the reference's fixture
# ----------------------------------------------------------------------------------------------
def _lim(precision):
    return 1e-3 if precision == "fp32" else BF16_GRADS


def _metrics(gold, key, t, metrics, tag):
    """error of the sampled entries and of the L2 norm, both relative to the reference tensor's own scale (largest entry / norm)"""
    tn = t.detach().cpu().numpy()
    assert t.dtype == torch.float32 and tuple(tn.shape) == tuple(gold[key + ".shape"]), (key, tn.shape)
    nrm, amax = (float(v) for v in gold[key + ".stats"])
    metrics[tag] = float(np.abs(G.pin_sample(tn, GG.SAMPLE).astype(np.float64) - gold[key]).max()) / amax
    metrics[tag + "_norm"] = abs(float(np.linalg.norm(tn.astype(np.float64))) - nrm) / nrm


# (attn_grad, the fixture's kind, variant)
RUNS = [("grad", "grad", v) for v in GG.GRAD_VARIANTS] + [("cam", "cam", v) for v in AG.VARIANTS]


@pytest.mark.parametrize("name", list(AG.CASES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_attn_grad_vs_reference_fixture(golden_dir, name, precision):
    gold = dict(np.load(os.path.join(golden_dir, "attn_grad.npz")))
    case = AG.CASES[name]
    m = build(case, precision)
    m.train(case["training"])
    x = _dev(AG.inputs(case))
    a, b = (_dev(w) for w in GG.loss_weights(case))
    depth, lim = case["cfg"]["depth"], _lim(precision)
    for mode, kind, v in RUNS:
        rows, heads = AG.VARIANTS[v]
        if "torch_seed" in case:
            torch.manual_seed(case["torch_seed"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat, maps = m(x, attn=case["attn"], attn_rows=rows, attn_heads=heads, attn_grad=mode)
        assert all(t.grad is None and t.grad_fn is None for t in maps)                     # before the backward
        ((logits * a).sum() + (feat * b).sum()).backward()
        metrics = {}
        for k, t in zip(case["attn"], maps):
            assert t.grad is not None and t.grad.shape == t.shape and t.grad_fn is None
            _metrics(gold, f"{name}.{kind}.b{k % depth}.{v}", t.grad, metrics, f"b{k % depth}")
            if k % depth == depth - 1 and rows == "all":
                # only the cls / dist queries of the last block reach the loss: every other row is exactly zero
                assert float(t.grad[..., 2:, :].abs().max()) == 0.0 and float(t.grad[..., :2, :].abs().max()) > 0.0
        record(f"attn_grad.{name}[{precision},{kind},{v}]", **metrics)
        assert all(e < lim for e in metrics.values()), (mode, v, metrics)
        m.zero_grad()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_attn_grad_matches_every_clip_alone(golden_dir, precision):
    """The packed path: clip i's .grad against the reference run on clip i alone at batch size 1."""
    gold = dict(np.load(os.path.join(golden_dir, "attn_grad.npz")))
    case, lengths = AG.RAGGED, AG.RAGGED["lengths"]
    m = build(case, precision).eval()
    m.varlen_grad = True
    x = _dev(AG.ragged_inputs())
    a, b = (_dev(w) for w in GG.ragged_loss_weights())
    depth, lim = case["cfg"]["depth"], _lim(precision)
    for mode, kind, v in RUNS:
        rows, heads = AG.VARIANTS[v]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat, maps, tok = m(x, lengths=lengths, attn=case["attn"], attn_rows=rows, attn_heads=heads, attn_grad=mode)
        assert all(t.grad is None for per_clip in maps for t in per_clip)
        ((logits * a).sum() + (feat * b).sum()).backward()
        for i in range(len(lengths)):
            metrics = {}
            for k, per_clip in zip(case["attn"], maps):
                t = per_clip[i]
                assert t.grad.shape == t.shape and t.grad.untyped_storage().data_ptr() == per_clip[0].grad.untyped_storage().data_ptr()
                _metrics(gold, f"ragged.{i}.{kind}.b{k % depth}.{v}", t.grad[None], metrics, f"b{k % depth}")
            record(f"attn_grad.ragged.{i}[{precision},{kind},{v}]", **metrics)
            assert all(e < lim for e in metrics.values()), (i, mode, v, metrics)
        m.zero_grad()


# ----------------------------------------------------------------------------------------------
# invariants, on the HIP path itself
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kw,mode", [(dict(attn=(0,)), "grad"), (dict(attn=(-1,), attn_rows="prefix"), "cam"),
                                     (dict(attn=(0, 1), attn_rows="prefix", attn_heads="mean"), "cam"), (dict(attn=(-1, 0)), True)])
def test_map_gradients_change_nothing_else(precision, kw, mode):
    """test_maps_change_nothing_else's training-mode step with ``attn_grad`` set against the same step with ``attn=`` alone: logits,
    features, the maps, x.grad and every parameter gradient are bit for bit the same; the maps still carry no grad_fn."""
    m0, out0, x0 = _train_step(precision, **kw)
    m1, out1, x1 = _train_step(precision, attn_grad=mode, **kw)
    assert len(out1) == 3 and len(out1[2]) == len(kw["attn"])
    assert all(t.grad_fn is None and not t.requires_grad and t.dtype == torch.float32 for t in out1[2])
    assert all(t.grad is None for t in out0[2])
    assert all(t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == torch.float32 and torch.isfinite(t.grad).all() for t in out1[2])
    assert all(torch.equal(u, v) for u, v in zip(out0[2], out1[2]))
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1]) and torch.equal(x0.grad, x1.grad)
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        if n.startswith("head_dist."):
            assert p0.grad is None and p1.grad is None
        else:
            assert torch.equal(p0.grad, p1.grad), n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_cam_is_relu_of_map_times_gradient(precision):
    """Two steps with the same draws: "cam" with each head is relu(map * "grad") to one f32 rounding, and its head mean the mean of it."""
    kw = dict(attn=(0, -1))
    _, out_g, _ = _train_step(precision, attn_grad="grad", **kw)
    _, out_c, _ = _train_step(precision, attn_grad="cam", **kw)
    _, out_m, _ = _train_step(precision, attn_grad="cam", attn_heads="mean", **kw)
    for tg, tc, tm in zip(out_g[2], out_c[2], out_m[2]):
        want = torch.relu(tg * tg.grad)
        assert rel_err(tc.grad, want) < 2.0 ** -22
        assert rel_err(tm.grad, want.double().mean(1)) < 1e-6          # f32 sum of H non-negative terms


def test_bad_requests_raise_before_anything_is_drawn():
    case = HG.CASES["patchout_train"]
    m = build(case, "fp32").train()
    x = _dev(HG.inputs(case)[0])
    torch.manual_seed(5)
    state = torch.random.get_rng_state()
    for kw in (dict(attn=(0,), attn_grad="gradient"), dict(attn=(0,), attn_grad=1), dict(attn_grad="cam"), dict(attn_grad=True),
               dict(attn=(0,), attn_heads="mean", attn_grad="grad"), dict(attn=(0,), attn_heads="mean", attn_grad=True)):
        with pytest.raises(ValueError, match="attn_grad"):
            m(x, **kw)
    with pytest.raises(ValueError, match="come out of a backward"), torch.no_grad():
        m(x, attn=(0,), attn_grad="cam")
    with pytest.raises(ValueError, match="come out of a backward"):
        m.eval()(x, lengths=[250, 100, 64], attn=(0,), attn_grad="cam")            # the ragged forward records nothing unless asked to
    m.train().requires_grad_(False)
    with pytest.raises(ValueError, match="come out of a backward"):
        m(x, attn=(0,), attn_grad="cam")
    assert torch.equal(torch.random.get_rng_state(), state)
    ens = passt_amd.passt.EnsembelerModel([m])
    with pytest.raises(ValueError, match="attn_grad"):
        ens(x, attn=(0,), attn_grad="cam")

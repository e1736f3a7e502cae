"""``net(x, rollout=...)`` on the HIP path: the pa_attention_rollout kernel against fp64 on the head-mean maps the sibling kernels write,
repeatability, the packed form against the fixed one, the model against its own maps and against the real reference's fixture
(tests/golden/rollout.npz), ragged batches, the invariants of the interface and two ranks under passt_amd.ddp.attach.

Kernel bound.  out = a r + b_ sum_{q < nq} r[q] M[q][k] with every term non-negative, so nothing cancels and the bound is elementwise
and relative: the kernel forms the same tiles as pa_attention_probs / pa_attention_probs_grad (head_mean) -- all three take them
from passt_amd/csrc/pa_attn_tile.h, and the one-hot identity test below pins that bit for bit --, whose f32 output M is the
reference's matrix and differs from the registers by the one rounding of (sum over heads) / H; the fused sum over nq products carries
at most nq roundings (fma: the products are exact), the scaling by 1 / H, b_ and the addition of a r a few more:
    |out - ref| <= (nq + 16) * 2^-24 * ref + 1e-37.
Model limits.  (a) fused against the section 1.6 recipe in fp64 on this build's own maps of the same call: depth applications of the
kernel bound, L * (Ntok + 16) * 2^-24 relative to the largest entry (the recipe's renormalisation of rows that already sum to 1 is
inside it).  (b) against the fixture: fp32 within the 1e-3 of tests/test_gpu_attn_grad.py relative to the largest reference entry;
bf16: the fused error may exceed the unfused recipe's own error against the fixture, measured in the same run, by (a)'s limit at
most (triangle inequality).  The prefix-only tail against the full tail (``hidden=(-1,)``, or every row of the last map), both modes
and both precisions: (a)'s limit.  A packed clip against the clip alone at batch 1: (a)'s limit for the clip's own token count -- the
kernels in front of the rollout give a packed clip the bits it gets alone, so what differs is the grouping of the query tiles into
slices, which the kernel bound covers.
Every measured value is recorded through test_gpu_kernels.record() / test_gpu_model.record() ("attn_rollout[...]" / "rollout." names,
filed as profiles/rollout_parity_metrics.json).

Every test but the two one-hot identity tests failed on the commit before ``rollout=``: the kernel tests on the missing ops, the others
with a TypeError on the keyword."""
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from oracle import passt_oracle as O  # noqa: E402
from passt_amd import _lib, ops  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32  # noqa: E402
from tests.golden import make_attn_golden as AG  # noqa: E402
from tests.golden import make_attn_grad_golden as GG  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_rollout_golden as RG  # noqa: E402
from tests.test_gpu_attn import _dev, _train_step  # noqa: E402
from tests.test_gpu_kernels import TD, _attn_inputs, rnd  # noqa: E402
from tests.test_gpu_kernels import record as record_kernel  # noqa: E402
from tests.test_gpu_model import DEV, build  # noqa: E402
from tests.test_gpu_model import record as record_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTN, CAM = ops.ATTN_ROLLOUT_ATTN, ops.ATTN_ROLLOUT_CAM
U = 2.0 ** -24


def record(name, **kw):
    (record_model if name.startswith("rollout.") else record_kernel)(name, **kw)
    print(name, {k: float(v) for k, v in kw.items()})


def _twice(fn):
    """fn() -- checked bit-repeatable"""
    a, b = fn(), fn()
    assert torch.equal(a, b)
    return a


def _compact(d_o, B, N, nq):
    return d_o.view(B, N, -1)[:, :nq].reshape(B * nq, -1).contiguous()


def _slices(total, B, N, nq, nr, slices=0):
    """the slice count S the library runs this call with (1: no workspace)"""
    ws = _lib.load().pa_attention_rollout_ws_floats(total, B, N, nq, nr, slices)
    assert ws >= 0 and ws % (nr * total) == 0
    return max(1, ws // (nr * total))


def _matrix(qkv, lse, d_o, B, H, N, nq, mode, pre, g_scale, compact):
    """M as the sibling kernels write it: f32 (B, nq, N), the head mean of the probabilities / of relu(p * g_scale * g)"""
    if mode == ATTN:
        return ops.attention_probs(qkv, lse, B, H, N, 0.125, nq=nq, head_mean=True, flags=pre)[:, 0]
    return ops.attention_probs_grad(qkv, lse, d_o * g_scale, B, H, N, 0.125, nq=nq, head_mean=True, mode=ops.ATTN_PGRAD_CAM,
                                    do_compact=compact, flags=pre)[:, 0]


def _excess(out, ref, nq):
    """largest |out - ref| in units of the bound (nq + 16) * 2^-24 * ref + 1e-37: <= 1 passes"""
    out, ref = out.double().cpu(), ref.double().cpu()
    return float(((out - ref).abs() / ((nq + 16) * U * ref + 1e-37)).max())


def _check(tag, qkv, d_o, r, B, H, N, nq, mode, pre, slices_list):
    lse = ops.attention_fwd(qkv, B, H, N, 0.125, nq=nq, flags=pre)[1]
    compact = mode == CAM and nq < N
    d_in = None if mode == ATTN else (_compact(d_o, B, N, nq) if compact else d_o)
    worst = {}
    for g_scale in ((1.0,) if mode == ATTN else (1.0, 2.0)):
        M = _matrix(qkv, lse, d_in, B, H, N, nq, mode, pre, g_scale, compact).double().cpu()
        assert float(M.min()) >= 0 and float(M.max()) > 0
        rM = r.double().cpu()[:, :, :nq] @ M
        for a, b in ((0.5, 0.5), (1.0, 1.0)):
            ref = a * r.double().cpu() + b * rM
            for slices in slices_list:
                S = _slices(B * N, B, N, nq, 2, slices)
                out = _twice(lambda: ops.attention_rollout(qkv, lse, r, B, H, N, 0.125, a, b, nq=nq, d_o=d_in, mode=mode, g_scale=g_scale,
                                                           do_compact=compact, flags=pre, slices=slices))
                assert out.shape == (B, 2, N) and out.dtype == torch.float32 and torch.isfinite(out).all()
                worst[f"g{g_scale:g}_a{a:g}_S{S}"] = _excess(out, ref, nq)
    record(tag, **worst)
    assert all(v <= 1.0 for v in worst.values()), worst


# a one-tile sequence, a tail of 1 key and 1 query (33), tails of 3 (67), exact tile multiples, fifteen tiles with three heads
SHAPES = [(1, 1, 20), (1, 1, 33), (2, 2, 67), (3, 2, 64), (1, 3, 474)]


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("mode", [ATTN, CAM], ids=["attn", "cam"])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("prefix", [False, True], ids=["all", "nq2"])
@pytest.mark.parametrize("B,H,N", SHAPES)
def test_attention_rollout_vs_fp64(B, H, N, prefix, dt, mode, pre):
    """nq = N with a query tail (33, 67) catches a clamped row being summed, nq = 2 every row of the one tile but two; a key lane past
    N that leaked would show in columns >= 32 * (N // 32).  The library's own slice count (S > 1 for every multi-tile shape: 15 at
    474 tokens; S = 1 at 20 tokens and for nq = 2) and, where there are tiles to cut, 1 and 4 slices."""
    D = H * 64
    x = rnd(B * N, 3 * D, seed=17, scale=1.5)
    if N > 70:                                                   # test_attention_fwd_bwd's spike
        x[N - 3, 0:64] *= 4.0
        x[69, D:D + 64] = x[N - 3, 0:64]
    qkv, _ = _attn_inputs(x, dt, D, pre)
    d_o = rnd(B * N, D, seed=29).to(TD[dt]).to(DEV)
    r = rnd(B, 2, N, seed=41).abs().to(DEV)
    nq = 2 if prefix else N
    S = _slices(B * N, B, N, nq, 2)
    assert S == (1 if nq <= 32 else min(-(-nq // 32), S)) and (S > 1) == (nq > 32)
    if (B, H, N) == (1, 3, 474) and not prefix:
        assert S == 15
    _check(f"attn_rollout[{B},{H},{N},nq{nq},{dt},{'cam' if mode else 'attn'},pre{pre}]", qkv, d_o, r, B, H, N, nq, mode, pre,
           (0,) if nq <= 64 else (0, 1, 4))


@pytest.mark.parametrize("mode", [ATTN, CAM], ids=["attn", "cam"])
@pytest.mark.parametrize("N", [33, 67])
def test_attention_rollout_strongly_negative_scores_with_keys_past_n(N, mode):
    """tests/test_gpu_attn_grad.py's construction (scores ~ -128, lse < -100): a key lane past N inside a live tile would see
    exp2(0 - lse * log2 e) = inf, and inf * r or inf * 0 would reach the sums.  Every output is finite and within the bound, every
    element of a NaN-filled buffer is overwritten, and the guard behind it stays as it was."""
    B, H = 2, 2
    D = H * 64
    x = rnd(B * N, 3 * D, seed=77, scale=1.5)
    x[:, D:2 * D] += 4.0
    x[:, :D] -= 4.0
    qkv, _ = _attn_inputs(x, PA_BF16, D, 1)
    d_o = rnd(B * N, D, seed=31).to(torch.bfloat16).to(DEV)
    r = rnd(B, 2, N, seed=43).abs().to(DEV)
    worst = {}
    for nq in (N, 2):
        lse = ops.attention_fwd(qkv, B, H, N, 0.125, nq=nq, flags=1)[1]
        assert float(lse.max()) < -100.0
        compact = mode == CAM and nq < N
        d_in = None if mode == ATTN else (_compact(d_o, B, N, 2) if compact else d_o)
        M = _matrix(qkv, lse, d_in, B, H, N, nq, mode, 1, 1.0, compact).double().cpu()
        ref = r.double().cpu() + r.double().cpu()[:, :, :nq] @ M
        n = B * 2 * N
        buf = torch.full((n + 4 * N,), float("nan"), device=DEV)
        ops.attention_rollout(qkv, lse, r, B, H, N, 0.125, 1.0, 1.0, nq=nq, d_o=d_in, mode=mode, do_compact=compact, flags=1,
                              out=buf[:n].view(B, 2, N))
        torch.cuda.synchronize()
        assert torch.isfinite(buf[:n]).all() and torch.isnan(buf[n:]).all(), nq
        worst[f"nq{nq}"] = _excess(buf[:n].view(B, 2, N), ref, nq)
    record(f"attn_rollout[negative,{N},{'cam' if mode else 'attn'}]", **worst)
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("nq", [None, 2], ids=["all", "nq2"])
@pytest.mark.parametrize("mode", [ATTN, CAM], ids=["attn", "cam"])
def test_attention_rollout_packed_equals_fixed_per_clip(dt, nq, mode):
    """Packed sequences of 101, 45 and 5 tokens: every clip's (2, N_b) block is bit for bit what the fixed entry gives the clip alone
    at B = 1 with the same number of query tiles per slice -- one slice (every tile in order), one tile per slice (slices = 4 = the
    longest clip's tiles) and the library's own choice, which at these sizes is one tile per slice on both sides; with nq = 2 from
    the token-row d_o and from the compact one.  The whole (NaN-filled) buffer is written and the guard behind it is not."""
    lens, H = [101, 45, 5], 2
    D, B, total = H * 64, len(lens), sum(lens)
    x = rnd(total, 3 * D, seed=23, scale=1.5)
    qkv, _ = _attn_inputs(x, dt, D, 1)
    d_tok = rnd(total, D, seed=37).to(TD[dt]).to(DEV)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu_dev = torch.from_numpy(cu).to(DEV)
    rs = [rnd(1, 2, n, seed=50 + i).abs().to(DEV) for i, n in enumerate(lens)]
    r = torch.cat([t.reshape(-1) for t in rs]).view(2, total).contiguous()
    lse = ops.attention_fwd_varlen(qkv, cu_dev, B, H, max(lens), 0.125, nq=nq, flags=1)[1]
    forms = [(d_tok, False)] if mode == CAM else [(None, False)]
    if mode == CAM and nq is not None:
        forms.append((torch.cat([d_tok[cu[i]:cu[i] + nq] for i in range(B)]).contiguous(), True))
    for d_o, compact in forms:
        for slices in (1, 4, 0):
            buf = torch.full((2 * total + 512,), float("nan"), device=DEV)
            got = _twice(lambda: ops.attention_rollout_varlen(qkv, lse, r, cu_dev, B, H, max(lens), 0.125, 1.0, 0.5, nq=nq, d_o=d_o, mode=mode,
                                                              g_scale=2.0, do_compact=compact, flags=1, slices=slices,
                                                              out=buf[:2 * total].view(2, total)))
            torch.cuda.synchronize()
            assert torch.isfinite(buf[:2 * total]).all() and torch.isnan(buf[2 * total:]).all()
            for i, (N, view) in enumerate(zip(lens, ops.rollout_views(got, lens))):
                q1 = qkv[cu[i]:cu[i + 1]].contiguous()
                nq1 = N if nq is None else min(nq, N)
                lse1 = ops.attention_fwd(q1, 1, H, N, 0.125, nq=nq1, flags=1)[1]
                d1 = None if d_o is None else (d_o[i * nq:i * nq + nq1].contiguous() if compact else d_tok[cu[i]:cu[i + 1]].contiguous())
                alone = ops.attention_rollout(q1, lse1, rs[i], 1, H, N, 0.125, 1.0, 0.5, nq=nq1, d_o=d1, mode=mode, g_scale=2.0,
                                              do_compact=compact, flags=1, slices=slices)
                assert torch.equal(view, alone[0]), (i, N, compact, slices)


def _one_hot_rows(qs, N):
    r = torch.zeros(len(qs), N)
    r[torch.arange(len(qs)), torch.tensor(qs)] = 1.0
    return r


def _identity_maps(qkv, lse, d_in, B, H, N, nq, mode, pre, compact):
    """the sibling kernel's head-mean map (B, nq, N) for g_scale = 1; for another power of two the map is that multiple, exactly"""
    return _matrix(qkv, lse, d_in, B, H, N, nq, mode, pre, 1.0, compact)


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("mode", [ATTN, CAM], ids=["attn", "cam"])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("prefix", [False, True], ids=["all", "nq2"])
def test_rollout_of_a_one_hot_row_is_a_row_of_the_sibling_map_bit_for_bit(prefix, dt, mode, pre):
    """What sharing passt_amd/csrc/pa_attn_tile.h promises: with a = 0, b = 1 and r_in[b, j] = e_q the rollout returns row q of the
    head-mean map that pa_attention_probs (ATTN) / pa_attention_probs_grad (CAM) writes -- torch.equal, not a bound.  Exact because
    fma(acc, 1, 0) = acc and fma(acc, 0, t) = t for finite acc, the other lane half and every slice without q add 0, and
    fma(1, part / H, 0 * r) is the map kernel's acc * (1 / H); g_scale = 2 doubles every term exactly.  So a single differing
    operation in the tile of either kernel shows as a differing bit.
    B = 2, H = 2, N = 45: two query tiles (the second a 13-row tail), two key waves (the second with 19 dead lanes); the one-hots sit
    in both lane halves (rows 3 / 5), the last row of the full tile (31) and the last live row of the tail (44); 1 and 2 slices.
    nq = 2: rows 0 and 1, CAM from the compact d_o."""
    B, H, N = 2, 2, 45
    D = H * 64
    qkv, _ = _attn_inputs(rnd(B * N, 3 * D, seed=19, scale=1.5), dt, D, pre)
    d_o = rnd(B * N, D, seed=33).to(TD[dt]).to(DEV)
    nq, qs, slices_list = (2, (0, 1), (1,)) if prefix else (N, (3, 5, 31, 44), (1, 2))
    r = _one_hot_rows(qs, N).expand(B, len(qs), N).contiguous().to(DEV)
    lse = ops.attention_fwd(qkv, B, H, N, 0.125, nq=nq, flags=pre)[1]
    compact = mode == CAM and prefix
    d_in = None if mode == ATTN else (_compact(d_o, B, N, nq) if compact else d_o)
    M = _identity_maps(qkv, lse, d_in, B, H, N, nq, mode, pre, compact)
    assert M.shape == (B, nq, N) and float(M.max()) > 0
    for g_scale in ((1.0,) if mode == ATTN else (1.0, 2.0)):
        want = M[:, list(qs), :] * g_scale
        for slices in slices_list:
            assert _slices(B * N, B, N, nq, len(qs), slices) == slices
            out = ops.attention_rollout(qkv, lse, r, B, H, N, 0.125, 0.0, 1.0, nq=nq, d_o=d_in, mode=mode, g_scale=g_scale,
                                        do_compact=compact, flags=pre, slices=slices)
            assert out.shape == want.shape and torch.equal(out, want), (g_scale, slices, float((out - want).abs().max()))


def test_packed_rollout_of_one_hot_rows_is_the_fixed_map_of_every_clip_bit_for_bit():
    """The same identity through the packed entry, clips of 45 and 5 tokens: clip i's block against the map rows the fixed-layout
    sibling kernel gives the clip alone at B = 1 (both types, both modes, all queries, 1 and 2 slices)."""
    lens, H = [45, 5], 2
    D, B, total = H * 64, len(lens), sum(lens)
    qs = [(3, 5, 31, 44), (0, 1, 3, 4)]
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu_dev = torch.from_numpy(cu).to(DEV)
    r = torch.cat([_one_hot_rows(q, n).reshape(-1) for q, n in zip(qs, lens)]).view(4, total).contiguous().to(DEV)
    for dt in (PA_F32, PA_BF16):
        qkv, _ = _attn_inputs(rnd(total, 3 * D, seed=21, scale=1.5), dt, D, 1)
        d_tok = rnd(total, D, seed=35).to(TD[dt]).to(DEV)
        lse = ops.attention_fwd_varlen(qkv, cu_dev, B, H, max(lens), 0.125, flags=1)[1]
        for mode in (ATTN, CAM):
            maps = []
            for i, N in enumerate(lens):
                q1 = qkv[cu[i]:cu[i + 1]].contiguous()
                lse1 = ops.attention_fwd(q1, 1, H, N, 0.125, flags=1)[1]
                d1 = None if mode == ATTN else d_tok[cu[i]:cu[i + 1]].contiguous()
                maps.append(_identity_maps(q1, lse1, d1, 1, H, N, N, mode, 1, False)[0][list(qs[i])])
            for slices in (1, 2):
                got = ops.attention_rollout_varlen(qkv, lse, r, cu_dev, B, H, max(lens), 0.125, 0.0, 1.0, d_o=None if mode == ATTN else d_tok,
                                                   mode=mode, flags=1, slices=slices)
                for i, view in enumerate(ops.rollout_views(got, lens)):
                    assert torch.equal(view, maps[i]), (dt, mode, slices, i)


# ----------------------------------------------------------------------------------------------
# model against its own maps and against the reference's fixture
# ----------------------------------------------------------------------------------------------
def _lim_a(depth, ntok):
    return depth * (ntok + 16) * U


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _call(m, case, x, a, b, mode, **kw):
    """One call (+ the fixture's backward for "cam"): (the returned tuple, the rolled-out rows as a tensor or a list of tensors)"""
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    m.zero_grad()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if mode == "attn":
            with torch.no_grad():
                out = m(x, rollout="attn", **kw)
        else:
            out = m(x, rollout="cam", **kw)
    roll = out[2 + ("attn" in kw)]
    views = roll if isinstance(roll, list) else [roll]
    assert all(v.dtype == torch.float32 and v.grad_fn is None and not v.requires_grad and v.grad is None for v in views)
    if mode == "attn":
        return out, roll
    assert all(float(v.sum()) == v.numel() / v.shape[-1] and float(v[..., 0, 0].min()) == 1.0 and float(v[..., 1, 1].min()) == 1.0
               for v in views)                                   # the one-hot start rows
    ((out[0] * a).sum() + (out[1] * b).sum()).backward()
    assert all(v.grad is not None and v.grad.shape == v.shape and v.grad.dtype == torch.float32 for v in views)
    return out, ([v.grad for v in roll] if isinstance(roll, list) else roll.grad)


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("mode", ["attn", "cam"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(AG.CASES))
def test_rollout_vs_own_maps_and_reference_fixture(golden_dir, name, precision, mode, first):
    gold = dict(np.load(os.path.join(golden_dir, "rollout.npz")))
    case = AG.CASES[name]
    depth = case["cfg"]["depth"]
    m = build(case, precision)
    m.train(case["training"])
    x = _dev(AG.inputs(case))
    a, b = (_dev(w) for w in GG.loss_weights(case))
    # the fused rows and this build's own maps in ONE call (asking for every row of the last block's map makes it a full tail)
    kw = dict(attn=range(depth), attn_heads="mean", rollout_from=first, **(dict(attn_grad="cam") if mode == "cam" else {}))
    out, fused = _call(m, case, x, a, b, mode, **kw)
    maps = [(t.grad if mode == "cam" else t).double().cpu().numpy() for t in out[2]]
    unfused = (RG.recipe_cam if mode == "cam" else RG.recipe_attn)(maps, first)
    fused = fused.double().cpu().numpy()
    ntok = fused.shape[-1]
    assert fused.shape == (case["B"], 2, ntok) == unfused.shape
    lim_a = _lim_a(depth, ntok)
    metrics = dict(vs_own_maps=_rel(fused, unfused), lim_a=lim_a)
    # the same rows from the prefix-only tail (no maps asked for): the last block enters with its two query rows
    _, tail = _call(m, case, x, a, b, mode, rollout_from=first)
    metrics["prefix_tail_vs_full_tail"] = _rel(tail.double().cpu().numpy(), fused)
    key = f"{name}.{mode}.from{first}"
    if key in gold:
        ref = gold[key]
        assert ref.shape == fused.shape
        metrics.update(vs_fixture=_rel(fused, ref), unfused_vs_fixture=_rel(unfused, ref), prefix_tail_vs_fixture=_rel(tail.double().cpu().numpy(), ref))
    else:
        assert first == 1 and name != "three_blocks"
    record(f"rollout.{name}[{precision},{mode},from{first}]", **metrics)
    assert metrics["vs_own_maps"] <= lim_a, metrics
    if key in gold:
        if precision == "fp32":
            assert metrics["vs_fixture"] < 1e-3 and metrics["prefix_tail_vs_fixture"] < 1e-3, metrics
        else:
            assert metrics["vs_fixture"] <= metrics["unfused_vs_fixture"] + lim_a, metrics
    # the two tails agree to rounding: the prefix-only tail computes the same two rows of the last block
    assert metrics["prefix_tail_vs_full_tail"] <= lim_a, metrics


@pytest.mark.parametrize("mode", ["attn", "cam"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_rollout_matches_every_clip_alone(golden_dir, precision, mode):
    """Eval mode ("cam": net.varlen_grad): clip i's rows against the same model on clip i alone at batch size 1, and in fp32 against
    the reference run on clip i alone."""
    gold = dict(np.load(os.path.join(golden_dir, "rollout.npz")))
    case, lengths = AG.RAGGED, AG.RAGGED["lengths"]
    m = build(case, precision).eval()
    m.varlen_grad = True
    x = _dev(AG.ragged_inputs())
    a, b = (_dev(w) for w in GG.ragged_loss_weights())
    out, rolls = _call(m, case, x, a, b, mode, lengths=lengths)
    assert len(out) == 4 and out[3].tolist() == np.concatenate([[0], np.cumsum([r.shape[-1] for r in rolls])]).tolist()
    assert len({r.untyped_storage().data_ptr() for r in rolls}) == 1
    for i, n in enumerate(lengths):
        _, alone = _call(m, case, x[i:i + 1, :, :, :n].contiguous(), a[i:i + 1], b[i:i + 1], mode)
        got, ref = rolls[i].double().cpu().numpy()[None], gold[f"ragged.{i}.{mode}.from0"]
        assert got.shape == ref.shape == tuple(alone.shape)
        lim_a = _lim_a(case["cfg"]["depth"], got.shape[-1])
        metrics = dict(vs_alone=_rel(got, alone.double().cpu().numpy()), vs_fixture=_rel(got, ref), lim_a=lim_a)
        record(f"rollout.ragged.{i}[{precision},{mode}]", **metrics)
        assert metrics["vs_alone"] <= lim_a, (i, metrics)
        if precision == "fp32":
            assert metrics["vs_fixture"] < 1e-3, (i, metrics)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_train_rollout_matches_every_clip_alone(precision):
    """net.varlen_train: Patchout is drawn clip after clip, so after the same seed the packed call and the loop over the clips alone
    keep the same patches, and clip i's "cam" rows are what the clip gets alone at batch size 1 in training mode."""
    case = dict(cfg=O.make_cfg(**dict(G.SMALL, img_size=(128, 998), s_patchout_t=6, s_patchout_f=3)), seed=76, lengths=[998, 437, 250])
    lengths = case["lengths"]
    m = build(case, precision).train()
    m.varlen_train = True
    x = _dev(AG.inputs(dict(case, B=3, T=998)))
    a, b = (_dev(w) for w in GG.loss_weights(case, 3))
    torch.manual_seed(77)
    out, rolls = _call(m, case, x, a, b, "cam", lengths=lengths)
    torch.manual_seed(77)
    for i, n in enumerate(lengths):
        _, alone = _call(m, case, x[i:i + 1, :, :, :n].contiguous(), a[i:i + 1], b[i:i + 1], "cam")
        assert tuple(alone.shape) == (1,) + tuple(rolls[i].shape) and rolls[i].shape[-1] < 2 + 12 * ((n - 16) // 10 + 1)      # Patchout happened
        e = _rel(rolls[i].double().cpu().numpy()[None], alone.double().cpu().numpy())
        lim_a = _lim_a(case["cfg"]["depth"], rolls[i].shape[-1])
        record(f"rollout.ragged_train.{i}[{precision},cam]", vs_alone=e, lim_a=lim_a)
        assert e <= lim_a, (i, e)


# ----------------------------------------------------------------------------------------------
# invariants, on the HIP path itself
# ----------------------------------------------------------------------------------------------
def _same_step(m0, out0, x0, m1, out1, x1, n_same):
    def flat(v):
        return [t for e in v for t in flat(e)] if isinstance(v, (list, tuple)) else [v]

    for s, t in zip(flat(out0[:n_same]), flat(out1[:n_same])):
        assert torch.equal(s, t)
        if s.grad_fn is None:                                        # a map: its gradient, where one was asked for
            assert (s.grad is None) == (t.grad is None) and (s.grad is None or torch.equal(s.grad, t.grad))
    assert torch.equal(x0.grad, x1.grad)
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        if n.startswith("head_dist."):
            assert p0.grad is None and p1.grad is None
        else:
            assert torch.equal(p0.grad, p1.grad), n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("kw", [dict(), dict(attn=(0, -1), attn_rows="prefix", attn_heads="mean", attn_grad="cam"), dict(attn=(0,)),
                                dict(hidden=(-1,))], ids=["plain", "maps_and_cams", "map", "full_tail"])
@pytest.mark.parametrize("mode", ["attn", "cam"])
def test_rollout_changes_nothing_else(precision, kw, mode):
    """tests/test_gpu_attn.py's training-mode step (Patchout, same seed, same draws) with and without ``rollout``: logits, features,
    token outputs, maps and their gradients, x.grad and every parameter gradient are bit for bit the same."""
    m0, out0, x0 = _train_step(precision, **kw)
    m1, out1, x1 = _train_step(precision, rollout=mode, **kw)
    assert len(out1) == len(out0) + 1
    roll = out1[-1]
    assert roll.shape[:2] == (3, 2) and roll.grad_fn is None and not roll.requires_grad and roll.dtype == torch.float32
    rows = roll.grad if mode == "cam" else roll
    assert (roll.grad is None) == (mode == "attn") and torch.isfinite(rows).all() and float(rows.min()) >= 0
    _same_step(m0, out0, x0, m1, out1, x1, len(out0))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["attn", "cam"])
def test_full_tail_agrees_with_the_prefix_only_tail(precision, mode):
    """``hidden=(-1,)`` makes the last block run on all rows, and the rollout then uses all its query rows; without it the last block
    enters with its two prefix rows.  The rows (``roll.grad`` for "cam") agree within (a)'s limit, on the fixed path (training mode,
    Patchout, same draws) and on the ragged one (eval, net.varlen_grad)."""
    depth = AG.CASES["patchout_train"]["cfg"]["depth"]
    _, out_p, _ = _train_step(precision, rollout=mode)
    _, out_f, _ = _train_step(precision, rollout=mode, hidden=(-1,))
    rows = [(out_p[2], out_f[3])]
    case, lengths = AG.RAGGED, AG.RAGGED["lengths"]
    m = build(case, precision).eval()
    m.varlen_grad = True
    x = _dev(AG.ragged_inputs())
    a, b = (_dev(w) for w in GG.ragged_loss_weights())

    def ragged(**kw):
        m.zero_grad()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = m(x, lengths=lengths, rollout=mode, **kw)
        ((out[0] * a).sum() + (out[1] * b).sum()).backward()
        return out[2 + ("hidden" in kw)]

    rows += list(zip(ragged(), ragged(hidden=(-1,))))
    worst = {}
    for i, (p, f) in enumerate(rows):
        p, f = (t.grad if mode == "cam" else t for t in (p, f))
        assert p is not None and f is not None and p.shape == f.shape and float(p.max()) > 0
        lim = _lim_a(depth, p.shape[-1])
        worst["fixed" if i == 0 else f"ragged{i - 1}"] = _rel(f.double().cpu().numpy(), p.double().cpu().numpy()) / lim
    record(f"rollout.full_tail_vs_prefix_tail[{precision},{mode}]", **worst)          # in units of (a)'s limit
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rollout_changes_nothing_else_on_the_ragged_path(precision):
    case, lengths = AG.RAGGED, AG.RAGGED["lengths"]
    x = _dev(AG.ragged_inputs())
    a, b = (_dev(w) for w in GG.ragged_loss_weights())

    def step(**kw):
        m = build(case, precision).eval()
        m.varlen_grad = True
        xg = x.clone().requires_grad_()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = m(xg, lengths=lengths, attn=(-1,), attn_rows="prefix", **kw)
        ((out[0] * a).sum() + (out[1] * b).sum()).backward()
        return m, out, xg

    m0, out0, x0 = step()
    for mode in ("attn", "cam"):
        m1, out1, x1 = step(rollout=mode)
        assert len(out1) == 5 and torch.equal(out0[3], out1[4])
        _same_step(m0, out0, x0, m1, out1, x1, 3)


def test_bad_requests_raise_before_anything_is_drawn():
    case = AG.CASES["patchout_train"]
    m = build(case, "fp32").train()
    x = _dev(AG.inputs(case))
    torch.manual_seed(5)
    state = torch.random.get_rng_state()
    for kw in (dict(rollout="grad"), dict(rollout=True), dict(rollout="attn", rollout_from=2), dict(rollout="cam", rollout_from=0.0),
               dict(rollout_from=1)):
        with pytest.raises(ValueError, match="rollout"):
            m(x, **kw)
    with pytest.raises(ValueError, match="come out of a backward"), torch.no_grad():
        m(x, rollout="cam")
    with pytest.raises(ValueError, match="come out of a backward"):
        m.eval()(x, lengths=[250, 100, 64], rollout="cam")             # the ragged forward records nothing unless asked to
    m.train().requires_grad_(False)
    with pytest.raises(ValueError, match="come out of a backward"):
        m(x, rollout="cam")
    assert torch.equal(torch.random.get_rng_state(), state)
    with pytest.raises(ValueError, match="rollout"):
        passt_amd.passt.EnsembelerModel([m])(x, rollout="attn")


# ----------------------------------------------------------------------------------------------
# two gloo ranks on one GPU
# ----------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, "tests", "ddp_rollout_worker.py")


def _run(out, world):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, WORKER, "--out", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=420)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace")[-2000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return torch.load(out)


def test_attached_reducer_leaves_every_rank_its_own_rows(tmp_path):
    """Two ranks under ddp.attach, half a batch each: the node divides dlogits by 2 and the kernel multiplies the maps' gradients by 2,
    both exact, so ``roll.grad`` of a rank is what a single process gives on that half batch."""
    ref = _run(str(tmp_path / "ref.pt"), 1)
    dp = _run(str(tmp_path / "dp.pt"), 2)
    assert ref["world"] == 1 and dp["world"] == 2
    for r in range(2):
        got, want = dp["rows"][r], ref["rows"][r]
        assert got.shape == want.shape and got.shape[:2] == (4, 2) and float(want.max()) > 1.0
        e = _rel(got.numpy(), want.numpy())
        record(f"rollout.ddp.rank{r}[fp32,cam]", vs_single_process=e, lim_a=_lim_a(ref["depth"], got.shape[-1]))
        assert e <= _lim_a(ref["depth"], got.shape[-1]), (r, e)
        assert torch.equal(got, want), r                            # halving and doubling are exact

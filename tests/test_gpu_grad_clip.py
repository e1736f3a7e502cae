"""Global-norm gradient clipping and gradient accumulation on the GPU: the kernels (pa_grad_accum_sumsq, pa_clip_coef, pa_adamw_clip,
pa_adamw_stage_clip) on guarded buffers, TrainStep(clip_grad_norm=, accumulate=) and passt_amd.optim.AdamW(max_grad_norm=).
References, bounds and buffer builders: tests/grad_clip_cases.py (pinned to torch by tests/test_grad_clip_cpu.py)."""
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
import passt_amd.optim  # noqa: E402
from passt_amd import _lib, ops  # noqa: E402
from passt_amd.train import TrainStep  # noqa: E402
from tests import grad_clip_cases as GC  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.test_gpu_finetune import HYPER, PARAMS, SCALES, SENT, _freeze, _group_case, _group_tables  # noqa: E402
from tests.test_gpu_model import build, rel  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = dict(G.CASES["model_small_train"], seed=901)
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sumsq(values, offset):
    """partials of pa_grad_accum_sumsq over ``values`` placed at element ``offset`` of a NaN-guarded buffer, the partial slots
    guarded too -> (partials on the CPU, [norm, factor(max_norm = 1)] on the CPU)"""
    n, k = values.numel(), GC.n_partials(values.numel())
    buf, span = GC.guarded(values, offset, NAN, DEV)
    pbuf, part = GC.guarded(torch.zeros(k), 1, SENT, DEV)
    ops.grad_accum_sumsq(span, partials=part)
    out = torch.full((2,), SENT, device=DEV)
    ops.clip_coef(part, 1.0, out)
    torch.cuda.synchronize()
    assert GC.guards_intact(pbuf, 1, k, SENT)
    assert torch.equal(_bits(span.cpu()), _bits(values))           # the gradients are read, never written
    return part.cpu(), out.cpu()


# ---- kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4096, 4097, 65537, 1000003])
def test_exact_integer_sums(n, offset):
    assert ops.grad_norm_partials(n) == GC.n_partials(n)
    g = GC.integer_grads(n, 100 + n)
    part, out = _sumsq(g, offset)
    want = GC.ref_partials(g.numpy())
    total = int(want.sum())
    assert total < 2 ** 24
    assert np.array_equal(part.numpy().astype(np.float64), want)                  # every chunk's sum, exactly
    assert float(np.float32(part.double().sum().item())) == float(total)
    assert float(out[0]) == float(np.float32(np.sqrt(np.float64(total))))
    assert GC.is_correctly_rounded_sqrt(out[0].numpy(), total)


@pytest.mark.parametrize("n,scale", [(5, 1e-2), (4097, 1.0), (65537, 1e-3), (1000003, 1e-2)])
def test_random_gradients_norm_bound_and_determinism(n, scale):
    g = GC.random_grads(n, 7 + n, scale)
    runs = [_sumsq(g, off) for off in (0, 0, 0, 1)]
    for part, out in runs[1:]:          # three launches, and the same data one element further: the same bits
        assert torch.equal(_bits(part), _bits(runs[0][0])) and torch.equal(_bits(out), _bits(runs[0][1]))
    part, out = runs[0]
    want = GC.ref_partials(g.numpy())
    e_part = float(np.max(np.abs(part.numpy().astype(np.float64) - want) / want))
    e_norm = abs(float(out[0]) - GC.ref_norm(g.numpy())) / GC.ref_norm(g.numpy())
    print(f"n={n}: worst partial rel err {e_part:.3e} (bound {GC.PARTIAL_BOUND:.3e}), norm rel err {e_norm:.3e} (bound {GC.NORM_BOUND:.3e})")
    assert e_part <= GC.PARTIAL_BOUND and e_norm <= GC.NORM_BOUND


@pytest.mark.parametrize("g_off,a_off", [(0, 0), (1, 1), (3, 3), (1, 0)])
@pytest.mark.parametrize("n", [3, 4097, 70001])
def test_accumulate_kernel(n, g_off, a_off):
    g, a0 = GC.random_grads(n, 31 + n), GC.random_grads(n, 32 + n, 1.0)
    gbuf, gs = GC.guarded(g, g_off, NAN, DEV)
    k = GC.n_partials(n)
    # first: acc is never read (it holds NaN), acc = g exactly
    abuf = torch.full((GC.GUARD + a_off + n + GC.GUARD,), SENT, device=DEV)
    acc = abuf[GC.GUARD + a_off:GC.GUARD + a_off + n]
    acc.fill_(NAN)
    part = torch.full((k,), SENT, device=DEV)
    ops.grad_accum_sumsq(gs, acc, first=True, partials=part)
    assert torch.equal(_bits(acc.cpu()), _bits(g)) and GC.guards_intact(abuf, a_off, n, SENT)
    assert torch.equal(_bits(part.cpu()), _bits(_sumsq(g, 0)[0]))
    # not first: one f32 addition, torch's; the partials are those of the RESULT
    acc.copy_(a0.to(DEV))
    want = a0.to(DEV) + gs
    ops.grad_accum_sumsq(gs, acc, first=False, partials=part)
    assert torch.equal(_bits(acc), _bits(want)) and GC.guards_intact(abuf, a_off, n, SENT)
    assert torch.equal(_bits(part.cpu()), _bits(_sumsq(want.cpu(), 0)[0]))
    assert not torch.equal(_bits(part.cpu()), _bits(_sumsq(g, 0)[0]))
    # without partials: the fold alone
    acc.copy_(a0.to(DEV))
    ops.grad_accum_sumsq(gs, acc, first=False)
    assert torch.equal(_bits(acc), _bits(want)) and GC.guards_intact(abuf, a_off, n, SENT)
    assert torch.equal(_bits(gs.cpu()), _bits(g)) and GC.guards_intact(gbuf, g_off, n, NAN)


def test_accumulate_kernel_needs_an_output():
    g = torch.ones(8, device=DEV)
    with pytest.raises(_lib.PasstAmdError, match=r"code -1"):
        ops.grad_accum_sumsq(g)
    assert _lib.load().pa_grad_accum_sumsq(g.data_ptr(), None, 0, 8, None, None) == -1          # PA_EINVAL


def _coef(values, max_norm):
    part = torch.zeros(GC.n_partials(values.numel()), device=DEV)
    ops.grad_accum_sumsq(values.to(DEV), partials=part)
    out = torch.full((2,), SENT, device=DEV)
    ops.clip_coef(part, max_norm, out)
    return out.cpu().numpy()


def test_clip_coef():
    g = GC.random_grads(5000, 3, 1.0)                   # norm ~ 70
    for max_norm in (1.0, 0.3, 60.0, 7.5e-3):           # above max_norm: the f32 formula, bit for bit
        norm, coef = _coef(g, max_norm)
        assert norm > max_norm and coef < 1.0
        assert coef.tobytes() == GC.ref_coef(norm, max_norm).tobytes()
    for max_norm in (80.0, 1e4, float("inf")):          # below: exactly 1
        norm, coef = _coef(g, max_norm)
        assert norm < max_norm and coef == np.float32(1.0)
    norm, coef = _coef(torch.zeros(4097), 1.0)
    assert norm == 0.0 and coef == np.float32(1.0)
    poisoned = g.clone()
    poisoned[4100] = NAN
    norm, coef = _coef(poisoned, 1.0)
    assert np.isnan(norm) and np.isnan(coef)


def _adamw_launch(dtype, entry, which, hyper_dev, clip, factor):
    """One launch per case of tests/test_gpu_finetune.py's guarded table.  clip=False: today's entry, on g * factor formed by torch in
    f32 (factor None: on g).  clip=True: the *_clip entry with the factor in device memory (None: gscale_dev = NULL)."""
    c = _group_case(dtype)
    g_in = c["g"] if (clip or factor is None) else c["g"] * torch.tensor(factor, dtype=torch.float32)
    dev = dict(p=c["p"].to(DEV), g=g_in.to(DEV), m=c["m"].to(DEV), v=c["v"].to(DEV))
    g_before = dev["g"].clone()
    h = HYPER
    hyper = (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"])
    if hyper_dev:
        host = torch.empty(7, dtype=torch.float32)
        ops.adamw_hyper(*hyper, host)
        hyper = host.to(DEV)
    gs = torch.tensor([factor], dtype=torch.float32, device=DEV) if (clip and factor is not None) else None
    sc = ops.make_adamw_scales(SCALES[which], DEV) if entry in ("stage_groups", "groups") else None
    pgmv = (dev["p"], dev["g"], dev["m"], dev["v"])
    if entry == "flat":
        name = "pa_adamw_clip" if clip else "pa_adamw_dev" if hyper_dev else "pa_adamw"
        for off, (rows, cols, _, _) in zip(c["offs"], PARAMS):          # every parameter as its own flat span (two are misaligned)
            ops.adamw_update(*(t[off:off + rows * cols] for t in pgmv), hyper, gscale=gs, entry=name)
    else:
        ops.adamw_update(*pgmv, hyper, table=_group_tables(c, entry != "groups"), scales=sc, dtype=dtype, gscale=gs,
                         entry="pa_adamw_stage_clip" if clip else "pa_adamw_" + entry)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dev["g"]), _bits(g_before))                # the gradient buffer is not written
    out = {k: dev[k].cpu() for k in "pmv"}
    out["copies"] = c["copies"].cpu()
    out["case"] = c
    return out


@pytest.mark.parametrize("hyper_dev", [False, True])
@pytest.mark.parametrize("entry,which", [("stage", None), ("stage_groups", "a"), ("stage_groups", "b"), ("groups", "a"), ("groups", "b"),
                                         ("flat", None)])
@pytest.mark.parametrize("dtype", [_lib.PA_BF16, _lib.PA_F32])
def test_adamw_clip_kernels(dtype, entry, which, hyper_dev):
    for factor in (None, 1.0, 0.25, 0.3):
        want = _adamw_launch(dtype, entry, which, hyper_dev, False, None if factor == 1.0 else factor)
        got = _adamw_launch(dtype, entry, which, hyper_dev, True, factor)
        live = want["case"]["live"]
        for k in ("p", "m", "v", "copies"):     # parameters, moments, both copies and every sentinel around them
            assert torch.equal(_bits(got[k]), _bits(want[k])), (k, factor)
        for k in "pmv":
            assert bool((got[k][~live] == SENT).all()), k
        assert not torch.equal(got["p"][live], want["case"]["p"][live])
        if factor in (0.25, 0.3):               # ... and the factor did something
            plain = _adamw_launch(dtype, entry, which, hyper_dev, False, None)
            assert not torch.equal(got["m"], plain["m"])


# ---- TrainStep -----------------------------------------------------------------------------------------------------------------------
def _inputs():
    x, y = G.model_inputs(CASE)
    return torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)


def _run_steps(ts, xg, yg, n, seed=50):
    losses = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(n):
            torch.manual_seed(seed + step)
            np.random.seed(seed + step)
            losses.append(ts.step(xg, yg).clone())
    torch.cuda.synchronize()
    return losses


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_step_huge_clip_equals_no_clip(precision):
    xg, yg = _inputs()
    outs = []
    for clip in (None, 1e30):
        ts = TrainStep(build(CASE, precision).train(), None, lr=1e-3, weight_decay=1e-2, use_mixup=False, clip_grad_norm=clip)
        _run_steps(ts, xg, yg, 3)
        outs.append((ts.flat_p.clone(), ts.m.clone(), ts.v.clone()))
        if clip:
            assert float(ts.grad_norm) > 0 and ts.grad_norm.shape == (1,) and float(ts._clip_out[1]) == 1.0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _first_norm(xg, yg, freeze=None):
    net = build(CASE, "fp32").train()
    if freeze:
        _freeze(net, freeze)
    ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=False, clip_grad_norm=1e30)
    _run_steps(ts, xg, yg, 1)
    return float(ts.grad_norm)


@pytest.mark.parametrize("variant", ["plain", "groups", "block1_head"])
def test_train_step_clipping_that_bites_vs_torch(variant):
    """the autograd path + torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW against TrainStep(clip_grad_norm=c), c = half the first
    step's norm; the set-up and the bounds of test_train_step_layer_decay_and_no_weight_decay_vs_torch"""
    from passt_amd import passt as P
    xg, yg = _inputs()
    freeze = variant if variant == "block1_head" else None
    c = 0.5 * _first_norm(xg, yg, freeze)
    m1, m2 = build(CASE, "fp32").train(), build(CASE, "fp32").train()
    if freeze:
        _freeze(m1, freeze), _freeze(m2, freeze)
    depth, lr, wd = len(m1.blocks), 1e-3, 1e-2
    named = [(n, p) for n, p in m1.named_parameters() if not n.startswith("head_dist.") and p.requires_grad]
    kw = {}
    if variant == "groups":
        nwd = {n for n, p in named if p.dim() <= 1} | set(m1.no_weight_decay())
        groups = [dict(params=[p], lr=lr * 0.75 ** (depth - P.param_stage(n, depth)), weight_decay=0.0 if n in nwd else wd) for n, p in named]
        kw = dict(layer_decay=0.75, no_weight_decay="bias_norm")
    else:
        groups = [p for _, p in named]
    opt = torch.optim.AdamW(groups, lr=lr, weight_decay=wd)
    ts = TrainStep(m2, None, lr=lr, weight_decay=wd, use_mixup=False, clip_grad_norm=c, **kw)
    assert [n for n, _ in ts.named] == [n for n, _ in named]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(3):
            torch.manual_seed(50 + step)
            lg, _ = m1(xg)
            loss1 = torch.nn.functional.binary_cross_entropy_with_logits(lg, yg, reduction="none").mean()
            opt.zero_grad()
            loss1.backward()
            norm1 = float(torch.nn.utils.clip_grad_norm_([p for _, p in named], c))
            opt.step()
            torch.manual_seed(50 + step)
            loss2 = ts.step(xg, yg)
            norm2, coef2 = float(ts.grad_norm), float(ts._clip_out[1])
            print(f"{variant} step {step}: norm torch {norm1:.8e} ours {norm2:.8e} rel {abs(norm2 - norm1) / norm1:.3e} factor {coef2:.6f}")
            assert abs(loss1.item() - loss2.item()) < 1e-5, step
            assert abs(norm2 - norm1) <= (GC.NORM_BOUND + 2e-4) * norm1, step
            assert (coef2 < 1.0) == (norm2 > c) and (step > 0 or coef2 < 1.0), step       # it bites on the first step at least
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert rel(p2.detach().cpu(), p1.detach().cpu()) < 2e-4, k
    ts.close()


@pytest.mark.parametrize("groups", [False, True])
def test_train_step_clip_graph_equals_eager(groups):
    xg, yg = _inputs()
    c = 0.5 * _first_norm(xg, yg)
    kw = dict(layer_decay=0.75, no_weight_decay="bias_norm") if groups else {}
    outs = []
    for graph in (False, True):
        ts = TrainStep(build(CASE, "bf16").train(), None, lr=1e-3, weight_decay=1e-2, use_mixup=True, clip_grad_norm=c, graph=graph, **kw)
        ts.graph_warmup = 1
        losses = _run_steps(ts, xg, yg, 4, seed=70)
        assert ts.t == 4 and (not graph or "graph" in ts._g)
        outs.append((torch.cat([l.reshape(1) for l in losses]), ts.flat_p.clone(), ts.m.clone(), ts.v.clone(), ts.grad_norm.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][4]) > 0


@pytest.mark.parametrize("groups", [False, True])
@pytest.mark.parametrize("variant", ["no_fused_stage", "one_launch", "overlap_wgrad"])
def test_train_step_clip_launch_variants_bitwise(variant, groups, monkeypatch):
    """the A/B switches of the step keep working under clipping: the optimizer without the fused staging (PASST_AMD_NO_FUSED_STAGE=1),
    one optimizer launch over the whole buffer (PASST_AMD_BLOCK_OPT=0) -- the same bits as the default step; and with the weight
    gradients (and the bucket reports, hence the partial sums) on the side stream, per-bucket updates against the one launch"""
    xg, yg = _inputs()
    c = 0.5 * _first_norm(xg, yg)
    kw = dict(layer_decay=0.75, no_weight_decay="bias_norm") if groups else {}
    outs = []
    for on in (False, True):
        if on:
            monkeypatch.setenv(*(("PASST_AMD_NO_FUSED_STAGE", "1") if variant == "no_fused_stage" else ("PASST_AMD_BLOCK_OPT", "0")))
        net = build(CASE, "bf16").train()
        net.overlap_wgrad = variant == "overlap_wgrad"
        ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=False, clip_grad_norm=c, **kw)
        assert not on or (not ts.fused_stage if variant == "no_fused_stage" else not ts.block_optimizer)
        _run_steps(ts, xg, yg, 3)
        outs.append((ts.flat_p.clone(), ts.m.clone(), ts.v.clone(), ts.grad_norm.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _micro_batches():
    xg, yg = _inputs()
    return [(xg, yg), (xg.flip(0).contiguous(), yg.flip(0).contiguous())]


def _micro(ts, xy, seed):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(seed)
        np.random.seed(seed)
        return ts.step(*xy)


def _micro_grads(mb):
    """g1, g2: flat_g of two accumulate=1, lr=0, weight_decay=0 steps on the two micro-batches and their seeds"""
    ts = TrainStep(build(CASE, "fp32").train(), None, lr=0.0, weight_decay=0.0, use_mixup=False)
    p0 = ts.flat_p.clone()
    out = []
    for i, xy in enumerate(mb):
        _micro(ts, xy, 60 + i)
        out.append(ts.flat_g.clone())
    assert torch.equal(ts.flat_p, p0)
    return out


def test_train_step_accumulate_two(monkeypatch):
    mb = _micro_batches()
    g1, g2 = _micro_grads(mb)
    lr, wd = 1e-3, 1e-2
    net = build(CASE, "fp32").train()
    ts = TrainStep(net, None, lr=lr, weight_decay=wd, use_mixup=False, accumulate=2)
    before = (ts.flat_p.clone(), ts.m.clone(), ts.v.clone())
    calls, real = [], ops.stage_weights

    def counted(*a, **k):
        calls.append((ts.t, ts._micro))
        return real(*a, **k)
    monkeypatch.setattr(ops, "stage_weights", counted)
    loss1 = _micro(ts, mb[0], 60)
    torch.cuda.synchronize()
    for a, b in zip(before, (ts.flat_p, ts.m, ts.v)):       # micro-step 1: nothing but the two gradient buffers moved
        assert torch.equal(a, b)
    assert ts.t == 0 and ts._micro == 1
    st = net._staged
    copies = {k: out.clone() for k, (ver, out, p) in st.cache.items()}
    assert copies and all(ver == st._version(p) for ver, out, p in st.cache.values())
    assert torch.equal(ts.flat_acc, ts.flat_g)
    loss2 = _micro(ts, mb[1], 61)
    torch.cuda.synchronize()
    assert [c for c in calls if c[1] == 1] == [], calls      # the forward of micro-step 2 restaged nothing
    assert ts.t == 1 and ts._micro == 0
    # the accumulated buffer: 0.5 g1 + 0.5 g2 -- a factor of 1/2 through the backward is exact down to the underflow range
    want = 0.5 * g1 + 0.5 * g2
    big = want.abs() >= 2.0 ** -100
    assert torch.equal(ts.flat_acc[big], want[big]) and float(big.float().mean()) > 0.9
    assert float((ts.flat_acc - want)[~big].abs().max() if bool((~big).any()) else 0.0) <= 2.0 ** -100
    # torch, stepping once on the mean of the two micro-batch losses
    m1 = build(CASE, "fp32").train()
    opt = torch.optim.AdamW([p for n, p in m1.named_parameters() if not n.startswith("head_dist")], lr=lr, weight_decay=wd)
    total = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, (x_, y_) in enumerate(mb):
            torch.manual_seed(60 + i)
            lg, _ = m1(x_)
            li = torch.nn.functional.binary_cross_entropy_with_logits(lg, y_, reduction="none").mean()
            assert abs(li.item() - (loss1, loss2)[i].item()) < 1e-5
            total = total + 0.5 * li
    total.backward()
    opt.step()
    for (k, p1), (_, p2) in zip(m1.named_parameters(), net.named_parameters()):
        assert rel(p2.detach().cpu(), p1.detach().cpu()) < 2e-4, k
    for k, (ver, out, p) in st.cache.items():               # ... and the update rewrote the copies
        w = p.detach().reshape(p.shape[0], -1)
        assert torch.equal(out, (w.t().contiguous() if k[2] else w).to(out.dtype))


@pytest.mark.parametrize("clip", [False, True])
def test_train_step_accumulate_three_flush(clip):
    mb = _micro_batches()
    g1, g2 = _micro_grads(mb)
    lr, wd = 1e-3, 1e-2
    acc_want = g1 / 3.0 + g2 / 3.0
    norm_want = GC.ref_norm(acc_want.cpu().numpy())
    c = 0.5 * norm_want if clip else None
    ts = TrainStep(build(CASE, "fp32").train(), None, lr=lr, weight_decay=wd, use_mixup=False, accumulate=3, clip_grad_norm=c)
    p0 = ts.flat_p.clone()
    ts.flush()                                              # nothing pending: nothing happens
    assert ts.t == 0 and torch.equal(ts.flat_p, p0)
    _micro(ts, mb[0], 60)
    _micro(ts, mb[1], 61)
    assert ts.t == 0 and torch.equal(ts.flat_p, p0)
    ts.flush()
    torch.cuda.synchronize()
    assert ts.t == 1 and ts._micro == 0
    # 1/3 is no power of two: every intermediate of the backward rounds anew; a gradient entry is a sum over at most 2^10 tokens,
    # so the worst case is 2^10 * 2^-24 of the largest entry
    assert rel(ts.flat_acc.cpu(), acc_want.cpu()) < 2.0 ** -14
    coef = 1.0
    if clip:
        norm_acc = GC.ref_norm(ts.flat_acc.cpu().numpy())
        assert abs(float(ts.grad_norm) - norm_acc) <= GC.NORM_BOUND * norm_acc
        coef = GC.ref_coef(ts.grad_norm.cpu().numpy()[0], c)
        assert coef < 1.0 and float(ts._clip_out[1]) == float(coef)
    pw, mw, vw = GC.ref_clipped_adamw(p0.cpu(), ts.flat_acc.cpu(), torch.zeros_like(p0).cpu(), torch.zeros_like(p0).cpu(), coef, lr, 0.9,
                                      0.999, 1e-8, wd, 1)
    assert torch.allclose(ts.flat_p.cpu(), pw, rtol=2e-6, atol=1e-7) and torch.allclose(ts.m.cpu(), mw, rtol=2e-6, atol=1e-7)
    after = (ts.flat_p.clone(), ts.m.clone(), ts.v.clone())
    ts.flush()                                              # a second flush: a no-op
    torch.cuda.synchronize()
    assert ts.t == 1 and all(torch.equal(a, b) for a, b in zip(after, (ts.flat_p, ts.m, ts.v)))


def test_train_step_argument_errors():
    net = build(CASE, "bf16").train()
    with pytest.raises(ValueError):
        TrainStep(net, None, optimizer="sgd", clip_grad_norm=1.0)
    with pytest.raises(NotImplementedError, match="accumulate"):
        TrainStep(net, None, accumulate=2, graph=True)
    for bad in (dict(accumulate=0), dict(clip_grad_norm=0.0), dict(clip_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            TrainStep(net, None, **bad)


# ---- two ranks -----------------------------------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, "tests", "ddp_clip_worker.py")
_DDP = {}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_worker(out, world, extra=()):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, WORKER, "--out", out, *extra], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace")[-2000:])
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    return torch.load(out)


def _ddp_reference(tmp_path_factory):
    """once for both wire types: the clip value (half the first update's norm, from an unclipped single-process run) and the
    single-process run on the concatenated micro-batches"""
    if not _DDP:
        d = tmp_path_factory.mktemp("ddp_clip")
        probe = _run_worker(str(d / "probe.pt"), 1, ("--clip", "1e30", "--updates", "1"))
        _DDP["clip"] = 0.5 * probe["norms"][0][0]
        _DDP["ref"] = _run_worker(str(d / "ref.pt"), 1, ("--clip", repr(_DDP["clip"])))
    return _DDP["clip"], _DDP["ref"]


@pytest.mark.parametrize("wire", ["fp32", "bf16"])
def test_two_ranks_clip_and_accumulate_equal_one_process(tmp_path, tmp_path_factory, wire):
    clip, ref = _ddp_reference(tmp_path_factory)
    dp = _run_worker(str(tmp_path / "dp.pt"), 2, ("--clip", repr(clip), "--comm-dtype", wire))
    assert dp["world"] == 2 and all(same for same, _ in dp["flags"]) and torch.equal(dp["init"], ref["init"])
    for i, full in enumerate(ref["flags"][0][1]):           # mean of the two half-batch losses = the full micro-batch's loss
        halves = [l[i] for _, l in dp["flags"]]
        assert abs(sum(halves) / 2 - full) < (5e-6 if wire == "fp32" else 5e-4), (i, halves, full)
    assert dp["norms"][0] == dp["norms"][1]                 # the same grad_norm on both ranks, update by update
    for a, b in zip(dp["norms"][0], ref["norms"][0]):
        print(f"{wire}: grad_norm two ranks {a:.8e} one process {b:.8e} clip {clip:.8e}")
        assert abs(a - b) <= (1e-4 if wire == "fp32" else 1e-2) * b
    assert dp["norms"][0][0] > clip and ref["norms"][0][0] > clip         # it bites on the first update at least
    nb = dp["buckets"]
    assert nb > 0 and dp["allreduces"] == [0, nb, 0, nb] and ref["allreduces"] == [0, 0, 0, 0]
    d_dp, d_ref = (dp["params"] - dp["init"]).double(), (ref["params"] - ref["init"]).double()
    e = float((d_dp - d_ref).norm() / d_ref.norm())         # AdamW: judged in the L2 norm, as the test this one is modelled on
    print(f"{wire}: update rel l2 {e:.3e}")
    assert float(d_ref.abs().max()) > 0 and e < 2e-2, e


# ---- the drop-in optimizer --------------------------------------------------------------------------------------------------------
def _backward(net, xy, seed):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(seed)
        lg, _ = net(xy[0])
        torch.nn.functional.binary_cross_entropy_with_logits(lg, xy[1], reduction="none").mean().backward()


@pytest.mark.parametrize("backwards", [1, 2])
@pytest.mark.parametrize("flat_grads", [True, False])
def test_optim_adamw_max_grad_norm(flat_grads, backwards, monkeypatch):
    """passt_amd.optim.AdamW(max_grad_norm=c) against a twin stepped by the same optimizer without it on grad * factor, the factor
    formed from opt.grad_norm by the f32 formula and the product written into the twin's .grad by torch: bit-identical parameters and
    moments.  backwards=2: autograd accumulation -- two backwards before one step, the norm is that of the summed gradients."""
    if not flat_grads:
        monkeypatch.setenv("PASST_AMD_NO_FLAT_GRADS", "1")
    mb = _micro_batches()
    net, twin = build(CASE, "fp32").train(), build(CASE, "fp32").train()
    c = None
    for step in range(3):
        if step == 0:                                       # the clip value: half the first step's norm
            probe = build(CASE, "fp32").train()
            for i in range(backwards):
                _backward(probe, mb[i], 80 + i)
            c = 0.5 * float(torch.nn.utils.clip_grad_norm_(probe.parameters(), float("inf")))
            opt = passt_amd.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-2, max_grad_norm=c)
            ref = passt_amd.optim.AdamW(twin.parameters(), lr=1e-3, weight_decay=1e-2)
        opt.zero_grad()
        ref.zero_grad()
        for i in range(backwards):
            _backward(net, mb[i], 80 + 10 * step + i)
            _backward(twin, mb[i], 80 + 10 * step + i)
        grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        opt.step()
        assert bool(flat_grads) == bool(opt._bound) or step == 0
        for n, p in net.named_parameters():                 # p.grad keep the unclipped values
            assert p.grad is None or torch.equal(p.grad, grads[n]), n
        norm_t = float(torch.nn.utils.clip_grad_norm_(twin.parameters(), float("inf")))     # factor 1: the twin's gradients keep their bits
        norm = opt.grad_norm.cpu().numpy()[0]
        print(f"flat={flat_grads} backwards={backwards} step {step}: norm {norm:.8e} torch {norm_t:.8e} rel {abs(norm - norm_t) / norm_t:.3e}")
        assert abs(float(norm) - norm_t) <= GC.NORM_BOUND * norm_t
        coef = GC.ref_coef(norm, c)
        assert coef < 1.0 or step > 0
        for p in twin.parameters():
            if p.grad is not None:
                p.grad.mul_(float(coef))
        ref.step()
        for (n, p), (_, q) in zip(net.named_parameters(), twin.named_parameters()):
            assert torch.equal(p.detach(), q.detach()), (step, n)
            if p in opt.state:
                assert torch.equal(opt.state[p]["exp_avg"], ref.state[q]["exp_avg"]), (step, n)
                assert torch.equal(opt.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"]), (step, n)

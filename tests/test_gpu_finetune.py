"""Partial fine-tuning on the GPU: gradients of a partly frozen network, TrainStep on one, and the AdamW kernels with parameter
groups (pa_adamw_stage_groups / pa_adamw_groups).

Model: tests/golden/make_golden.py's ``model_small_train`` (depth 2, D = 128, 2 heads; stages -1 patch, 0, 1 blocks, 2 norm + head).
Freeze cases: head_only, block1_head, block0_head (block 1 frozen in between), norm_only (every 2-D weight frozen).  Where a whole
stage is frozen the launches that produce the remaining gradients are the all-trainable ones on the same inputs: bit-equal.  Where
the launches change -- block0_head's blocks.0.mlp.fc2.bias (summed by the column-sum kernel, the frozen block above reduces nothing),
and norm_only (reductions behind their producers, not in a finishing launch) -- the gradients meet tests/test_gpu_model.py's bounds
against the reference's golden gradients."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from oracle import passt_oracle as O  # noqa: E402
from passt_amd import _lib, ops  # noqa: E402
from passt_amd import passt as P  # noqa: E402
from passt_amd.train import TrainStep, group_scales  # noqa: E402
from tests.adamw_cases import GUARD, HYPER, PARAMS, SCALES, SENT, group_case  # noqa: E402,F401
from tests.golden import make_golden as G  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, build, rel  # noqa: E402

DEV = "cuda"
CASE = G.CASES["model_small_train"]
FREEZE = {
    "head_only": lambda n, p: n.startswith(("norm.", "head.")),
    "block1_head": lambda n, p: n.startswith(("blocks.1.", "norm.", "head.")),
    "block0_head": lambda n, p: n.startswith(("blocks.0.", "norm.", "head.")),
    "norm_only": lambda n, p: p.dim() <= 1,
}


def _freeze(net, case):
    for n, p in net.named_parameters():
        p.requires_grad_(bool(FREEZE[case](n, p)))
    return net


def _fwd_bwd(net, xg, yg, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(CASE["torch_seed"])
        logits, feat = net(xg, **kw)[:2]
        torch.nn.functional.binary_cross_entropy_with_logits(logits, yg, reduction="none").mean().backward()
    return logits.detach(), feat.detach()


_FULL = {}


def _full(precision):
    """the all-trainable forward + backward of the build under test, once per precision: (logits, features, {name: grad})"""
    if precision not in _FULL:
        x, y = G.model_inputs(CASE)
        net = build(CASE, precision).train()
        lo, fe = _fwd_bwd(net, torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
        _FULL[precision] = (lo, fe, {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
    return _FULL[precision]


@pytest.mark.parametrize("case", list(FREEZE))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradients_of_a_partly_frozen_net(golden_dir, precision, case):
    gold = dict(np.load(os.path.join(golden_dir, "model_small_train.npz")))
    lo0, fe0, g0 = _full(precision)
    x, y = G.model_inputs(CASE)
    net = _freeze(build(CASE, precision).train(), case)
    lo, fe = _fwd_bwd(net, torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
    assert torch.equal(lo, lo0) and torch.equal(fe, fe0)
    lim = 1e-3 if precision == "fp32" else BF16_GRADS
    n_equal = 0
    for n, p in net.named_parameters():
        if not p.requires_grad or n.startswith("head_dist."):
            assert p.grad is None, n
            continue
        got, _ = G.subsample(p.grad.detach().cpu().numpy())
        e = rel(got, gold["grad." + n])
        print(f"{case}[{precision}] {n}: vs golden {e:.3e}, equal to all-trainable: {torch.equal(p.grad, g0[n])}")
        assert e < lim, (n, e)
        if case != "norm_only" and not (case == "block0_head" and n == "blocks.0.mlp.fc2.bias"):
            assert torch.equal(p.grad, g0[n]), n
            n_equal += 1
    assert case == "norm_only" or n_equal >= 6


def test_gradients_of_a_partly_frozen_net_packed():
    """varlen_train (Patchout per clip): block 1 + head trainable, against the all-trainable packed backward of the same build."""
    x, y = G.model_inputs(CASE)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    lengths = [250, 170, 96]
    outs = []
    for case in (None, "block1_head"):
        net = build(CASE, "bf16").train()
        net.varlen_train = True
        if case:
            _freeze(net, case)
        lo, fe = _fwd_bwd(net, xg, yg, lengths=lengths)
        outs.append((lo, fe, net))
    (lo0, fe0, n0), (lo1, fe1, n1) = outs
    assert torch.equal(lo0, lo1) and torch.equal(fe0, fe1)
    for (n, p0), (_, p1) in zip(n0.named_parameters(), n1.named_parameters()):
        if p1.requires_grad and not n.startswith("head_dist."):
            assert torch.equal(p0.grad, p1.grad), n
        else:
            assert p1.grad is None, n


# ---- TrainStep -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["bce", "ce"])
@pytest.mark.parametrize("case", ["block1_head", "head_only"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_step_two_steps_partly_frozen_vs_oracle(precision, case, loss):
    """tests/test_gpu_model.py's two-step test (mixup, Patchout, both losses, fused AdamW; its bounds) on a partly frozen network: the
    oracle's forward / backward with torch.optim.AdamW over the trainable parameters.  Frozen parameters keep their bits."""
    cfg, B = CASE["cfg"], CASE["B"]
    x, y = G.model_inputs(CASE)
    if loss == "ce":
        y = (detgen.uniform(CASE["seed"], "cls", (B,), 0.0, float(cfg["num_classes"])).astype(np.int64) % cfg["num_classes"])
    lr, wd, alpha = 1e-3, 1e-2, 0.3
    sd = O.to_torch(detgen.passt_state_dict(cfg, CASE["seed"]), requires_grad=True)
    for k, v in sd.items():
        v.requires_grad_(bool(FREEZE[case](k, v)) and not k.startswith("head_dist."))
    init = {k: v.detach().clone() for k, v in sd.items()}
    opt = torch.optim.AdamW([v for v in sd.values() if v.requires_grad], lr=lr, weight_decay=wd)
    ref_losses = []
    for step in range(2):
        torch.manual_seed(4000 + step)
        np.random.seed(4000 + step)
        rn, lam = O.my_mixup(B, alpha)
        if loss == "bce":
            xm, ym = O.mixup_apply(torch.from_numpy(x), torch.from_numpy(y), rn, lam)
        else:
            xm, _ = O.mixup_apply(torch.from_numpy(x), torch.zeros(B, 1), rn, lam)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lo, _ = O.passt_forward(sd, xm, cfg, training=True)
        lv = O.bce_loss(lo, ym) if loss == "bce" else O.ce_mixup_loss(lo, torch.from_numpy(y), rn, lam)
        opt.zero_grad()
        lv.backward()
        opt.step()
        ref_losses.append(float(lv.detach()))
    net = _freeze(build(CASE, precision).train(), case)
    ts = TrainStep(net, None, lr=lr, weight_decay=wd, mixup_alpha=alpha, use_mixup=True, loss=loss)
    assert {n for n, _ in ts.named} == {k for k, v in sd.items() if v.requires_grad}
    assert ts.flat_p.numel() == ts.m.numel() == sum(v.numel() for v in sd.values() if v.requires_grad)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    losses = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(2):
            torch.manual_seed(4000 + step)
            np.random.seed(4000 + step)
            losses.append(float(ts.step(xg, yg).item()))
    ltol = 2e-5 if precision == "fp32" else 3e-3
    print(f"{case}[{precision},{loss}] losses {losses} reference {ref_losses}")
    assert all(abs(a - b) < ltol for a, b in zip(losses, ref_losses)), (losses, ref_losses)
    trainable = dict(ts.named)
    for name, p in net.named_parameters():
        if name not in trainable:
            assert torch.equal(p.detach().cpu(), init[name]), name            # frozen: never written
            assert p.grad is None, name
            continue
        d = (p.detach().double().cpu() - init[name].double()).reshape(-1)
        dr = (sd[name].detach().double() - init[name].double()).reshape(-1)
        if name.endswith("attn.qkv.bias"):              # the K third's true gradient is 0 (tests/test_gpu_model.py)
            third = d.numel() // 3
            keep = torch.cat([torch.arange(0, third), torch.arange(2 * third, 3 * third)])
            d, dr = d[keep], dr[keep]
        if float(dr.norm()) == 0.0:
            continue
        cos = float((d @ dr) / (d.norm() * dr.norm() + 1e-300))
        l2 = float((d - dr).norm() / dr.norm())
        print(f"  {name}: cosine {cos:.6f} rel l2 {l2:.3e}")
        assert cos > (0.999 if precision == "fp32" else 0.9), (name, cos)
        if precision == "fp32":
            assert l2 < 3e-2, (name, l2)
    ts.close()


def _steps(ts, xg, yg, n):
    losses = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(n):
            torch.manual_seed(70 + step)
            np.random.seed(70 + step)
            losses.append(ts.step(xg, yg).clone())
    torch.cuda.synchronize()
    return torch.cat([l.reshape(1) for l in losses]).cpu()


@pytest.mark.parametrize("case", ["block1_head", "head_only"])
def test_train_step_partly_frozen_graph_equals_eager(case):
    x, y = G.model_inputs(CASE)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    outs = []
    for graph in (False, True):
        net = _freeze(build(CASE, "bf16").train(), case)
        ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=True, graph=graph)
        losses = _steps(ts, xg, yg, 5)
        assert ts.t == 5 and (not graph or "graph" in ts._g)
        outs.append((losses, ts.flat_p.clone(), ts.m.clone(), ts.v.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["block1_head", "head_only"])
def test_train_step_partly_frozen_never_restages(case, monkeypatch):
    """A steady-state step holds no pa_stage_weights launch: the optimizer rewrites the copies of what it updates, and the copies of
    the frozen weights stay current."""
    x, y = G.model_inputs(CASE)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    net = _freeze(build(CASE, "bf16").train(), case)
    init = {n: p.detach().clone() for n, p in net.named_parameters()}
    ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=False)
    calls, real = [], ops.stage_weights

    def counted(*a, **k):
        calls.append(ts.t)
        return real(*a, **k)
    monkeypatch.setattr(ops, "stage_weights", counted)
    _steps(ts, xg, yg, 4)
    assert [t for t in calls if t >= 1] == [], calls             # ts.t counts finished steps: none from the second step on
    st = net._staged
    assert st.cache and all(ver == st._version(p) for ver, out, p in st.cache.values())
    for (pid, dt, transposed), (ver, out, p) in st.cache.items():
        w = p.detach().reshape(p.shape[0], -1)
        assert torch.equal(out, (w.t().contiguous() if transposed else w).to(out.dtype))
    moved = {n for n, p in net.named_parameters() if not torch.equal(p.detach(), init[n])}
    assert moved == {n for n, _ in ts.named}


def test_head_only_forward_keeps_less():
    x, _ = G.model_inputs(CASE)
    xg = torch.from_numpy(x).to(DEV)
    used = {}
    for case in ("all", "head_only"):
        net = build(CASE, "bf16").train()
        if case != "all":
            _freeze(net, case)
        plan = P.trainable_plan(net)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            torch.manual_seed(3)
            P.passt_forward(net, xg, save=plan)                         # warm: staged weight copies, cached index tensors
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.manual_seed(3)
            out = P.passt_forward(net, xg, save=plan)
            torch.cuda.synchronize()
        used[case] = torch.cuda.memory_allocated() - base
        assert [s is None for s in out[2]["saved"]] == [case == "head_only"] * 2
        del out
    print("bytes held by a forward:", used)
    assert 0 < used["head_only"] < used["all"], used


def test_train_step_sgd_drop_path_and_errors():
    x, y = G.model_inputs(CASE)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    net = build(CASE, "bf16").train().requires_grad_(False)
    with pytest.raises(ValueError):
        TrainStep(net, None)
    net = _freeze(build(CASE, "bf16").train(), "head_only")
    with pytest.raises(ValueError):
        TrainStep(net, None, optimizer="sgd", layer_decay=0.75)
    init = {n: p.detach().clone() for n, p in net.named_parameters()}
    ts = TrainStep(net, None, lr=1e-2, optimizer="sgd", use_mixup=False)
    _steps(ts, xg, yg, 2)
    assert {n for n, p in net.named_parameters() if not torch.equal(p.detach(), init[n])} == {n for n, _ in ts.named}
    # stochastic depth through a partly frozen step: the frozen block draws its masks like the trainable one
    cfg = CASE["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"], s_patchout_f=cfg["s_patchout_f"],
                              img_size=cfg["img_size"], stride=cfg["stride"], num_classes=cfg["num_classes"], embed_dim=cfg["embed_dim"],
                              depth=cfg["depth"], num_heads=cfg["num_heads"], distilled=True, drop_path_rate=0.2)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in detgen.passt_state_dict(cfg, CASE["seed"]).items()})
    net.precision = "bf16"
    net = _freeze(net.to(DEV).train(), "block1_head")
    init = {n: p.detach().clone() for n, p in net.named_parameters()}
    ts = TrainStep(net, None, lr=1e-3, use_mixup=True)
    losses = _steps(ts, xg, yg, 2)
    assert torch.isfinite(losses).all()
    assert {n for n, p in net.named_parameters() if not torch.equal(p.detach(), init[n])} == {n for n, _ in ts.named}


# ---- parameter groups --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_train_step_layer_decay_and_no_weight_decay_vs_torch(graph):
    """TrainStep(layer_decay=0.75, no_weight_decay="bias_norm") against the autograd path + torch.optim.AdamW with the equivalent
    param_groups (exact-f32 kernels, the bound of test_train_step_driver_matches_autograd_path); graph mode captures after one eager
    step and must then equal the eager run bit for bit."""
    case = dict(CASE, seed=901)
    m1 = build(case, "fp32").train()
    x, y = G.model_inputs(case)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    depth, lr, wd = len(m1.blocks), 1e-3, 1e-2
    named = [(n, p) for n, p in m1.named_parameters() if not n.startswith("head_dist.")]
    nwd = {n for n, p in named if p.dim() <= 1} | set(m1.no_weight_decay())
    groups = [dict(params=[p], lr=lr * 0.75 ** (depth - P.param_stage(n, depth)), weight_decay=0.0 if n in nwd else wd) for n, p in named]
    opt = torch.optim.AdamW(groups, lr=lr, weight_decay=wd)
    runs = []
    for g in ((False, True) if graph else (False,)):
        m2 = build(case, "fp32").train()
        ts = TrainStep(m2, None, lr=lr, weight_decay=wd, use_mixup=False, layer_decay=0.75, no_weight_decay="bias_norm", graph=g)
        ts.graph_warmup = 1
        assert ts.groups == group_scales([(n, p.dim()) for n, p in named], depth, 0.75, "bias_norm", m1.no_weight_decay())
        runs.append((m2, ts))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(3):
            torch.manual_seed(50 + step)
            lg, _ = m1(xg)
            loss1 = torch.nn.functional.binary_cross_entropy_with_logits(lg, yg, reduction="none").mean()
            opt.zero_grad()
            loss1.backward()
            opt.step()
            for m2, ts in runs:
                torch.manual_seed(50 + step)
                loss2 = ts.step(xg, yg)
                assert abs(loss1.item() - loss2.item()) < 1e-5, step
    for m2, ts in runs:
        assert not ts.graph or "graph" in ts._g
        for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
            assert rel(p2.detach().cpu(), p1.detach().cpu()) < 2e-4, k
    if graph:
        (_, e), (_, g) = runs
        assert torch.equal(e.flat_p, g.flat_p) and torch.equal(e.m, g.m) and torch.equal(e.v, g.v)


def _group_case(dtype):
    """flat p / g / m / v with sentinel guards around every parameter, guarded copies (tests/adamw_cases.py)"""
    return group_case(dtype, DEV)


def _group_tables(c, with_copies):
    entries = [(off, rows, cols, c["dst"] if (cp and with_copies) else None, c["dst_t"] if (cp and with_copies) else None)
               for off, (rows, cols, cp, _) in zip(c["offs"], PARAMS)]
    if not with_copies:
        entries = [(off, 1, rows * cols, None, None) for off, rows, cols, _, _ in entries]
    return ops.make_adamw_stage_table(entries, DEV)


def _run_groups(dtype, entry, scales, hyper_dev=False):
    """one launch of ``entry`` ("stage" = pa_adamw_stage, "stage_groups", "groups") on a fresh guarded case -> CPU results"""
    c = _group_case(dtype)
    dev = {k: c[k].to(DEV) for k in "pgmv"}
    tab, n, items = _group_tables(c, entry != "groups")
    h = HYPER
    hyper = (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"])
    if hyper_dev:
        host = torch.empty(7, dtype=torch.float32)
        ops.adamw_hyper(*hyper, host)
        hyper = host.to(DEV)
    sc = None if entry == "stage" else ops.make_adamw_scales(scales, DEV)
    ops.adamw_update(dev["p"], dev["g"], dev["m"], dev["v"], hyper, table=(tab, n, items), scales=sc, dtype=dtype, entry="pa_adamw_" + entry)
    torch.cuda.synchronize()
    out = {k: dev[k].cpu() for k in "pmv"}
    out["copies"] = c["copies"].cpu()
    out["case"] = c
    return out


def _check_groups(out, scales, dtype, copies):
    c, h = out["case"], HYPER
    live = c["live"]
    for k in "pmv":                          # nothing outside a parameter was written
        assert torch.equal(out[k][~live], c[k][~live]), k
    rows, cols = PARAMS[0][:2]
    cp = out["copies"]
    assert bool((cp[:, :GUARD] == SENT).all()) and bool((cp[:, GUARD + rows * cols:] == SENT).all())
    for off, (r, cl, _, _), (ls, ws) in zip(c["offs"], PARAMS, scales):
        sl = slice(off, off + r * cl)
        p0, g0, m0, v0 = (c[k][sl].double() for k in "pgmv")
        lr, wd = h["lr"] * ls, h["wd"] * ws
        m1 = h["b1"] * m0 + (1 - h["b1"]) * g0
        v1 = h["b2"] * v0 + (1 - h["b2"]) * g0 * g0
        p1 = p0 * (1 - lr * wd) - lr / (1 - h["b1"] ** h["step"]) * m1 / (v1.sqrt() / (1 - h["b2"] ** h["step"]) ** 0.5 + h["eps"])
        assert float((out["p"][sl].double() - p1).abs().max()) < 2e-6, (off, ls, ws)
        assert rel(out["m"][sl], m1) < 1e-6 and rel(out["v"][sl], v1) < 1e-6
        if ls == 0.0:
            assert torch.equal(out["p"][sl], c["p"][sl])          # lr_scale 0: the parameter keeps its bits
        else:
            assert not torch.equal(out["p"][sl], c["p"][sl])
    td = ops.TORCH_DTYPE[dtype]
    w = out["p"][c["offs"][0]:c["offs"][0] + rows * cols].view(rows, cols)
    body = cp[:, GUARD:GUARD + rows * cols]
    if copies:
        assert torch.equal(body[0].view(rows, cols), w.to(td)) and torch.equal(body[1].view(cols, rows), w.t().contiguous().to(td))
    else:
        assert bool((body == SENT).all())


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("entry", ["stage_groups", "groups"])
@pytest.mark.parametrize("dtype", [_lib.PA_BF16, _lib.PA_F32])
def test_adamw_groups_kernels(dtype, entry, which):
    scales = SCALES[which]
    out = _run_groups(dtype, entry, scales)
    _check_groups(out, scales, dtype, entry == "stage_groups")
    dev = _run_groups(dtype, entry, scales, hyper_dev=True)         # the step's scalars from device memory: the same bits
    for k in ("p", "m", "v", "copies"):
        assert torch.equal(out[k], dev[k]), k


@pytest.mark.parametrize("dtype", [_lib.PA_BF16, _lib.PA_F32])
def test_adamw_groups_of_ones_equal_the_plain_launches(dtype):
    base = _run_groups(dtype, "stage", None)
    ones = _run_groups(dtype, "stage_groups", SCALES["ones"])
    plain = _run_groups(dtype, "groups", SCALES["ones"])
    for k in ("p", "m", "v"):
        assert torch.equal(base[k], ones[k]) and torch.equal(base[k], plain[k]), k
    assert torch.equal(base["copies"], ones["copies"])
    _check_groups(ones, SCALES["ones"], dtype, True)

"""Stochastic depth (drop_path_rate > 0) on the HIP path: the residual epilogues and the LayerNorm backward with row factors against
fp64 torch, the model against the real reference's fixture (tests/golden/drop_path.npz, masks fed through ``drop_path_masks``), and
the invariants of the interface (eval, device draws, captured graph).

Bounds: 1e-4 for the residual GEMM (tests.test_gpu_kernels.test_gemm_split_k_store_and_resid's bound for the same f32 sums of
bf16 products), tests.test_gpu_kernels.tol for the LayerNorm copy and column sums, 1e-3 (fp32) and BF16_LOGITS / BF16_GRADS of
tests/test_gpu_model.py for the model.  Every measured value is printed and recorded before it is asserted.

Every test fails on the parent commit: at construction (drop_path_rate raises there) or at the missing ``rowscale`` arguments."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from passt_amd import _lib, ops  # noqa: E402
from passt_amd import passt as P  # noqa: E402
from passt_amd._lib import EPI_RESID, PA_BF16, PA_F32  # noqa: E402
from tests.golden import make_drop_path_golden as DG  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_hidden_golden as HG  # noqa: E402
from tests.test_gpu_kernels import TD, rel_err, rnd, tol  # noqa: E402
from tests.test_gpu_kernels import record as record_kernel  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, BF16_LOGITS, DEV, rel  # noqa: E402
from tests.test_gpu_model import record as record_model  # noqa: E402


def record(name, **kw):
    (record_model if name.startswith("drop_path.model") else record_kernel)(name, **kw)
    print(name, {k: float(v) for k, v in kw.items()})


def _factors(M, run=7):
    """factors from {1 / 0.9, 0, 2, 1} in runs of ``run`` rows: a tile of any height holds several"""
    vals = torch.tensor([1.0 / 0.9, 0.0, 2.0, 1.0])
    return vals[(torch.arange(M) // run) % 4].contiguous()


# ----------------------------------------------------------------------------------------------
# residual epilogue with a row factor
# ----------------------------------------------------------------------------------------------
RESID_SHAPES = [(1000, 768, 768, PA_BF16), (333, 768, 3072, PA_BF16), (24, 768, 3072, PA_BF16), (77, 192, 128, PA_BF16),
                (200, 768, 768, PA_F32)]


@pytest.mark.parametrize("M,N,K,dt", RESID_SHAPES)
def test_resid_rowscale(M, N, K, dt):
    """out = resid + rowscale[m] * (A B^T + bias) against fp64 on the shapes of the issue (role-split with edge tiles, split-K, the
    small generic kernel, f32), as the library picks the kernel and -- bf16 -- under every forced role-split / generic variant with
    both epilogues, so that every instantiation with a factor runs.  On the same launches: factor-0 rows are resid bit for bit, all
    ones is the unscaled call bit for bit, in place equals out of place; at (1000, 768, 768) the LDS-free epilogue and the
    one-item-per-workgroup launch equal the default bit for bit."""
    A = rnd(M, K, seed=51).to(TD[dt]).to(DEV)
    W = rnd(N, K, seed=52).to(TD[dt]).to(DEV)
    bias, resid = rnd(N, seed=53).to(DEV), rnd(M, N, seed=54, scale=2.0).to(DEV)
    rs = _factors(M)
    want = resid.double().cpu() + rs.double()[:, None] * (A.double().cpu() @ W.double().cpu().T + bias.double().cpu())
    rs = rs.to(DEV)
    if (M, K) == (24, 3072):
        assert _lib.load().pa_gemm_nt_splitk_plan(M, N, K, EPI_RESID, dt) > 1          # the finishing pass is what runs here

    def run(rowscale, out=None, **kw):
        out = torch.full((M, N), float("nan"), device=DEV) if out is None else out
        ops.gemm_nt(A, W, dt, EPI_RESID, bias=bias, resid=resid, out_f32=out, rowscale=rowscale, **kw)
        return out

    variants = [dict()] + ([dict(tune=t, flags=f) for t in (1, 6, 7, 17, 8, 18) for f in (0, _lib.GEMM_EPILOGUE_V3)
                            if not (f and t in (1, 6))] if dt == PA_BF16 else [])
    zero = (rs == 0).nonzero().flatten()
    errs, outs = {}, {}
    for kw in variants:
        out = run(rs, **kw)
        tag = "default" if not kw else f"tune{kw['tune']}{'_v3' if kw['flags'] else ''}"
        errs[tag], outs[tag] = rel_err(out, want), out
        assert torch.equal(out[zero], resid[zero]), tag                                 # a dropped row IS the residual stream
        ones = run(torch.ones(M, device=DEV), **kw)
        plain = torch.empty(M, N, device=DEV)
        ops.gemm_nt(A, W, dt, EPI_RESID, bias=bias, resid=resid, out_f32=plain, **kw)
        assert torch.equal(ones, plain), tag
    record(f"drop_path.resid[{dt},{M},{N},{K}]", **errs)
    assert max(errs.values()) < 1e-4, errs
    for tag in outs:                                  # the LDS-free epilogue: the bits of the default one, tile by tile
        if tag.endswith("_v3"):
            assert torch.equal(outs[tag], outs[tag[:-3]]), tag
    base = run(rs)
    if (M, N, K) == (1000, 768, 768):
        for fl in (_lib.GEMM_EPILOGUE_V3, _lib.GEMM_NO_PERSIST):
            assert torch.equal(run(rs, flags=fl), base), fl
    # the public wrapper, and in place on the residual stream
    assert torch.equal(ops.linear_resid(A, W, bias, resid, dt, rowscale=rs), base)
    stream = resid.clone()
    ops.linear_resid(A, W, bias, stream, dt, out=stream, rowscale=rs)
    assert torch.equal(stream, base)


def test_resid_rowscale_argument_checks():
    A, W = rnd(64, 128, seed=1).bfloat16().to(DEV), rnd(64, 128, seed=2).bfloat16().to(DEV)
    resid = rnd(64, 64, seed=3).to(DEV)
    out = torch.empty_like(resid)
    for bad in (torch.ones(63, device=DEV), torch.ones(64, device=DEV, dtype=torch.bfloat16), torch.ones(128, device=DEV)[::2]):
        with pytest.raises(_lib.PasstAmdError):
            ops.gemm_nt(A, W, PA_BF16, EPI_RESID, resid=resid, out_f32=out, rowscale=bad)
    with pytest.raises(_lib.PasstAmdError):
        ops.gemm_nt(A, W, PA_BF16, ops.EPI_STORE, out_lp=torch.empty(64, 64, device=DEV, dtype=torch.bfloat16), rowscale=torch.ones(64, device=DEV))


# ----------------------------------------------------------------------------------------------
# LayerNorm backward with a scaled copy
# ----------------------------------------------------------------------------------------------
def _finish(jobs):
    for part, rows, pitch, n, out in jobs:
        out.copy_(torch.as_strided(part, (rows, n), (pitch, 1)).double().sum(0).float())


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M", [948, 37, 6])
@pytest.mark.parametrize("D", [768, 128])
@pytest.mark.parametrize("add2", [False, True])
@pytest.mark.parametrize("defer", [False, True])
def test_layernorm_bwd_rowscale(dt, M, D, add2, defer):
    """dx, dgamma and dbeta are bit for bit those of the call without a factor; the copy is rowscale[m] * dx[m] (a second f32 buffer
    in f32 mode) and the third column sum the sum of the scaled rows, against fp64 torch."""
    x = rnd(M, D, seed=12, scale=3.0).to(DEV) + 0.5
    g = (rnd(D, seed=13) * 0.3 + 1).to(DEV)
    b = rnd(D, seed=14).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-6, dt)
    dy = rnd(M, D, seed=15).to(TD[dt]).to(DEV)
    dres = rnd(M, D, seed=16).to(DEV)
    dres2 = rnd(M, D, seed=17, scale=2.0).to(DEV) if add2 else None
    rs = _factors(M, 7 if M > 20 else 1).to(DEV)
    xr = x.double().cpu().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (D,), g.double().cpu(), b.double().cpu(), 1e-6).backward(dy.double().cpu())
    want = xr.grad + dres.double().cpu() + (dres2.double().cpu() if add2 else 0)
    want_s = want * rs.double().cpu()[:, None]

    def call(rowscale):
        dg, db, dcol = (torch.full((D,), 7.0, device=DEV) for _ in range(3))
        jobs = [] if defer else None
        kw = dict(dcolsum=dcol, defer=jobs, **({} if rowscale is None else dict(rowscale=rowscale)))
        if add2:
            dx, lp = ops.layernorm_bwd2(dy, x, g, mean, rstd, dres, dres2, dg, db, True, **kw)
        else:
            dx, lp = ops.layernorm_bwd(dy, x, g, mean, rstd, dres, dg, db, True, **kw)
        if defer:
            _finish(jobs)
        return dx, lp, dg, db, dcol
    dx0, lp0, dg0, db0, _ = call(None)
    dx, lp, dg, db, dcol = call(rs)
    assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
    assert lp is not dx and lp.dtype == TD[dt] and lp.data_ptr() != dx.data_ptr()
    e = dict(dx=rel_err(dx, want), lp=rel_err(lp, want_s), dcol=rel_err(dcol, want_s.sum(0)))
    record(f"drop_path.layernorm_bwd[{dt},{M},{D},{int(add2)},{'partial' if defer else 'full'}]", **e)
    assert e["dx"] < tol(PA_F32) and e["lp"] < tol(dt) and e["dcol"] < tol(PA_F32), e      # the sums are f32 arithmetic on either type
    zero = (rs == 0).nonzero().flatten()
    assert not lp[zero].any()                                                          # a dropped clip sends nothing into the branch


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", [(37, 128), (948, 768)])
@pytest.mark.parametrize("add2", [False, True])
def test_layernorm_bwd_null_factor_is_todays_entry(dt, M, D, add2):
    """The C entries: pa_layernorm_bwd[_partial]_rowscale with rowscale = NULL against pa_layernorm_bwd[2][_partial], every output and
    the whole partial-row workspace, bit for bit."""
    lib = _lib.load()
    x = rnd(M, D, seed=22, scale=3.0).to(DEV) + 0.5
    g = (rnd(D, seed=23) * 0.3 + 1).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, g, torch.zeros_like(g), 1e-6, dt)
    dy, dres = rnd(M, D, seed=25).to(TD[dt]).to(DEV), rnd(M, D, seed=26).to(DEV)
    dres2 = rnd(M, D, seed=27).to(DEV) if add2 else None
    st = torch.cuda.current_stream().cuda_stream
    nws = lib.pa_layernorm_bwd_ws_floats(M, D)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def bufs():
        return dict(dx=torch.empty(M, D, device=DEV), lp=torch.empty(M, D, device=DEV, dtype=TD[dt]), ws=torch.zeros(nws, device=DEV),
                    dg=torch.empty(D, device=DEV), db=torch.empty(D, device=DEV), dc=torch.empty(D, device=DEV))
    head = (p(dy), dt, p(x), p(g), p(mean), p(rstd), p(dres))
    for partial in (False, True):
        o, n = bufs(), bufs()
        if partial:
            old = lib.pa_layernorm_bwd2_partial(*head, p(dres2), p(o["dx"]), p(o["lp"]), p(o["ws"]), M, D, st) if add2 else \
                lib.pa_layernorm_bwd_partial(*head, p(o["dx"]), p(o["lp"]), p(o["ws"]), M, D, st)
            new = lib.pa_layernorm_bwd_partial_rowscale(*head, p(dres2), None, p(n["dx"]), p(n["lp"]), p(n["ws"]), M, D, st)
        else:
            tail = lambda d: (p(d["dx"]), p(d["lp"]), p(d["dg"]), p(d["db"]), p(d["dc"]), 0, p(d["ws"]), M, D, st)  # noqa: E731
            old = lib.pa_layernorm_bwd2(*head, p(dres2), *tail(o)) if add2 else lib.pa_layernorm_bwd(*head, *tail(o))
            new = lib.pa_layernorm_bwd_rowscale(*head, p(dres2), None, *tail(n))
        torch.cuda.synchronize()
        assert old == 0 and new == 0
        for k in ("dx", "lp", "ws") + (() if partial else ("dg", "db", "dc")):
            assert torch.equal(o[k], n[k]), (partial, k)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", [(12, 128), (948, 768)])
def test_convert_rowscale(dt, M, D):
    """the copy that carries the head's gradient into the last block's MLP branch: (dtype)(rowscale[m] * x[m]), one rounding"""
    x, rs = rnd(M, D, seed=31).to(DEV), _factors(M).to(DEV)
    out = ops.convert(x, dt, rowscale=rs)
    assert out.dtype == TD[dt] and out.data_ptr() != x.data_ptr()
    assert torch.equal(out, (x * rs[:, None]).to(TD[dt]))


# ----------------------------------------------------------------------------------------------
# the model against the reference's fixture
# ----------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build(case, precision, rate=DG.RATE):
    cfg = case["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.PaSST(u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"], s_patchout_f=cfg["s_patchout_f"],
                            img_size=cfg["img_size"], patch_size=cfg["patch"], stride=cfg["stride"], num_classes=cfg["num_classes"],
                            embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], distilled=True,
                            drop_path_rate=rate)
    sd = detgen.passt_state_dict(cfg, case["seed"])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m.precision = precision
    return m.to(DEV)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "drop_path.npz")))


def _step(m, case, masks, route):
    """(logits, features, block-1 output, dx, {parameter: gradient}) of one train-mode step of the fixture's loss with the masks fed
    through ``drop_path_masks``: ``route`` "autograd" = net(x); loss.backward(), "direct" = passt_forward / passt_backward."""
    x, a, b = HG.inputs(case)
    torch.manual_seed(case["torch_seed"])              # the Patchout draws are the fixture's
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if route == "autograd":
            m.input_grad = True
            m.zero_grad()
            xg = _dev(x).requires_grad_(True)
            logits, feat, hs = m(xg, hidden=(DG.HIDDEN,), drop_path_masks=masks)
            ((logits * _dev(a)).sum() + (feat * _dev(b)).sum()).backward()
            grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
            return logits.detach(), feat.detach(), hs[0].detach(), xg.grad, grads
        logits, feat, ctx, hs = P.passt_forward(m, _dev(x), True, hidden=P.parse_hidden((DG.HIDDEN,), len(m.blocks)), drop_path_masks=masks)
        grads = {n: torch.full_like(p, float("nan")) for n, p in m.named_parameters() if not n.startswith("head_dist.")}
        dx = P.passt_backward(m, ctx, _dev(a), _dev(b), grads, want_dx=True)
        return logits, feat, hs[0], dx, grads


@pytest.mark.parametrize("name", list(DG.CASES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("route", ["autograd", "direct"])
def test_model_vs_reference_fixture(gold, name, precision, route):
    case = DG.CASES[name]
    m = build(case, precision).train()
    masks = torch.from_numpy(gold[name + ".masks"])
    logits, feat, h, dx, grads = _step(m, case, masks, route)
    key = f"{name}.hidden.b{DG.HIDDEN}"
    assert tuple(h.shape) == tuple(gold[key + ".shape"]) and dx.shape == (case["B"], 1, case["cfg"]["img_size"][0], case["T"])
    metrics = dict(logits=rel(logits.cpu(), gold[name + ".logits"]), features=rel(feat.cpu(), gold[name + ".features"]),
                   hidden=rel(G.pin_sample(h.cpu().numpy(), DG.SAMPLE), gold[key]),
                   dx=rel(G.pin_sample(dx.cpu().numpy(), DG.SAMPLE), gold[name + ".dx"]))
    for k in DG.PARAM_GRADS:
        metrics["grad." + k] = rel(G.pin_sample(grads[k].cpu().numpy(), DG.SAMPLE), gold[f"{name}.grad.{k}"])
    record(f"drop_path.model.{name}[{precision},{route}]", **metrics)
    lim_out, lim_g = (1e-3, 1e-3) if precision == "fp32" else (BF16_LOGITS, BF16_GRADS)
    for k, v in metrics.items():
        assert v < (lim_g if k.startswith(("dx", "grad.")) else lim_out), (k, v, metrics)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dropped_branch_leaves_the_clip_rows_untouched(gold, precision):
    """Flipping ONE clip's MLP mask in block 1 changes block 1's output on that clip's rows only: every other clip's rows are bit for
    bit what they were (a factor of 0 adds nothing; nothing else crosses clips).  And a clip dropped in both branches of block 1 leaves
    that block with the rows it entered with."""
    name = "plain"
    case = DG.CASES[name]
    m = build(case, precision).train()
    masks = torch.from_numpy(gold[name + ".masks"]).clone()
    x = _dev(HG.inputs(case)[0])

    def hidden(mk, which):
        torch.manual_seed(case["torch_seed"])
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return m(x, hidden=which, drop_path_masks=mk)[2]
    base = hidden(masks, (DG.HIDDEN,))[0]
    clip = int((masks[1, 1] == 1).nonzero()[0])
    flipped = masks.clone()
    flipped[1, 1, clip] = 0
    other = hidden(flipped, (DG.HIDDEN,))[0]
    rest = [b for b in range(case["B"]) if b != clip]
    assert torch.equal(other[rest], base[rest]) and not torch.equal(other[clip], base[clip])
    both = masks.clone()
    both[1, :, clip] = 0
    h0, h1 = hidden(both, (0, 1))
    assert torch.equal(h1[clip], h0[clip]) and not torch.equal(h1[rest[0]], h0[rest[0]])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_eval_equals_a_model_without_drop_path(precision):
    case = DG.CASES["patchout"]
    x = _dev(HG.inputs(case)[0])
    outs = []
    for rate in (DG.RATE, 0.0):
        m = build(case, precision, rate).eval()
        with torch.no_grad():
            outs.append(m(x, drop_path_masks=torch.zeros(3, 2, case["B"])) if rate else m(x))      # masks are ignored in eval
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_device_draws_follow_the_reference_order():
    """In train mode net(x) consumes the device generator as 2 (depth - 1) torch.rand((B, 1, 1)) calls do, and computes what a
    second run fed those masks explicitly computes, bit for bit."""
    case = DG.CASES["plain"]
    m = build(case, "bf16").train()
    x = _dev(HG.inputs(case)[0])
    B, depth = case["B"], case["cfg"]["depth"]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(123)
        drawn = m(x)
        state = torch.cuda.get_rng_state()
        torch.manual_seed(123)
        for _ in range(2 * (depth - 1)):
            torch.rand((B, 1, 1), dtype=torch.float32, device=DEV)
        assert torch.equal(torch.cuda.get_rng_state(), state)
        torch.manual_seed(123)
        masks = (P.drop_path_draws(m, B, x.device) > 0).float()
        assert 0 < masks[1:].sum() < masks[1:].numel()
        torch.manual_seed(123)
        state = torch.cuda.get_rng_state()
        fed = m(x, drop_path_masks=masks)
        assert torch.equal(torch.cuda.get_rng_state(), state)          # nothing drawn
    assert torch.equal(drawn[0], fed[0]) and torch.equal(drawn[1], fed[1])


def test_train_step_graph_equals_eager_with_drop_path():
    """TrainStep(graph=True) on a model with drop_path_rate = 0.2: the step's factors are drawn ahead of the replay into a buffer of
    fixed address; 3 warm-up steps and 2 replayed ones leave the parameters and moments of the eager TrainStep, bit for bit."""
    from passt_amd.train import TrainStep
    case = dict(G.CASES["model_small_train"], seed=961)
    x, y = G.model_inputs(case)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    outs = []
    for graph in (False, True):
        net = build(case, "bf16", rate=0.2).train()
        ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=True, graph=graph)
        losses = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for step in range(5):
                torch.manual_seed(80 + step)
                np.random.seed(80 + step)
                losses.append(ts.step(xg, yg).clone())
        torch.cuda.synchronize()
        assert ts.t == 5 and (not graph or ("graph" in ts._g and ts._g["dp"] is not None))
        outs.append((torch.cat([l.reshape(1) for l in losses]).cpu(), ts.flat_p.clone(), ts.m.clone(), ts.v.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)

"""``net(x, hidden=...)`` on the HIP path: the two new kernels against fp64 torch, the model against the real reference's fixture
(tests/golden/hidden.npz: forward hooks on ``blocks[i]`` / ``norm``), and the invariants of the interface.

Bounds are the project's own: tests.test_gpu_kernels.tol for the kernels, 1e-3 (fp32) and BF16_LOGITS / BF16_GRADS of
tests/test_gpu_model.py for the model (BF16_LOGITS also for the token outputs), error = largest deviation over the largest reference
entry as in tests/test_gpu_input_grad.py.  Every measured value is recorded through test_gpu_kernels.record() / test_gpu_model.record()
(kernel_parity_metrics.json, model_parity_metrics.json; the "hidden." entries are filed as profiles/hidden_parity_metrics.json).

Every test fails on the parent commit with a TypeError on the ``hidden=`` keyword (the kernel tests: on the missing ops)."""
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import ops  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_hidden_golden as HG  # noqa: E402
from tests.test_gpu_input_grad import _Count  # noqa: E402
from tests.test_gpu_kernels import TD, rel_err, rnd, tol  # noqa: E402
from tests.test_gpu_kernels import record as record_kernel  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, BF16_LOGITS, DEV, build, rel  # noqa: E402
from tests.test_gpu_model import record as record_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def record(name, **kw):
    """into the suite's own parity files (test_gpu_kernels.record for kernels, test_gpu_model.record for the model), and printed"""
    (record_model if name.startswith("hidden.") else record_kernel)(name, **kw)
    print(name, {k: float(v) for k, v in kw.items()})


# ----------------------------------------------------------------------------------------------
# kernels
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", [(37, 128), (1000, 768), (130, 1024), (64, 192)])
@pytest.mark.parametrize("defer", [False, True])
def test_layernorm_bwd_second_addend(dt, M, D, defer):
    """pa_layernorm_bwd2 / pa_layernorm_bwd2_partial against fp64 torch at test_gpu_kernels.test_layernorm's shapes; with the second
    addend folded into the first by hand the old entry gives the same dx to rounding, and the column sums and the 16-bit copy
    include the addend."""
    x = rnd(M, D, seed=12, scale=3.0).to(DEV) + 0.5
    g = (rnd(D, seed=13) * 0.3 + 1).to(DEV)
    b = rnd(D, seed=14).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-6, dt)
    xr = x.double().cpu().requires_grad_(True)
    gr, br = g.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    dy = rnd(M, D, seed=15).to(TD[dt]).to(DEV)
    dres, dres2 = rnd(M, D, seed=16).to(DEV), rnd(M, D, seed=17, scale=2.0).to(DEV)
    torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-6).backward(dy.double().cpu())
    want = xr.grad + dres.double().cpu() + dres2.double().cpu()
    dg, db, dcol = (torch.full((D,), 7.0, device=DEV) for _ in range(3))
    jobs = [] if defer else None
    dx, dx_lp = ops.layernorm_bwd2(dy, x, g, mean, rstd, dres, dres2, dg, db, True, dcolsum=dcol, defer=jobs)
    if defer:                                    # finish the partial rows the way the block's finishing launch does
        assert [j[4] is o for j, o in zip(jobs, (dg, db, dcol))] == [True] * 3
        for part, rows, pitch, n, out in jobs:
            out.copy_(torch.as_strided(part, (rows, n), (pitch, 1)).double().sum(0).float())
    e = dict(dx=rel_err(dx, want), dgamma=rel_err(dg, gr.grad), dbeta=rel_err(db, br.grad), dcol=rel_err(dcol, want.sum(0)),
             lp=rel_err(dx_lp, dx))
    record(f"layernorm_bwd2[{dt},{M},{D},{'partial' if defer else 'full'}]", **e)
    assert max(e["dx"], e["dgamma"], e["dbeta"], e["dcol"]) < tol(PA_F32), e         # f32 arithmetic on either input type
    assert e["lp"] < tol(dt, 1e-7, 5e-3)
    # no first addend: the second alone
    dx1, _ = ops.layernorm_bwd2(dy, x, g, mean, rstd, None, dres2, dg, db, True)
    assert rel_err(dx1, xr.grad + dres2.double().cpu()) < tol(PA_F32)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", [(37, 128), (1000, 768)])
def test_layernorm_bwd_null_addend_is_bit_identical_to_the_old_entries(dt, M, D):
    """The C entries themselves: pa_layernorm_bwd2[_partial] with dres2 = NULL against pa_layernorm_bwd[_partial], every output
    and the whole partial-row workspace, bit for bit."""
    from passt_amd import _lib
    lib = _lib.load()
    x = rnd(M, D, seed=22, scale=3.0).to(DEV) + 0.5
    g = (rnd(D, seed=23) * 0.3 + 1).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, g, torch.zeros_like(g), 1e-6, dt)
    dy, dres = rnd(M, D, seed=25).to(TD[dt]).to(DEV), rnd(M, D, seed=26).to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    nws = lib.pa_layernorm_bwd_ws_floats(M, D)

    def bufs():
        return dict(dx=torch.empty(M, D, device=DEV), lp=torch.empty(M, D, device=DEV, dtype=TD[dt]), ws=torch.zeros(nws, device=DEV),
                    dg=torch.empty(D, device=DEV), db=torch.empty(D, device=DEV), dc=torch.empty(D, device=DEV))
    p = lambda t: t.data_ptr()  # noqa: E731
    for partial in (False, True):
        o, n = bufs(), bufs()
        if partial:
            rc0 = lib.pa_layernorm_bwd_partial(p(dy), dt, p(x), p(g), p(mean), p(rstd), p(dres), p(o["dx"]), p(o["lp"]), p(o["ws"]), M, D, st)
            rc1 = lib.pa_layernorm_bwd2_partial(p(dy), dt, p(x), p(g), p(mean), p(rstd), p(dres), None, p(n["dx"]), p(n["lp"]), p(n["ws"]), M, D, st)
        else:
            rc0 = lib.pa_layernorm_bwd(p(dy), dt, p(x), p(g), p(mean), p(rstd), p(dres), p(o["dx"]), p(o["lp"]), p(o["dg"]), p(o["db"]),
                                       p(o["dc"]), 0, p(o["ws"]), M, D, st)
            rc1 = lib.pa_layernorm_bwd2(p(dy), dt, p(x), p(g), p(mean), p(rstd), p(dres), None, p(n["dx"]), p(n["lp"]), p(n["dg"]), p(n["db"]),
                                        p(n["dc"]), 0, p(n["ws"]), M, D, st)
        torch.cuda.synchronize()
        assert rc0 == 0 and rc1 == 0
        for k in ("dx", "lp", "ws") + (() if partial else ("dg", "db", "dc")):
            assert torch.equal(o[k], n[k]), (partial, k)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", [(37, 128), (1000, 768), (130, 1024), (64, 192)])
@pytest.mark.parametrize("addends", [(False, False), (True, False), (False, True), (True, True)])
def test_tail_inject(dt, M, D, addends):
    """pa_tail_inject against fp64 torch: both addends optional, the scattered rows land on idx only, every element is written (the
    outputs start as NaN) and the 16-bit copy is the f32 result rounded once."""
    n_idx = max(2, 2 * (M // 40))
    idx = torch.arange(n_idx // 2, dtype=torch.int32).repeat_interleave(2) * (M // (n_idx // 2)) + torch.tensor([0, 1], dtype=torch.int32).repeat(n_idx // 2)
    rows = rnd(n_idx, D, seed=31).to(DEV)
    a0 = rnd(M, D, seed=32).to(DEV) if addends[0] else None
    a1 = rnd(M, D, seed=33, scale=0.5).to(DEV) if addends[1] else None
    want = torch.zeros(M, D, dtype=torch.float64)
    for a in (a0, a1):
        if a is not None:
            want += a.double().cpu()
    want[idx.long()] += rows.double().cpu()
    dx, dx_lp = ops.tail_inject(rows, idx.to(DEV), M, a0, a1, dt)
    torch.cuda.synchronize()
    assert dx.shape == (M, D) and dx.dtype == torch.float32 and torch.isfinite(dx).all()
    e = rel_err(dx, want)
    assert e < tol(PA_F32), e
    if dt == PA_F32:
        assert dx_lp is dx
    else:
        assert dx_lp.dtype == torch.bfloat16 and torch.equal(dx_lp, dx.to(torch.bfloat16))
    if not any(addends):                         # what scatter_rows_into_zeros gave: exact zeros elsewhere, the rows themselves on idx
        assert torch.equal(dx, ops.scatter_rows_into_zeros(rows, idx.to(DEV), M))
    record(f"tail_inject[{dt},{M},{D},{int(addends[0])}{int(addends[1])}]", dx=e)
    assert torch.equal(ops.tail_inject(rows, idx.to(DEV), M, a0, a1, dt)[0], dx)             # bit-repeatable


# ----------------------------------------------------------------------------------------------
# model against the reference's fixture
# ----------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def product_step(case, precision, m=None, hidden="case", use_hidden=True, x_grad=True):
    """(model, logits, features, [token outputs], x leaf) after one backward of the fixture's loss.  ``hidden``: the request ("case" =
    the fixture's; None = a plain call); ``use_hidden=False``: the loss reads logits / features only."""
    if m is None:
        m = build(case, precision)
        m.train(case["training"])
        m.requires_grad_(not case["frozen"])
        m.input_grad = True
    hidden = case["hidden"] if hidden == "case" else hidden
    x, a, b = HG.inputs(case)
    xg = _dev(x).requires_grad_(x_grad)
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = m(xg) if hidden is None else m(xg, hidden=hidden)
    logits, feat, hs = out[0], out[1], (out[2] if hidden is not None else [])
    cs = [_dev(HG.hidden_weights(case["seed"], h, tuple(t.shape))) for h, t in zip(hidden or (), hs)] if use_hidden else []
    HG.loss_of(logits, feat, hs if use_hidden else [], _dev(a), _dev(b), cs, case.get("hidden_only", False) and use_hidden).backward()
    return m, logits.detach(), feat.detach(), [h.detach() for h in hs], xg


def _limits(precision):
    return (1e-3, 1e-3) if precision == "fp32" else (BF16_LOGITS, BF16_GRADS)


def _hidden_metrics(gold, prefix, hidden, hs, metrics):
    for h, t in zip(hidden, hs):
        k = f"{prefix}.hidden.{HG.key_of(h)}"
        tn = t.cpu().numpy()
        assert t.dtype == torch.float32 and tuple(tn.shape) == tuple(gold[k + ".shape"]), (k, tn.shape)
        metrics["hidden." + HG.key_of(h)] = rel(G.pin_sample(tn, HG.SAMPLE), gold[k])
        nrm = float(gold[k + ".stats"][0])
        metrics["hidden." + HG.key_of(h) + "_norm"] = abs(float(np.linalg.norm(tn.astype(np.float64))) - nrm) / nrm


@pytest.mark.parametrize("name", list(HG.CASES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_hidden_vs_reference_fixture(golden_dir, name, precision):
    """Token outputs, logits, features, dx and the two recorded parameter gradients against the reference's hooks and autograd.
    The bf16 error of the token outputs had not been measured when this was written; every value is recorded."""
    gold = dict(np.load(os.path.join(golden_dir, "hidden.npz")))
    case = HG.CASES[name]
    m, logits, feat, hs, xg = product_step(case, precision)
    assert xg.grad is not None and xg.grad.shape == xg.shape
    metrics = dict(logits=rel(logits.cpu(), gold[name + ".logits"]), features=rel(feat.cpu(), gold[name + ".features"]))
    _hidden_metrics(gold, name, case["hidden"], hs, metrics)
    dxn = xg.grad.cpu().numpy()
    metrics["dx"] = rel(G.pin_sample(dxn, HG.SAMPLE), gold[name + ".dx"])
    nrm = float(gold[name + ".dx.stats"][0])
    metrics["dx_norm"] = abs(float(np.linalg.norm(dxn.astype(np.float64))) - nrm) / nrm
    params = dict(m.named_parameters())
    for k in HG.PARAM_GRADS:
        if case["frozen"]:
            assert params[k].grad is None, k
        else:
            metrics["grad." + k] = rel(G.pin_sample(params[k].grad.cpu().numpy(), HG.SAMPLE), gold[f"{name}.grad.{k}"])
    record(f"hidden.{name}[{precision}]", **metrics)
    # "norm" rows 0 / 1 are the tokens whose mean is `features`
    if "norm" in case["hidden"]:
        hn = hs[case["hidden"].index("norm")]
        assert rel(hn[:, :2].mean(1).cpu(), feat.cpu()) < 1e-5       # an f32 LayerNorm of the same f32 rows in both precisions
    lim_out, lim_g = _limits(precision)
    for k, v in metrics.items():
        assert v < (lim_g if k.startswith(("dx", "grad.")) else lim_out), (k, v, metrics)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_hidden_matches_every_clip_alone(golden_dir, precision):
    """The packed path: rows tok_offsets[i] : tok_offsets[i + 1] and dx[i] against the reference run on clip i alone at batch size 1;
    dx is exactly 0 behind a clip's frames; a parameter gradient is the sum over the clips."""
    gold = dict(np.load(os.path.join(golden_dir, "hidden.npz")))
    case, lengths = HG.RAGGED, HG.RAGGED["lengths"]
    m = build(case, precision).eval()
    m.varlen_grad = True
    x, a, b = HG.ragged_inputs()
    xg = _dev(x).requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, feat, hs, tok = m(xg, lengths=lengths, hidden=case["hidden"])
    assert tok.dtype == torch.int64 and tok.device.type == "cpu" and tok.shape == (len(lengths) + 1,) and int(tok[0]) == 0
    D = case["cfg"]["embed_dim"]
    assert all(h.shape == (int(tok[-1]), D) and h.dtype == torch.float32 for h in hs)
    ntok = (tok[1:] - tok[:-1]).tolist()
    cs = [_dev(np.concatenate([HG.hidden_weights(case["seed"], h, (1, n, D), clip=i)[0] for i, n in enumerate(ntok)])) for h in case["hidden"]]
    HG.loss_of(logits, feat, hs, _dev(a), _dev(b), cs).backward()
    dx = xg.grad.cpu().numpy()
    lim_out, lim_g = _limits(precision)
    for i, n in enumerate(lengths):
        pre = f"ragged.{i}"
        metrics = dict(logits=rel(logits[i:i + 1].detach().cpu(), gold[pre + ".logits"]), features=rel(feat[i:i + 1].detach().cpu(), gold[pre + ".features"]))
        _hidden_metrics(gold, pre, case["hidden"], [h.detach()[int(tok[i]):int(tok[i + 1])][None] for h in hs], metrics)
        metrics["dx"] = rel(G.pin_sample(dx[i:i + 1, :, :, :n], HG.SAMPLE), gold[pre + ".dx"])
        assert (dx[i, :, :, n:] == 0).all()
        record(f"hidden.ragged.{i}[{precision}]", **metrics)
        for k, v in metrics.items():
            assert v < (lim_g if k.startswith("dx") else lim_out), (i, k, v, metrics)
    params = dict(m.named_parameters())
    metrics = {k: rel(G.pin_sample(params[k].grad.cpu().numpy(), HG.SAMPLE), gold[f"ragged.grad.{k}"]) for k in HG.PARAM_GRADS}
    record(f"hidden.ragged.grads[{precision}]", **metrics)
    assert all(v < lim_g for v in metrics.values()), metrics


# ----------------------------------------------------------------------------------------------
# invariants, on the HIP path itself
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_logits_and_features_with_and_without_hidden(precision):
    """Below the last block a request changes no launch: logits / features bit for bit.  A last-block / "norm" request runs the last
    block through the all-queries attention kernel instead of the 2-query form, which orders its sums differently: equal within the
    model bounds only (1e-3 / BF16_LOGITS), not bit for bit."""
    case = HG.CASES["intermediate"]
    m = build(case, precision).eval()
    x = _dev(HG.inputs(case)[0])
    with torch.no_grad():
        lo, fe = m(x)
        for k in (0, 1, -2):
            lo1, fe1, hs = m(x, hidden=[k])
            assert torch.equal(lo, lo1) and torch.equal(fe, fe1) and hs[0].shape == (x.shape[0], 290, 128)
        # the grid recipe: eval-mode rows 2.. are frequency-major F' x T'
        assert hs[0][:, 2:].view(x.shape[0], 12, 24, 128).shape == (x.shape[0], 12, 24, 128)
        lim = _limits(precision)[0]
        for req in ([-1], ["norm"], [2, "norm", 0]):
            lo2, fe2, hs2 = m(x, hidden=req)
            e = dict(logits=rel(lo2.cpu(), lo.cpu()), features=rel(fe2.cpu(), fe.cpu()))
            record(f"hidden.full_tail_vs_prefix_tail[{precision},{req}]", **e)
            assert e["logits"] < lim and e["features"] < lim, e
        # block 0's tokens do not depend on what else was asked for
        assert torch.equal(hs2[2], m(x, hidden=[0])[2][0])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_requested_but_unused_output_changes_no_gradient(precision):
    """An intermediate output that does not feed the loss arrives as None in the backward: dx and every parameter gradient are bit
    for bit those of the call without ``hidden`` (train mode with Patchout, the same draws)."""
    case = HG.CASES["patchout_train"]
    m0, lo0, fe0, _, x0 = product_step(case, precision, hidden=None)
    m1, lo1, fe1, hs, x1 = product_step(case, precision, hidden=(0,), use_hidden=False)
    assert len(hs) == 1 and torch.equal(lo0, lo1) and torch.equal(fe0, fe1) and torch.equal(x0.grad, x1.grad)
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        if n.startswith("head_dist."):
            assert p0.grad is None and p1.grad is None
        else:
            assert torch.equal(p0.grad, p1.grad), n


@pytest.mark.parametrize("hidden", [(0,), (0, -1, "norm")])
def test_frozen_network_runs_no_weight_gradient(hidden, monkeypatch):
    case = dict(HG.CASES["hidden_only"], frozen=True, hidden=hidden)
    m = build(case, "bf16").eval().requires_grad_(False)
    x, a, b = HG.inputs(case)
    xg = _dev(x).requires_grad_()
    logits, feat, hs = m(xg, hidden=hidden)
    assert all(h.grad_fn is not None for h in hs)
    count = _Count(monkeypatch)
    alloc = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *s, **k: alloc.append(s) or real_empty(*s, **k))
    sum((h * h).sum() for h in hs).backward()
    monkeypatch.undo()
    assert count.n == {}, count.n                         # no weight-gradient GEMM, no bias / parameter column sum
    n_params = sum(p.numel() for n, p in m.named_parameters() if not n.startswith("head_dist."))
    assert not any(len(s) == 1 and s[0] == n_params for s in alloc)        # no flat gradient buffer
    assert all(p.grad is None for p in m.parameters()) and xg.grad is not None and float(xg.grad.abs().max()) > 0


def test_flat_bound_optimizer_route_gives_the_same_gradients():
    """passt_amd.optim.AdamW binds the model to one flat gradient buffer (the node takes a token instead of the parameters): a loss
    on token outputs gives the same dx and the same parameter gradients as the per-parameter route, bit for bit."""
    from passt_amd import optim as pa_optim
    case = HG.CASES["patchout_train"]
    x, a, b = HG.inputs(case)

    def run(flat):
        if not flat:
            os.environ["PASST_AMD_NO_FLAT_GRADS"] = "1"
        try:
            net = build(case, "bf16").train()
            net.input_grad = True
            opt = pa_optim.AdamW(net.parameters(), lr=1e-3)
            dxs, gs = [], []
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for i in range(3):
                    torch.manual_seed(90 + i)
                    opt.zero_grad()
                    xg = _dev(x).requires_grad_()
                    lo, fe, hs = net(xg, hidden=case["hidden"])
                    cs = [_dev(HG.hidden_weights(case["seed"], h, tuple(t.shape))) for h, t in zip(case["hidden"], hs)]
                    HG.loss_of(lo, fe, hs, _dev(a), _dev(b), cs).backward()
                    gs.append({n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None})
                    opt.step()
                    dxs.append(xg.grad)
            return net, dxs, gs
        finally:
            os.environ.pop("PASST_AMD_NO_FLAT_GRADS", None)

    net_u, dx_u, g_u = run(False)
    net_b, dx_b, g_b = run(True)
    assert net_u._flat is None and net_b._flat is not None
    for i in range(3):
        assert torch.equal(dx_u[i], dx_b[i]), i
        assert g_u[i].keys() == g_b[i].keys() and len(g_u[i]) > 20
        for n in g_u[i]:
            assert torch.equal(g_u[i][n], g_b[i][n]), (i, n)


# ----------------------------------------------------------------------------------------------
# two gloo ranks on one GPU
# ----------------------------------------------------------------------------------------------
WORKER = os.path.join(ROOT, "tests", "ddp_hidden_worker.py")


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


def test_attached_reducer_averages_a_hidden_state_loss(tmp_path):
    """passt_amd.ddp.attach, two ranks on the one GPU over gloo, a loss on token outputs (intermediate block, last block, "norm") plus
    logits / features: the parameter gradients are the mean of the two ranks' own gradients -- which the single process computes
    one half-batch at a time -- and every rank's dx is the unscaled gradient of its own loss."""
    ref = _run(str(tmp_path / "ref.pt"), 1)
    dp = _run(str(tmp_path / "dp.pt"), 2)
    want = (ref["grads"][0].double() + ref["grads"][1].double()) / 2
    e = float((dp["grads"][0].double() - want).abs().max() / want.abs().max())
    same = bool(torch.equal(dp["grads"][0], dp["grads"][1]))
    e_dx = [float((dp["dx"][r].double() - ref["dx"][r].double()).abs().max() / ref["dx"][r].double().abs().max()) for r in range(2)]
    record("hidden.ddp_attach[fp32]", grads=e, dx0=e_dx[0], dx1=e_dx[1])
    assert same and e < 1e-5 and max(e_dx) < 1e-5, (same, e, e_dx)

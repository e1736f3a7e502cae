"""The gradient w.r.t. the input spectrogram on the HIP path: the fold kernel against torch's fold, the model against the real
reference's fixture (tests/golden/input_grad.npz) and the oracle, and the autograd semantics of ``x.requires_grad_()``.

Bounds are the project's own: tests.test_gpu_kernels.tol (2e-5 / 1.2e-2) for the kernel, 1e-3 (fp32) and BF16_LOGITS / BF16_GRADS
of tests/test_gpu_model.py for the model.  Every measured value is recorded through test_gpu_model.record() (model_parity_metrics.json).
"""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from passt_amd import ops  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32  # noqa: E402
from passt_amd.passt import patchout_draws  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_input_grad_golden as IG  # noqa: E402
from tests.test_gpu_kernels import TD, tol  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, BF16_LOGITS, DEV, build, record, rel  # noqa: E402
from tests.test_input_grad_cpu import oracle_step  # noqa: E402


# ----------------------------------------------------------------------------------------------
# kernel
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("subset", ["full", "random"])
@pytest.mark.parametrize("stride,T", [((10, 10), 998), ((12, 12), 250), ((14, 14), 333), ((16, 16), 320), ((20, 20), 250),
                                      ((10, 16), 331)])
def test_patch_input_bwd_vs_torch_fold(stride, T, subset, dt):
    """ops.patch_input_bwd against torch.nn.functional.fold in float64 on the CPU (dropped patches = zero columns); dx is pre-filled
    with NaN, so an element the kernel does not write fails the comparison."""
    B, F, P = 3, 128, 16
    fs, ts = stride
    Fg, Tg = (F - P) // fs + 1, (T - P) // ts + 1
    gen = torch.Generator().manual_seed(1000 * fs + ts + T)
    if subset == "full":
        keep = torch.arange(Fg * Tg)
    else:
        keep = torch.randperm(Fg * Tg, generator=gen)[:max(1, (Fg * Tg) // 3)].sort().values
    pf, pt = (keep // Tg).to(torch.int32), (keep % Tg).to(torch.int32)
    Np = keep.numel()
    dcols = ((torch.rand(B * Np, P * P, generator=gen) * 2 - 1)).to(TD[dt])
    # reference: scatter the kept rows into the full unfold layout [B][P*P][Fg*Tg], fold in float64
    full = torch.zeros(B, P * P, Fg * Tg, dtype=torch.float64)
    full[:, :, keep] = dcols.double().view(B, Np, P * P).transpose(1, 2)
    ref = torch.nn.functional.fold(full, output_size=(F, T), kernel_size=P, stride=(fs, ts))
    dx = torch.full((B, 1, F, T), float("nan"), device=DEV)
    assert ops.patch_input_bwd(dcols.to(DEV), pf.to(DEV), pt.to(DEV), B, F, T, P, fs, ts, out=dx) is dx
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
    err = float((dx.double().cpu() - ref).abs().max() / ref.abs().max())
    record(f"patch_input_bwd[{fs}x{ts},T{T},{subset},{'f32' if dt == PA_F32 else 'bf16'}]", err=err)
    assert err < tol(dt), err
    uncovered = ref == 0                        # (a covered pixel sums random values: never exactly 0)
    assert (dx.cpu()[uncovered] == 0).all()
    # deterministic: no atomics, no dependence on what ran before
    dx2 = ops.patch_input_bwd(dcols.to(DEV), pf.to(DEV), pt.to(DEV), B, F, T, P, fs, ts)
    assert dx2.shape == (B, 1, F, T) and dx2.dtype == torch.float32 and torch.equal(dx, dx2)


def test_patch_input_bwd_rejects_bad_shapes():
    from passt_amd._lib import PasstAmdError
    pf = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(PasstAmdError):
        ops.patch_input_bwd(torch.zeros(8, 255, device=DEV), pf, pf, 2, 128, 100, 16, 10, 10)       # not P*P columns
    with pytest.raises(PasstAmdError):
        ops.patch_input_bwd(torch.zeros(8, 256, device=DEV), pf, pf, 2, 128, 15, 16, 10, 10)        # shorter than one patch
    with pytest.raises(PasstAmdError):
        ops.patch_input_bwd(torch.zeros(8, 256, device=DEV), pf, pf, 2, 16, 16, 16, 10, 10)         # more kept patches than grid cells


# ----------------------------------------------------------------------------------------------
# model against the reference's fixture and the oracle
# ----------------------------------------------------------------------------------------------
def product_step(case, precision, m=None, x_grad=True):
    """(model, logits, features, x leaf) after one backward of the fixture's loss."""
    if m is None:
        m = build(case, precision)
        m.train(case["training"])
        m.requires_grad_(not case["frozen"])
        m.input_grad = True                     # needed (and only looked at) when parameters are trainable
    x, a, b = IG.inputs(case)
    xg = torch.from_numpy(x).to(DEV).requires_grad_(x_grad)
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, feat = m(xg)
    IG.loss_of(logits, feat, torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).backward()
    return m, logits.detach(), feat.detach(), xg


def covered_pixels(m, case):
    """bool [F][T]: pixels under at least one kept patch, from the product's own draws (same seed, same call order)."""
    x_shape = (case["B"], 1, case["cfg"]["img_size"][0], case["T"])
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = patchout_draws(m, x_shape)
    P, (fs, ts) = case["cfg"]["patch"], case["cfg"]["stride"]
    cov = np.zeros(x_shape[2:], bool)
    for f, t in zip(d["pf"], d["pt"]):
        cov[f * fs:f * fs + P, t * ts:t * ts + P] = True
    return cov


@pytest.mark.parametrize("name", list(IG.CASES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_input_grad_vs_reference_fixture(golden_dir, name, precision):
    """Measured on MI355X (profiles/input_grad_model_parity_metrics.json): fp32 dx 1.1e-6 .. 2.7e-6, bf16 dx 5.7e-3 .. 8.7e-3 (the same
    runs' patch_embed.proj.weight gradient 4.4e-3 .. 8.6e-3), against bounds of 1e-3 and BF16_GRADS = 2.5e-2."""
    gold = dict(np.load(os.path.join(golden_dir, "input_grad.npz")))
    case = IG.CASES[name]
    m, logits, feat, xg = product_step(case, precision)
    dx = xg.grad
    assert dx is not None and dx.shape == xg.shape and dx.dtype == torch.float32
    dxn = dx.cpu().numpy()
    metrics = dict(logits=rel(logits.cpu(), gold[name + ".logits"]), features=rel(feat.cpu(), gold[name + ".features"]),
                   dx=rel(G.pin_sample(dxn, IG.DX_SAMPLE), gold[name + ".dx"]))
    nrm = float(gold[name + ".dx.stats"][0])
    metrics["dx_norm"] = abs(float(np.linalg.norm(dxn.astype(np.float64))) - nrm) / nrm
    # the whole dx (not a sample) against the oracle's autograd, itself pinned to the fixture by tests/test_input_grad_cpu.py
    _, _, odx, osd = oracle_step(case)
    metrics["dx_vs_oracle"] = rel(dxn, odx.numpy())
    params = dict(m.named_parameters())
    for k in IG.PARAM_GRADS:
        if case["frozen"]:
            assert params[k].grad is None, k
        else:
            got = params[k].grad.cpu().numpy()
            metrics["grad." + k] = rel(G.pin_sample(got, IG.DX_SAMPLE), gold[f"{name}.grad.{k}"])
    if case["frozen"]:
        assert all(p.grad is None for p in m.parameters())
    record(f"input_grad.{name}[{precision}]", **metrics)
    print(f"input_grad.{name}[{precision}]", metrics)
    # exactly zero where no kept patch reaches: dropped Patchout patches, behind the time cut, behind the last patch row / column
    cov = covered_pixels(m, case)
    assert (dxn[:, 0][:, ~cov] == 0).all()
    lim_out, lim_g = (1e-3, 1e-3) if precision == "fp32" else (BF16_LOGITS, BF16_GRADS)
    assert metrics["logits"] < lim_out and metrics["features"] < lim_out, metrics
    for k, v in metrics.items():
        if k.startswith(("dx", "grad.")):
            assert v < lim_g, (k, v, metrics)


# ----------------------------------------------------------------------------------------------
# autograd semantics
# ----------------------------------------------------------------------------------------------
SMALL_EVAL = dict(IG.CASES["batch4"], seed=77)


def _loss(case, logits, feat):
    _, a, b = IG.inputs(case)
    return IG.loss_of(logits, feat, torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))


def test_input_requiring_grad_gets_one():
    """fails on the parent commit: forward() raised NotImplementedError for an input that requires a gradient"""
    case = dict(SMALL_EVAL, frozen=True)
    m, logits, feat, xg = product_step(case, "fp32")
    assert xg.grad is not None and xg.grad.shape == xg.shape and float(xg.grad.abs().max()) > 0


class _Count:
    def __init__(self, monkeypatch):
        self.n = {}
        for name in ("wgrad", "wgrad_tn", "wgrad_tn_batched", "colsum", "colsum_f32"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def counted(*a, **k):
            self.n[name] = self.n.get(name, 0) + 1
            return fn(*a, **k)
        return counted


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frozen_network_has_grad_fn_and_runs_no_weight_gradient(precision, monkeypatch):
    case = dict(SMALL_EVAL, frozen=True)
    m = build(case, precision).eval().requires_grad_(False)
    x, _, _ = IG.inputs(case)
    xg = torch.from_numpy(x).to(DEV).requires_grad_()
    logits, feat = m(xg)
    assert logits.grad_fn is not None and feat.grad_fn is not None
    count = _Count(monkeypatch)
    _loss(case, logits, feat).backward()
    assert count.n == {}, count.n                         # no weight-gradient GEMM, no bias / parameter column sum
    assert all(p.grad is None for p in m.parameters())
    assert xg.grad is not None
    # the same net with trainable parameters does launch them (the counter sees what it is meant to see)
    m.requires_grad_(True)
    m.input_grad = True
    xg2 = torch.from_numpy(x).to(DEV).requires_grad_()
    lo2, fe2 = m(xg2)
    _loss(case, lo2, fe2).backward()
    assert sum(count.n.values()) > 0
    # and the input gradient does not depend on which parameters were trainable (same kernels up to the epilogue variants that
    # also produce bias sums)
    assert rel(xg2.grad.cpu(), xg.grad.cpu()) < (1e-6 if precision == "fp32" else BF16_GRADS)
    # only `features` feeding the loss / only logits
    m.requires_grad_(False)
    xg3 = torch.from_numpy(x).to(DEV).requires_grad_()
    m(xg3)[1].sum().backward()
    xg4 = torch.from_numpy(x).to(DEV).requires_grad_()
    m(xg4)[0].sum().backward()
    assert float(xg3.grad.abs().max()) > 0 and float(xg4.grad.abs().max()) > 0
    # ... and with trainable parameters (no logits gradient arrives at the node)
    m.requires_grad_(True)
    m.zero_grad()
    xg5 = torch.from_numpy(x).to(DEV).requires_grad_()
    m(xg5)[1].sum().backward()
    assert rel(xg5.grad.cpu(), xg3.grad.cpu()) < (1e-6 if precision == "fp32" else BF16_GRADS)
    assert m.head[1].weight.grad is not None and float(m.head[1].weight.grad.abs().max()) == 0


def test_gradient_comes_back_in_the_callers_shape_dtype_and_layout():
    case = dict(SMALL_EVAL, frozen=True)
    m = build(case, "fp32").eval().requires_grad_(False)
    x, _, _ = IG.inputs(case)
    xc = torch.from_numpy(x).to(DEV).requires_grad_()
    lo, fe = m(xc)
    _loss(case, lo, fe).backward()
    # a slice of a longer leaf: non-contiguous
    base = torch.zeros(x.shape[0], 1, x.shape[2], x.shape[3] + 57, device=DEV)
    base[..., 30:30 + x.shape[3]] = torch.from_numpy(x).to(DEV)
    base.requires_grad_()
    xs = base[..., 30:30 + x.shape[3]]
    assert not xs.is_contiguous()
    lo, fe = m(xs)
    _loss(case, lo, fe).backward()
    assert base.grad.shape == base.shape
    assert torch.equal(base.grad[..., 30:30 + x.shape[3]], xc.grad)
    assert float(base.grad[..., :30].abs().max()) == 0 and float(base.grad[..., 30 + x.shape[3]:].abs().max()) == 0
    # a transposed layout and a 16-bit leaf
    xt = torch.from_numpy(x).to(DEV).transpose(2, 3).contiguous().requires_grad_()
    lo, fe = m(xt.transpose(2, 3))
    _loss(case, lo, fe).backward()
    assert xt.grad.shape == xt.shape and torch.equal(xt.grad.transpose(2, 3), xc.grad)
    xh = torch.from_numpy(x).to(DEV).half().requires_grad_()
    lo, fe = m(xh)
    _loss(case, lo, fe).backward()
    assert xh.grad.dtype == torch.float16 and xh.grad.shape == xh.shape


def test_second_backward_accumulates_into_x_grad():
    case = dict(SMALL_EVAL, frozen=True)
    m = build(case, "fp32").eval().requires_grad_(False)
    x, _, _ = IG.inputs(case)
    xg = torch.from_numpy(x).to(DEV).requires_grad_()
    lo, fe = m(xg)
    _loss(case, lo, fe).backward()
    g1 = xg.grad.clone()
    lo, fe = m(xg)
    _loss(case, lo, fe).backward()
    assert torch.equal(xg.grad, g1 + g1)
    with pytest.raises(RuntimeError):                       # the node's saved activations are consumed, as before
        _loss(case, lo, fe).backward()


def test_autograd_grad_wrt_input_leaves_parameter_grads_alone():
    case = dict(SMALL_EVAL, frozen=False)
    m = build(case, "fp32").eval()
    m.input_grad = True
    x, _, _ = IG.inputs(case)
    xg = torch.from_numpy(x).to(DEV).requires_grad_()
    lo, fe = m(xg)
    (dx,) = torch.autograd.grad(_loss(case, lo, fe), xg)
    assert dx.shape == xg.shape and xg.grad is None
    assert all(p.grad is None for p in m.parameters())
    _, _, _, ref = product_step(dict(case, frozen=True), "fp32")
    assert rel(dx.cpu(), ref.grad.cpu()) < 1e-6


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_parameter_gradients_do_not_change_when_the_input_asks_for_a_gradient(precision):
    """x not requiring a gradient runs today's kernel sequence; asking for dx adds launches behind it and changes no parameter
    gradient: both routes bit for bit (train mode with Patchout, the same draws)."""
    case = IG.CASES["patchout_train"]
    m0, lo0, fe0, _ = product_step(case, precision, x_grad=False)
    m1, lo1, fe1, x1 = product_step(case, precision, x_grad=True)
    assert torch.equal(lo0, lo1) and torch.equal(fe0, fe1) and x1.grad is not None
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        if n.startswith("head_dist."):
            assert p0.grad is None and p1.grad is None
        else:
            assert torch.equal(p0.grad, p1.grad), n


def test_flat_bound_optimizer_route_returns_the_same_dx():
    """passt_amd.optim.AdamW binds the model to one flat gradient buffer (the autograd node then takes a token instead of the
    parameters): dx comes back in x's slot there too, bit for bit what the per-parameter route returns."""
    from passt_amd import optim as pa_optim
    case = IG.CASES["patchout_train"]
    x, a, b = IG.inputs(case)

    def run(flat):
        if not flat:
            os.environ["PASST_AMD_NO_FLAT_GRADS"] = "1"
        try:
            net = build(case, "bf16").train()
            net.input_grad = True
            opt = pa_optim.AdamW(net.parameters(), lr=1e-3)
            grads = []
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for i in range(3):
                    torch.manual_seed(90 + i)
                    opt.zero_grad()
                    xg = torch.from_numpy(x).to(DEV).requires_grad_()
                    lo, fe = net(xg)
                    IG.loss_of(lo, fe, torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).backward()
                    opt.step()
                    grads.append(xg.grad)
            return net, grads
        finally:
            os.environ.pop("PASST_AMD_NO_FLAT_GRADS", None)

    net_u, g_u = run(False)
    net_b, g_b = run(True)
    assert net_u._flat is None and net_b._flat is not None
    for i, (u, v) in enumerate(zip(g_u, g_b)):
        assert u is not None and v is not None and torch.equal(u, v), i


def test_dx_under_an_attached_reducer_is_the_gradient_of_the_local_loss():
    """passt_amd.ddp.attach pre-scales dlogits by 1 / world (mean over ranks of the PARAMETER gradients); dx is not reduced and must
    stay the gradient of this rank's loss.  One rank, a stand-in reducer of world 2 that reduces nothing: parameter gradients come
    out halved, dx unchanged."""
    case = dict(SMALL_EVAL, frozen=False)
    m = build(case, "fp32").eval()
    m.input_grad = True
    _, _, _, x0 = product_step(case, "fp32", m=m)
    g0 = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad()

    class Reducer:
        world, flat = 2, None
        total = m._graph_params()[1]
        blocks = []

        def on_block_done(self, i):
            self.blocks.append(i)

        def wait(self):
            pass

    red = Reducer()
    object.__setattr__(m, "_ddp", red)
    _, _, _, x1 = product_step(case, "fp32", m=m)
    assert red.blocks and red.blocks[-1] == -1
    assert torch.equal(x1.grad, x0.grad)                  # (x * 0.5) * 2 is exact in binary floating point
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, g0[n] * 0.5), n
    # a frozen network under the reducer: nothing to reduce, no hook call, the same dx
    m.requires_grad_(False)
    m.zero_grad()
    red.blocks.clear()
    _, _, _, x2 = product_step(dict(case, frozen=True), "fp32", m=m)
    assert red.blocks == [] and rel(x2.grad.cpu(), x0.grad.cpu()) < 1e-6


def test_lengths_forward_stays_without_grad():
    case = dict(SMALL_EVAL, frozen=True)
    m = build(case, "fp32").eval().requires_grad_(False)
    x, _, _ = IG.inputs(case)
    xg = torch.from_numpy(x).to(DEV).requires_grad_()
    lo, fe = m(xg, lengths=[x.shape[3]] * x.shape[0])
    assert lo.grad_fn is None and fe.grad_fn is None


def test_gradient_descent_on_the_input_lowers_a_feature_matching_loss():
    """The use the feature exists for: a frozen PaSST as a loss network.  Ten steps of plain gradient descent on the spectrogram
    toward another clip's feature vector; the step size is a tenth of the step that would cancel the loss to first order
    (loss / |grad|^2), so every step must lower the loss (fp32)."""
    case = dict(SMALL_EVAL, frozen=True)
    m = build(case, "fp32").eval().requires_grad_(False)
    x, _, _ = IG.inputs(case)
    with torch.no_grad():
        target = m(torch.from_numpy(x[::-1].copy()).to(DEV))[1]
    xg = torch.from_numpy(x).to(DEV).requires_grad_()
    losses = []
    for _ in range(11):
        xg.grad = None
        loss = ((m(xg)[1] - target) ** 2).sum()
        loss.backward()
        losses.append(float(loss.detach()))
        with torch.no_grad():
            xg -= 0.1 * loss / (xg.grad ** 2).sum() * xg.grad
    record("input_grad.descent[fp32]", first=losses[0], last=losses[-1])
    print("descent losses", losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


def test_frozen_backbone_and_input_checks_with_an_input_that_requires_grad():
    """tests/test_gpu_model.py::test_frozen_parameters_and_input_checks with ``input_grad`` switched on: without the switch a net
    with trainable parameters still refuses an input that requires a gradient; with it, a frozen backbone hands gradients to the
    trainable parameters only, bit-identical to the fully trainable net's, the input gets its gradient, and the input checks
    still refuse what they refused."""
    case = dict(G.CASES["model_small_train"], seed=321)
    m = build(case, "fp32").train()
    for n, p in m.named_parameters():
        p.requires_grad_(n.startswith(("head.", "norm.")))
    x, y = G.model_inputs(case)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    m2 = build(case, "fp32").train()
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    assert m.input_grad is False
    for net in (m, m2):
        with pytest.raises(NotImplementedError, match="input_grad"):
            net(xg.clone().requires_grad_(True))
        net.input_grad = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(3)
        xr = xg.clone().requires_grad_(True)
        bce(m(xr)[0], yg).backward()
        torch.manual_seed(3)
        xr2 = xg.clone().requires_grad_(True)
        bce(m2(xr2)[0], yg).backward()
    for (n, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        if p.requires_grad:
            assert torch.equal(p.grad, p2.grad), n
        else:
            assert p.grad is None, n
    assert xr.grad is not None and torch.equal(xr.grad, xr2.grad)        # a partially frozen net computes everything, as before
    with pytest.raises(ValueError):
        m2(torch.zeros(2, 3, 128, 250, device=DEV).requires_grad_())
    with pytest.raises(ValueError):
        m2(torch.zeros(128, 250, device=DEV).requires_grad_())

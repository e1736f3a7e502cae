"""GPU tests of the gradient w.r.t. the waveform through the fused front end (pa_mel_frontend_bwd / _bwd_varlen, the autograd node
of passt_amd.AugmentMelSTFT).  Reference values: tests/golden/wave_grad.npz (the real reference's autograd, kept samples + whole-clip
statistics) and, on EVERY sample, the float64 oracle that tests/test_wave_grad_cpu.py checks against the same fixture.

Bounds.  Errors of dwave are taken per clip, relative to that clip's largest |dwave|.  The front end is f32 in both precision modes:
the limit is the parity-mode bound 1e-3 (an f32 kernel should land near the 0.6-2.3e-5 by which f32 and f64 autograd of the oracle
differ).  The end-to-end case through the bf16 network inherits the spectrogram gradient's limit, 2.5e-2 (BF16_GRADS)."""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from passt_amd import ops  # noqa: E402
from passt_amd._lib import MelParams, PasstAmdError  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_input_grad_golden as IG  # noqa: E402
from tests.golden import make_wave_grad_golden as WG  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, DEV, build, record  # noqa: E402
from tests.test_wave_grad_cpu import LIMIT, clip_errors, oracle_dwave  # noqa: E402


def module(case, training=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.AugmentMelSTFT(**case["kw"]).to(DEV)
    return m.train(case["training"] if training is None else training)


def product_dwave(case, wave_np, g_np, lengths=None, m=None):
    """(spec, dwave, frames) of this library under the fixture's loss."""
    m = module(case) if m is None else m
    w = torch.from_numpy(np.ascontiguousarray(wave_np)).to(DEV).requires_grad_()
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    frames = None
    if lengths is None:
        spec = m(w)
    else:
        spec, frames = m(w, lengths=lengths)
    (spec * torch.from_numpy(np.ascontiguousarray(g_np)).to(DEV)).sum().backward()
    return spec.detach(), w.grad, frames


def per_clip(got, ref):
    """largest error of one clip relative to the clip's largest reference magnitude"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def case_io(name):
    case = WG.CASES[name]
    T = WG.frames_of(case["L"], case["kw"].get("hopsize", 320))
    return case, G.frontend_inputs(case), WG.upstream(case, (case["B"], case["kw"].get("n_mels", 128), T))


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_wave_requiring_grad_gets_one():
    case, wave, g = case_io("frontend_eval")
    m = module(case)
    w = torch.from_numpy(wave).to(DEV).requires_grad_()
    spec = m(w)
    assert spec.grad_fn is not None and spec.requires_grad
    (spec * torch.from_numpy(g).to(DEV)).sum().backward()
    assert w.grad is not None and w.grad.shape == w.shape and w.grad.dtype == torch.float32
    assert torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0


@pytest.mark.parametrize("training", [False, True])
def test_plain_call_is_unchanged_and_rng_consumption_is_the_same(training):
    case, wave, _ = case_io("frontend_train")
    m = module(case, training)
    w = torch.from_numpy(wave).to(DEV)
    torch.manual_seed(11)
    plain = m(w)
    state_plain = torch.get_rng_state()
    assert plain.grad_fn is None and not plain.requires_grad
    torch.manual_seed(11)
    with torch.no_grad():
        ng = m(w.clone().requires_grad_())
    assert ng.grad_fn is None and torch.equal(ng, plain) and torch.equal(torch.get_rng_state(), state_plain)
    torch.manual_seed(11)
    wg = m(w.clone().requires_grad_())
    assert wg.grad_fn is not None and torch.equal(wg.detach(), plain) and torch.equal(torch.get_rng_state(), state_plain)


def test_gradient_comes_back_in_the_callers_dtype_and_layout():
    case, wave, g = case_io("frontend_esc50")
    m = module(case)
    _, ref, _ = product_dwave(case, wave, g, m=m)
    gt = torch.from_numpy(g).to(DEV)
    wd = torch.from_numpy(wave).to(DEV).double().requires_grad_()
    (m(wd) * gt).sum().backward()
    assert wd.grad.dtype == torch.float64 and torch.equal(wd.grad.float(), ref)
    wide = torch.zeros(case["B"], 2 * case["L"], device=DEV)
    wide[:, ::2] = torch.from_numpy(wave).to(DEV)
    wide.requires_grad_()
    (m(wide[:, ::2]) * gt).sum().backward()
    assert torch.equal(wide.grad[:, ::2], ref) and float(wide.grad[:, 1::2].abs().max()) == 0.0


def test_second_backward_and_double_backward_raise():
    case, wave, g = case_io("frontend_esc50")
    m = module(case)
    w = torch.from_numpy(wave).to(DEV).requires_grad_()
    loss = (m(w) * torch.from_numpy(g).to(DEV)).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed by a backward"):
        loss.backward()
    w2 = torch.from_numpy(wave).to(DEV).requires_grad_()
    loss = (m(w2) * torch.from_numpy(g).to(DEV)).sum()
    gw, = torch.autograd.grad(loss, w2, create_graph=True)
    with pytest.raises(RuntimeError):
        gw.sum().backward()                       # once_differentiable: no graph through the backward


def test_ops_reject_a_mismatched_upstream_gradient():
    case, wave, g = case_io("frontend_esc50")
    m = module(case)
    w = torch.from_numpy(wave).to(DEV)
    p = MelParams()
    p.n_fft, p.hop, p.n_mels, p.n_frames = 1024, 320, 128, WG.frames_of(case["L"])
    with pytest.raises(PasstAmdError):
        ops.mel_frontend_bwd(w, m._window_padded, m._bin_mel, m._twiddle, p, torch.zeros(2, 128, 7, device=DEV))
    with pytest.raises(PasstAmdError):
        ops.mel_frontend_bwd(w[:, :400].contiguous(), m._window_padded, m._bin_mel, m._twiddle, p, torch.zeros(2, 128, p.n_frames, device=DEV))
    m.train()
    with pytest.raises(NotImplementedError):
        m(w.clone().requires_grad_(), lengths=[case["L"]] * 2)


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WG.CASES))
def test_dwave_vs_reference_fixture_and_oracle(golden_dir, name):
    gold = dict(np.load(os.path.join(golden_dir, "wave_grad.npz")))
    case, wave, g = case_io(name)
    spec, dw, _ = product_dwave(case, wave, g)
    ospec, odw = oracle_dwave(case, wave, g)
    dw = dw.cpu().numpy()
    fig = {}
    for i in range(case["B"]):
        e = clip_errors(gold, f"{name}.dwave.{i}", dw[i], ten_s=name == "frontend_eval_10s")
        fig[f"clip{i}_fixture"], fig[f"clip{i}_absmax"], fig[f"clip{i}_norm"] = e
        fig[f"clip{i}_oracle64"] = per_clip(dw[i], odw[i].numpy())
    record(f"wave_grad.{name}", **fig)
    print(f"wave_grad.{name}", fig)
    assert float((spec.cpu().double() - ospec).abs().max()) < 1e-3           # the forward the node launched is the plain forward
    assert max(fig.values()) <= LIMIT, fig


def test_masked_cells_contribute_nothing(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "wave_grad.npz")))
    case, wave, g = case_io("frontend_train")
    fs, fe, ts, te = (int(v) for v in gold["frontend_train.mask"][2:])
    assert fe > fs and te > ts
    _, ref, _ = product_dwave(case, wave, g)
    g2 = g.copy()
    g2[:, max(fs, 0):fe, :] = np.nan                      # the upstream values at masked cells are not used
    g2[:, :, max(ts, 0):te] = 1e30
    spec, got, _ = product_dwave(case, wave, g2)
    assert torch.equal(got, ref)
    const = float(spec[0, max(fs, 0), 0])
    assert abs(const - 0.9) < 1e-6                        # the mask constant out_add * out_scale


def ragged_io():
    case = WG.RAGGED
    waves = G.frontend_inputs(case)
    g = WG.upstream(case, (case["B"], 128, WG.frames_of(max(WG.RAGGED_LENS))))
    padded = waves.copy()
    for i, n in enumerate(WG.RAGGED_LENS):
        padded[i, n:] = np.nan                            # samples behind a clip's end are never read
    return case, waves, padded, g


def test_ragged_dwave_vs_fixture_and_batch_1(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "wave_grad.npz")))
    case, waves, padded, g = ragged_io()
    m = module(case)
    gn = g.copy()
    for i, n in enumerate(WG.RAGGED_LENS):
        gn[i, :, WG.frames_of(n):] = np.nan               # nor is the upstream gradient behind a clip's frames
    spec, dw, frames = product_dwave(case, padded, gn, lengths=WG.RAGGED_LENS, m=m)
    assert frames.dtype == torch.int64 and not frames.is_cuda and frames.tolist() == [WG.frames_of(n) for n in WG.RAGGED_LENS]
    assert spec.shape == (4, 128, WG.frames_of(max(WG.RAGGED_LENS)))
    fig = {}
    for i, n in enumerate(WG.RAGGED_LENS):
        assert float(dw[i, n:].abs().max()) == 0.0 if n < dw.shape[1] else True       # exact zeros at and behind lengths[i]
        assert torch.isfinite(dw[i]).all()
        e = clip_errors(gold, f"ragged.dwave.{i}", dw[i, :n].cpu().numpy())
        fig[f"clip{i}_fixture"], fig[f"clip{i}_absmax"], fig[f"clip{i}_norm"] = e
        _, own, _ = product_dwave(case, waves[i:i + 1, :n], g[i:i + 1, :, :WG.frames_of(n)], m=m)
        assert torch.equal(own[0], dw[i, :n]), i                                      # this library's own batch-1 call, bit for bit
        _, odw = oracle_dwave(case, waves[i:i + 1, :n], g[i:i + 1, :, :WG.frames_of(n)])
        fig[f"clip{i}_oracle64"] = per_clip(dw[i, :n].cpu().numpy(), odw[0].numpy())
    record("wave_grad.ragged", **fig)
    print("wave_grad.ragged", fig)
    assert max(fig.values()) <= LIMIT, fig


def test_ragged_permutation_and_equal_lengths_are_bit_exact():
    case, waves, padded, g = ragged_io()
    m = module(case)
    _, dw, _ = product_dwave(case, padded, g, lengths=WG.RAGGED_LENS, m=m)
    perm = [2, 0, 3, 1]
    _, dwp, _ = product_dwave(case, padded[perm], g[perm], lengths=[WG.RAGGED_LENS[i] for i in perm], m=m)
    assert torch.equal(dwp, dw[perm])
    _, fixed, _ = product_dwave(case, waves, g, m=m)
    _, same, _ = product_dwave(case, waves, g, lengths=[case["L"]] * case["B"], m=m)
    assert torch.equal(same, fixed)
    _, tens, _ = product_dwave(case, waves, g, lengths=torch.tensor([case["L"]] * case["B"], device=DEV), m=m)
    assert torch.equal(tens, fixed)


def test_repeated_backward_calls_are_bit_identical():
    case, wave, g = case_io("frontend_train")
    m = module(case)
    runs = [product_dwave(case, wave, g, m=m)[1] for _ in range(4)]
    assert all(torch.equal(r, runs[0]) for r in runs[1:])
    case, waves, padded, g = ragged_io()
    m = module(case)
    runs = [product_dwave(case, padded, g, lengths=WG.RAGGED_LENS, m=m)[1] for _ in range(4)]
    assert all(torch.equal(r, runs[0]) for r in runs[1:])


# ---- the kernel alone, other filterbanks ----------------------------------------------------------------------------------
def restated_frontend(x, window, hop, n_mels, fmin, fmax, fmask, tmask):
    """The front end as torch ops in the tensor's own precision: pre-emphasis, reflect padding, frames, one-sided DFT, power, DENSE
    triangle filterbank (bin k on the kaldi mel scale; triangle j rises over [c_j, c_j+1) and falls over [c_j+1, c_j+2)), log, masks."""
    dt = x.dtype
    y = x[:, 1:] - 0.97 * x[:, :-1]
    yp = torch.nn.functional.pad(y.unsqueeze(1), (512, 512), mode="reflect").squeeze(1)
    fr = yp.unfold(1, 1024, hop) * window.to(dt)
    spec = torch.fft.rfft(fr, dim=-1)
    P = (spec.real ** 2 + spec.imag ** 2)[..., :512]
    k = torch.arange(512, dtype=torch.float64)
    lo, hi = 1127.0 * np.log1p(fmin / 700.0), 1127.0 * np.log1p(fmax / 700.0)
    t = (1127.0 * torch.log1p(k * (32000 / 1024) / 700.0) - lo) * (n_mels + 1) / (hi - lo)
    j, u = torch.floor(t).long(), t - torch.floor(t)
    basis = torch.zeros(n_mels, 512, dtype=torch.float64)
    for kk in range(512):
        if 0 <= j[kk] < n_mels:
            basis[j[kk], kk] += u[kk]
        if 1 <= j[kk] <= n_mels:
            basis[j[kk] - 1, kk] += 1.0 - u[kk]
    mel = torch.log(torch.matmul(basis.to(dt), P.transpose(1, 2)) + 1e-5)
    keep = torch.ones_like(mel)
    keep[:, fmask[0]:fmask[1], :] = 0
    keep[:, :, tmask[0]:tmask[1]] = 0
    return (mel * keep + 4.5) / 5.0


@pytest.mark.parametrize("n_mels,fmin,fmax,hop,L,masks", [(8, 2000.0, 2600.0, 320, 9000, ((0, 0), (0, 0))),
                                                           (40, 300.0, 7000.0, 320, 12345, ((5, 9), (3, 11))),
                                                           (128, 0.0, 15000.0, 1024, 20000, ((0, 0), (0, 0))),
                                                           (64, 50.0, 14000.0, 37, 3000, ((60, 64), (0, 2))),
                                                           (4, 100.0, 16000.0, 250, 1100, ((0, 0), (0, 0)))])
def test_kernel_alone_on_other_filterbanks(n_mels, fmin, fmax, hop, L, masks):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.AugmentMelSTFT(n_mels=n_mels, hopsize=hop, fmin=fmin, fmax=fmax).to(DEV).eval()
    B, T = 3, WG.frames_of(L, hop)
    wave = G.frontend_inputs(dict(B=B, L=L, seed=61))
    g = detgen.uniform(61, "g", (B, n_mels, T), -1.0, 1.0)
    p = MelParams()
    p.n_fft, p.hop, p.n_mels, p.n_frames, p.preemph = 1024, hop, n_mels, T, 0.97
    lo, hi = 1127.0 * np.log1p(fmin / 700.0), 1127.0 * np.log1p(fmax / 700.0)
    p.mel_low, p.inv_mel_delta = lo, (n_mels + 1) / (hi - lo)
    p.log_eps, p.out_add, p.out_scale = 0.00001, 4.5, 0.2
    (p.fmask_start, p.fmask_end), (p.tmask_start, p.tmask_end) = masks
    w = torch.from_numpy(wave).to(DEV)
    dw = ops.mel_frontend_bwd(w, m._window_padded, m._bin_mel, m._twiddle, p, torch.from_numpy(g).to(DEV)).cpu().numpy()
    x64 = torch.from_numpy(wave).double().requires_grad_()
    out = restated_frontend(x64, m._window_padded.cpu().double(), hop, n_mels, fmin, fmax, *masks)
    (out * torch.from_numpy(g).double()).sum().backward()
    fwd = ops.mel_frontend(w, m._window_padded, m._bin_mel, m._twiddle, p).cpu().double()
    assert float((fwd - out.detach()).abs().max()) < 2e-3                   # the restatement is the forward the kernel differentiates
    errs = {f"clip{i}": per_clip(dw[i], x64.grad[i].numpy()) for i in range(B)}
    record(f"wave_grad.kernel[{n_mels},{fmin:.0f}-{fmax:.0f},hop{hop},L{L}]", **errs)
    print("wave_grad.kernel", n_mels, fmin, fmax, hop, L, errs)
    assert max(errs.values()) <= LIMIT, errs


# ---- end to end: wave -> mel -> frozen PaSST -> loss -> wave.grad ---------------------------------------------------------
def e2e_net(precision):
    case = WG.E2E
    net = build(dict(cfg=case["cfg"], seed=case["net_seed"]), precision).eval()
    net.requires_grad_(False)
    return case, net


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_end_to_end_through_the_frozen_network(golden_dir, precision):
    gold = dict(np.load(os.path.join(golden_dir, "wave_grad.npz")))
    case, net = e2e_net(precision)
    m = module(case)
    a, b = (torch.from_numpy(v).to(DEV) for v in WG.e2e_inputs(case))
    lim = LIMIT if precision == "fp32" else BF16_GRADS
    wave = G.frontend_inputs(case)
    fig = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = torch.from_numpy(wave).to(DEV).requires_grad_()
        logits, feat = net(m(w)[:, None])
        IG.loss_of(logits, feat, a, b).backward()
        fixed = w.grad
        for i in range(case["B"]):
            e = clip_errors(gold, f"e2e.dwave.{i}", fixed[i].cpu().numpy())
            fig[f"clip{i}_fixture"], fig[f"clip{i}_absmax"], fig[f"clip{i}_norm"] = e
        # the packed path: mel(wave, lengths=n) -> net(spec[:, None], lengths=frames) with varlen_grad
        net.varlen_grad = True
        lens = [case["L"], 48000]
        w2 = torch.from_numpy(wave).to(DEV).requires_grad_()
        spec, frames = m(w2, lengths=lens)
        logits2, feat2 = net(spec[:, None], lengths=frames)
        IG.loss_of(logits2, feat2, a, b).backward()
        assert w2.grad is not None and float(w2.grad[1, lens[1]:].abs().max()) == 0.0
        fig["packed_clip0_vs_fixed"] = per_clip(w2.grad[0].cpu().numpy(), fixed[0].cpu().numpy())
        # clip 1 cut to 48 000 samples, alone through the fixed-length path
        net.varlen_grad = False
        w3 = torch.from_numpy(wave[1:2, :lens[1]].copy()).to(DEV).requires_grad_()
        l3, f3 = net(m(w3)[:, None])
        IG.loss_of(l3, f3, a[1:2], b[1:2]).backward()
        fig["packed_clip1_vs_alone"] = per_clip(w2.grad[1, :lens[1]].cpu().numpy(), w3.grad[0].cpu().numpy())
    record(f"wave_grad.e2e[{precision}]", **fig)
    print(f"wave_grad.e2e[{precision}]", fig)
    assert max(fig.values()) <= lim, fig

"""GPU tests of the training-mode front end on ragged batches (``mel.train(); mel.varlen_train = True; mel(wave, lengths=...)``;
pa_mel_frontend_fwd_varlen_aug / pa_mel_frontend_bwd_varlen_aug).

Contract: every clip gets what ``mel.train()(wave[i:i+1, :lengths[i]])`` gives it alone -- its own fmin / fmax jitter, its own frequency
band, its own time band drawn against its own frames -- the draws being made clip after clip with the reference's RNG calls.  Reference
values: tests/golden/varlen_mel_train.npz (the real reference in training mode, one clip at a time under one seed).

Bounds are the neighbours': 1e-3 absolute on the spectrogram (tests/test_gpu_varlen.py::test_frontend_varlen), LIMIT = 1e-3 on dwave per
clip relative to the clip's largest |dwave| (tests/test_gpu_wave_grad.py), 1e-3 for the fp32 model (tests/test_gpu_varlen_train.py).
The mask constant is out_add * out_scale in f32, 4.5f * 0.2f -- "0.9" to one ulp, the fixed path's value.  Clip 3 (2 frames) lies wholly
under its time band: its dwave is exactly zero in the reference and must be here.  No MI355X figures yet: none could
be taken when this was written; every test prints and records (record(...)) what it measures before it asserts.
"""
import functools
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from oracle import passt_oracle as O  # noqa: E402
from passt_amd import ops  # noqa: E402
from passt_amd._lib import MelParams  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_mel_train_golden as MT  # noqa: E402
from tests.golden import make_varlen_train_golden as VT  # noqa: E402
from tests.test_gpu_model import DEV, build, record, rel  # noqa: E402
from tests.test_wave_grad_cpu import LIMIT, clip_errors  # noqa: E402

LENGTHS, FRAMES, B = MT.LENGTHS, [MT.frames_of(n) for n in MT.LENGTHS], len(MT.LENGTHS)
MASK_CONST = np.float32(4.5) * np.float32(1.0 / 5.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "varlen_mel_train.npz")


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(GOLDEN))


def _mel(train=True, switch=True):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.AugmentMelSTFT(**MT.MEL_KW).to(DEV).train(train)
    m.varlen_train = switch
    return m


@functools.lru_cache(maxsize=None)
def _io():
    """(waves, waves with NaN behind every clip's end, upstream gradient, upstream gradient with NaN behind every clip's frames)"""
    w, g = MT.wave_input(), MT.upstream()
    wn, gn = w.copy(), g.copy()
    for i, (n, T) in enumerate(zip(LENGTHS, FRAMES)):
        wn[i, n:] = np.nan
        gn[i, :, T:] = np.nan
    return w, wn, g, gn


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _packed():
    """The packed training call under the fixture's seed on the NaN-padded inputs, with its backward: computed once, shared, never
    modified.  The upstream gradient is NaN behind every clip's own frames."""
    w, wn, g, gn = _io()
    m = _mel()
    x = _t(wn).requires_grad_()
    torch.manual_seed(MT.TORCH_SEED)
    spec, frames = m(x, lengths=LENGTHS)
    state = torch.get_rng_state()
    spec.backward(_t(gn))                                   # NaN behind every clip's frames: the backward must not use it
    torch.cuda.synchronize()
    return spec.detach(), frames, x.grad, state


@functools.lru_cache(maxsize=None)
def _loop():
    """This library's own batch-1 training loop under the same seed: [(spec_i, dwave_i)], final generator state."""
    w, _, g, _ = _io()
    m = _mel()
    out = []
    torch.manual_seed(MT.TORCH_SEED)
    for i, (n, T) in enumerate(zip(LENGTHS, FRAMES)):
        x = _t(w[i:i + 1, :n]).requires_grad_()
        spec = m(x)
        spec.backward(_t(g[i:i + 1, :, :T]))
        out.append((spec.detach()[0], x.grad[0]))
    torch.cuda.synchronize()
    return out, torch.get_rng_state()


def _draw(i):
    return _gold()[f"draw.{i}"]


def _params(T_max, draw=None):
    """MelParams of the module's settings; ``draw`` = (fmin, fmax, fs, fe, ts, te) or None for the un-jittered, un-masked ones"""
    fmin, fmax, fs, fe, ts, te = (0.0, 15000.0, 0, 0, 0, 0) if draw is None else draw
    p = MelParams()
    p.n_fft, p.hop, p.n_mels, p.n_frames, p.preemph = 1024, 320, 128, T_max, 0.97
    lo, hi = 1127.0 * math.log(1.0 + fmin / 700.0), 1127.0 * math.log(1.0 + fmax / 700.0)      # the module's expressions
    p.mel_low, p.inv_mel_delta = lo, 129 / (hi - lo)
    p.log_eps, p.out_add, p.out_scale = 0.00001, 4.5, 1.0 / 5.0
    p.fmask_start, p.fmask_end, p.tmask_start, p.tmask_end = int(fs), int(fe), int(ts), int(te)
    return p


def _row(draw):
    fmin, fmax, fs, fe, ts, te = draw
    lo, hi = 1127.0 * math.log(1.0 + fmin / 700.0), 1127.0 * math.log(1.0 + fmax / 700.0)      # the module's expressions
    return (lo, 129 / (hi - lo), int(fs), int(fe), int(ts), int(te))


# ---- forward ---------------------------------------------------------------------------------------------------------------------
def test_forward_vs_fixture_and_batch_1_loop():
    gold = _gold()
    spec, frames, _, state = _packed()
    loop, loop_state = _loop()
    assert frames.dtype == torch.int64 and not frames.is_cuda and frames.tolist() == FRAMES == gold["frames"].tolist()
    assert spec.shape == (B, 128, max(FRAMES)) and spec.dtype == torch.float32
    assert np.array_equal(state.numpy(), gold["rng"]) and torch.equal(state, loop_state)      # the same draws, the same final state
    fig = {}
    for i, T in enumerate(FRAMES):
        got = spec[i, :, :T].cpu().numpy()
        assert np.isfinite(got).all(), i                                  # the NaNs behind the clip's end in the input do not show
        assert (spec[i, :, T:] == 0.0).all(), i                           # exactly 0.0 behind the clip's end, not the mask constant
        masked = MT.masked_cells(_draw(i), T)
        assert np.array_equal(got == MASK_CONST, masked), i               # exactly the clip's own two bands hold the constant
        fig[f"clip{i}_fixture"] = float(np.abs(G.pin_sample(got, MT.MEL_SAMPLE) - gold[f"mel.{i}"]).max())
        fig[f"clip{i}_batch1"] = float((spec[i, :, :T] - loop[i][0]).abs().max())
    record("varlen_mel_train.forward", **fig)
    print("varlen_mel_train.forward", fig)
    assert abs(float(MASK_CONST) - 0.9) < 1e-6
    assert max(fig.values()) < 1e-3, fig


# ---- backward --------------------------------------------------------------------------------------------------------------------
def test_backward_vs_fixture_and_batch_1_loop_bit_for_bit():
    gold = _gold()
    _, _, dw, _ = _packed()
    loop, _ = _loop()
    assert dw.shape == (B, max(LENGTHS)) and torch.isfinite(dw).all()
    fig = {}
    for i, n in enumerate(LENGTHS):
        if n < dw.shape[1]:
            assert float(dw[i, n:].abs().max()) == 0.0, i                 # exactly zero at and behind lengths[i]
        assert torch.equal(dw[i, :n], loop[i][1]), i                      # this library's own batch-1 training call, bit for bit
        if gold[f"dwave.{i}.stats"][1] == 0.0:                            # the clip that lies wholly under its time band
            assert float(dw[i].abs().max()) == 0.0, i
            continue
        e = clip_errors(gold, f"dwave.{i}", dw[i, :n].cpu().numpy())
        fig[f"clip{i}_fixture"], fig[f"clip{i}_absmax"], fig[f"clip{i}_norm"] = e
    record("varlen_mel_train.backward", **fig)
    print("varlen_mel_train.backward", fig)
    assert len(fig) == 3 * (B - 1) and max(fig.values()) <= LIMIT, fig


def test_upstream_gradient_on_masked_cells_and_behind_the_frames_is_not_used():
    w, wn, g, gn = _io()
    _, _, ref, _ = _packed()
    g2 = gn.copy()
    for i, T in enumerate(FRAMES):
        fs, fe, ts, te = (int(v) for v in _draw(i)[2:])
        g2[i, max(fs, 0):max(fe, 0), :] = 1e30
        g2[i, :, max(ts, 0):max(te, 0)] = np.nan
    m = _mel()
    x = _t(wn).requires_grad_()
    torch.manual_seed(MT.TORCH_SEED)
    spec, _ = m(x, lengths=LENGTHS)
    spec.backward(_t(g2))
    assert torch.equal(x.grad, ref)


# ---- invariants of the two entry points ------------------------------------------------------------------------------------------
def _ops_fwd_bwd(m, wave, lens, rows, g, fill=0.0):
    T_max = max(MT.frames_of(n) for n in lens)
    p = _params(T_max)
    lens_dev = ops.upload_small(torch.tensor(lens, dtype=torch.int32), DEV)
    clip_dev = ops.upload_mel_clips(rows, DEV)
    tabs = (m._window_padded, m._bin_mel, m._twiddle)
    spec = ops.mel_frontend_varlen_aug(wave, lens_dev, clip_dev, *tabs, p, fill=fill)
    dw = ops.mel_frontend_bwd_varlen_aug(wave, lens_dev, clip_dev, *tabs, p, g)
    return spec, dw


def test_permuting_the_clips_permutes_the_rows_bit_for_bit():
    w, wn, g, gn = _io()
    m = _mel()
    rows = [_row(_draw(i)) for i in range(B)]
    spec, dw = _ops_fwd_bwd(m, _t(wn), LENGTHS, rows, _t(gn))
    ref_spec, _, ref_dw, _ = _packed()
    assert torch.equal(spec, ref_spec) and torch.equal(dw, ref_dw)        # the module's call is this call
    perm = [3, 0, 4, 2, 1]
    sp, dp = _ops_fwd_bwd(m, _t(wn[perm]), [LENGTHS[i] for i in perm], [rows[i] for i in perm], _t(gn[perm]))
    assert torch.equal(sp, spec[perm]) and torch.equal(dp, dw[perm])
    # `fill` behind the clips' ends, never the mask constant (clip 3's time band reaches to frame 16, the clip has 2)
    sf, _ = _ops_fwd_bwd(m, _t(wn), LENGTHS, rows, _t(gn), fill=-7.0)
    for i, T in enumerate(FRAMES):
        assert (sf[i, :, T:] == -7.0).all() and torch.equal(sf[i, :, :T], spec[i, :, :T]), i


@pytest.mark.parametrize("draw", [None, (5.0, 15832, 76, 98, 89, 122)])
def test_a_uniform_table_gives_the_varlen_entry_points_outputs_bit_for_bit(draw):
    w, wn, g, gn = _io()
    m = _mel()
    T_max = max(FRAMES)
    p = _params(T_max, draw)
    lens_dev = ops.upload_small(torch.tensor(LENGTHS, dtype=torch.int32), DEV)
    tabs = (m._window_padded, m._bin_mel, m._twiddle)
    row = _row((0.0, 15000.0, 0, 0, 0, 0) if draw is None else draw)
    clip_dev = ops.upload_mel_clips([row] * B, DEV)
    q = _params(T_max, (123.0, 9000.0, 1, 127, 0, 150))                   # the six per-clip fields of *p are ignored by the _aug form
    wave, gt = _t(wn), _t(gn)
    assert torch.equal(ops.mel_frontend_varlen_aug(wave, lens_dev, clip_dev, *tabs, q), ops.mel_frontend_varlen(wave, lens_dev, *tabs, p))
    assert torch.equal(ops.mel_frontend_bwd_varlen_aug(wave, lens_dev, clip_dev, *tabs, q, gt),
                       ops.mel_frontend_bwd_varlen(wave, lens_dev, *tabs, p, gt))


# ---- interface -------------------------------------------------------------------------------------------------------------------
def test_switch_eval_mode_device_lengths_and_second_backward():
    w, wn, g, gn = _io()
    wave = _t(wn)
    ref_spec, ref_frames, _, ref_state = _packed()
    with pytest.raises(NotImplementedError, match="varlen_train"):
        _mel(switch=False)(wave, lengths=LENGTHS)
    # eval mode ignores the switch: today's result bit for bit, two randint consumed, no masks
    torch.manual_seed(9)
    today, _ = _mel(train=False, switch=False)(wave, lengths=LENGTHS)
    torch.manual_seed(9)
    ev, frames = _mel(train=False)(wave, lengths=LENGTHS)
    state = torch.get_rng_state()
    torch.manual_seed(9)
    torch.randint(10, (1,)), torch.randint(2000, (1,))
    assert torch.equal(ev, today) and frames.tolist() == FRAMES and torch.equal(torch.get_rng_state(), state)
    assert not (ev[0, :, :FRAMES[0]] == float(MASK_CONST)).any()
    # lengths as a device tensor is the same call
    m = _mel()
    torch.manual_seed(MT.TORCH_SEED)
    spec, frames = m(wave, lengths=torch.tensor(LENGTHS, device=DEV))
    assert torch.equal(spec, ref_spec) and torch.equal(frames, ref_frames) and torch.equal(torch.get_rng_state(), ref_state)
    assert spec.grad_fn is None                                           # no gradient wanted: the plain launch, the same bits
    # a rejected call consumes nothing
    state = torch.get_rng_state()
    with pytest.raises(passt_amd._lib.PasstAmdError, match="clip 3"):
        m(wave, lengths=[48000, 5120, 20001, 513, 48000])
    with pytest.raises(ValueError):
        m(wave, lengths=LENGTHS[:-1])
    assert torch.equal(torch.get_rng_state(), state)
    # one backward per forward
    x = _t(w).requires_grad_()
    loss = (m(x, lengths=LENGTHS)[0] * _t(g)).sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed by a backward"):
        loss.backward()


# ---- end to end: wave -> mel.varlen_train -> net.varlen_train -> loss -> wave.grad ------------------------------------------------
def test_end_to_end_is_the_batch_1_loop():
    """fp32, depth 2, img_size (128, 256).  The packed path draws every front-end number before any Patchout number, so the loop runs
    every clip alone through ``mel`` first and then every clip alone through ``net``.  Bounds: 1e-3 on logits and on wave.grad per clip
    relative to the clip's largest entry (test_packed_training_step_is_the_batch_1_loop, fp32)."""
    lens = [48000, 5120, 20001]                                            # 150 / 16 / 63 frames: 14 / 1 / 5 patch columns
    case = dict(cfg=O.make_cfg(embed_dim=128, depth=2, num_heads=2, num_classes=5, img_size=(128, 256), u_patchout=5), seed=58)
    w = MT.wave_input()[:3]
    a = _t(detgen.uniform(58, "a", (3, 5), -1.0, 1.0))
    b = _t(detgen.uniform(58, "b", (3, 128), -1.0, 1.0))
    m = _mel()
    net = build(case, "fp32").train()
    net.varlen_train = True
    net.input_grad = True                                                  # for the loop's fixed-path calls; the packed path does not consult it
    wn = w.copy()
    for i, n in enumerate(lens):
        wn[i, n:] = np.nan
    x = _t(wn).requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(31)
        spec, frames = m(x, lengths=lens)
        logits, feat = net(spec[:, None], lengths=frames)
        VT.loss_of(logits, feat, a, b).backward()
        state = torch.get_rng_state()
        # the loop: all front-end draws first, then the network clip by clip
        torch.manual_seed(31)
        xs = [_t(w[i:i + 1, :n]).requires_grad_() for i, n in enumerate(lens)]
        specs = [m(xi) for xi in xs]
        fig = {}
        for i, (xi, si) in enumerate(zip(xs, specs)):
            lo, fe = net(si[:, None])
            VT.loss_of(lo, fe, a[i:i + 1], b[i:i + 1]).backward()
            fig[f"clip{i}_logits"] = rel(logits[i].detach().cpu(), lo[0].detach().cpu())
            fig[f"clip{i}_features"] = rel(feat[i].detach().cpu(), fe[0].detach().cpu())
            fig[f"clip{i}_dwave"] = rel(x.grad[i, :lens[i]].cpu(), xi.grad[0].cpu())
            assert float(xi.grad.abs().max()) > 0
            if lens[i] < x.shape[1]:
                assert float(x.grad[i, lens[i]:].abs().max()) == 0.0
    assert torch.equal(torch.get_rng_state(), state)
    record("varlen_mel_train.e2e[fp32]", **fig)
    print("varlen_mel_train.e2e[fp32]", fig)
    assert all(v < 1e-3 for v in fig.values()), fig

"""GPU tests of the ragged-batch eval forward: packed ("varlen") attention, patch embedding, front end and the model on top.

Contract: for clips of valid lengths len_i, row i of every output equals -- within the project's existing parity bounds -- what the
same module returns for clip i alone, cropped to len_i, at batch size 1 in eval mode; input beyond len_i has no influence (the tests
fill it with NaN).  Reference values: tests/golden/varlen_eval.npz (the real reference run one clip at a time,
tests/golden/make_varlen_golden.py).
"""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from passt_amd import ops  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32, PasstAmdError  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_golden as V  # noqa: E402
from tests.test_gpu_kernels import TD, _attn_inputs, _attn_ref, rel_err, rnd, tol  # noqa: E402
from tests.test_gpu_model import BF16_LOGITS, build, record, rel  # noqa: E402

DEV = "cuda"
RAGGED = [474, 3, 14, 127, 128, 129, 1190, 35]


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)


def _lse_rows(lse, H, total, lo, hi):
    """(H, n) view of the packed all-queries lse [H][total] for token rows lo..hi."""
    return lse.view(H, total)[:, lo:hi]


# ---- 1. attention kernel vs fp64, per sequence --------------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("lens", [RAGGED, [300]], ids=["ragged", "single"])
def test_attention_varlen_vs_fp64(lens, H, full, dt, pre):
    D, B, total, scale = H * 64, len(lens), sum(lens), 0.125
    x = rnd(total, 3 * D, seed=23, scale=1.5)
    qkv, qref = _attn_inputs(x, dt, D, pre)
    nq = None if full else 2
    o, lse = ops.attention_fwd_varlen(qkv, _cu(lens), B, H, max(lens), scale, nq=nq, flags=pre)
    torch.cuda.synchronize()
    worst_o = worst_l = 0.0
    off = 0
    for b, n in enumerate(lens):
        ro, rlse, _ = _attn_ref(qref[off:off + n], 1, H, n, scale)
        if full:
            got_o, got_l = o[off:off + n], _lse_rows(lse, H, total, off, off + n)
        else:
            ro, rlse = ro[:2], rlse[:, :, :2]
            got_o, got_l = o[2 * b:2 * b + 2], lse.view(B, H, 2)[b]
        worst_o = max(worst_o, rel_err(got_o, ro))
        worst_l = max(worst_l, float((got_l.double().cpu() - rlse[0]).abs().max()))
        off += n
    record(f"varlen_attention[{dt},B{B},H{H},{'full' if full else 'nq2'},pre{pre}]", o=worst_o, lse=worst_l)
    assert worst_o < tol(dt, 2e-5, 1.5e-2), worst_o
    assert worst_l < tol(dt, 2e-5, 2e-2), worst_l


# ---- 2. equal lengths reproduce the fixed-length kernel bit for bit -------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("B,H,N", [(8, 12, 474), (3, 2, 130)])
@pytest.mark.parametrize("full", [True, False])
def test_attention_varlen_equal_lengths_bitwise(B, H, N, dt, full):
    D, scale = H * 64, 0.125
    qkv, _ = _attn_inputs(rnd(B * N, 3 * D, seed=29, scale=1.5), dt, D, 1)
    nq = None if full else 2
    o0, l0 = ops.attention_fwd(qkv, B, H, N, scale, nq=nq, flags=ops.ATTN_Q_PRESCALED)
    o1, l1 = ops.attention_fwd_varlen(qkv, _cu([N] * B), B, H, N, scale, nq=nq, flags=ops.ATTN_Q_PRESCALED)
    torch.cuda.synchronize()
    assert torch.equal(o0, o1)
    if full:        # fixed: lse[(b*H + h)*N + q]; packed: lse[h][b*N + q]
        assert torch.equal(l0.view(B, H, N).permute(1, 0, 2).reshape(H, B * N), l1)
    else:
        assert torch.equal(l0, l1)


# ---- 3. neighbours do not leak -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("full", [True, False])
def test_attention_varlen_neighbours_do_not_leak(dt, full):
    lens, H, scale = RAGGED, 2, 0.125
    D, B, total = H * 64, len(lens), sum(lens)
    clean, _ = _attn_inputs(rnd(total, 3 * D, seed=23, scale=1.5), dt, D, 1)
    other, _ = _attn_inputs(rnd(total, 3 * D, seed=57, scale=1.5) * 1e3, dt, D, 1)
    cu, nq = _cu(lens), (None if full else 2)
    o0, l0 = ops.attention_fwd_varlen(clean, cu, B, H, max(lens), scale, nq=nq, flags=ops.ATTN_Q_PRESCALED)
    off = 0
    for b, n in enumerate(lens):
        dirty = other.clone()
        dirty[off:off + n] = clean[off:off + n]
        o1, l1 = ops.attention_fwd_varlen(dirty, cu, B, H, max(lens), scale, nq=nq, flags=ops.ATTN_Q_PRESCALED)
        torch.cuda.synchronize()
        if full:
            assert torch.equal(o0[off:off + n], o1[off:off + n]), b
            assert torch.equal(_lse_rows(l0, H, total, off, off + n), _lse_rows(l1, H, total, off, off + n)), b
        else:
            assert torch.equal(o0[2 * b:2 * b + 2], o1[2 * b:2 * b + 2]), b
            assert torch.equal(l0.view(B, H, 2)[b], l1.view(B, H, 2)[b]), b
        off += n


def test_attention_varlen_argument_checks():
    qkv = torch.zeros(40, 3 * 128, device=DEV)
    with pytest.raises(PasstAmdError):
        ops.attention_fwd_varlen(qkv, _cu([20, 20, 1])[:3], 3, 2, 20, 0.125)          # cu_tok needs B + 1 entries
    with pytest.raises(PasstAmdError):
        ops.attention_fwd_varlen(qkv, _cu([20, 20]), 2, 2, 41, 0.125)                 # max_N beyond the packed rows
    with pytest.raises(PasstAmdError):
        ops.attention_fwd_varlen(qkv, _cu([20, 20]).long(), 2, 2, 20, 0.125)          # int32 on the device


# ---- patch kernels against a host restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
def test_patch_kernels_varlen(dt):
    from passt_amd.passt import varlen_geometry
    lens, F, P, s, D, Tpe = [60, 16, 47], 48, 16, 10, 64, 4
    Fd = (F - P) // s + 1
    g = varlen_geometry(lens, P, s, Fd, Tpe)
    x = rnd(len(lens), 1, F, max(lens), seed=3)
    for i, n in enumerate(lens):
        x[i, :, :, n:] = float("nan")
    dev = lambda a: torch.from_numpy(a).to(DEV)
    cols = ops.patch_gather_varlen(x.to(DEV), dev(g["row_clip"]), dev(g["row_f"]), dev(g["row_t"]), P, s, s, dt).float().cpu()
    bias, tpos, fpos = rnd(D, seed=4), rnd(1, D, 1, Tpe, seed=5), rnd(1, D, Fd, 1, seed=6)
    cls, dist, npe = rnd(1, 1, D, seed=7), rnd(1, 1, D, seed=8), rnd(1, 2, D, seed=9)
    table = ops.patch_pos_table_varlen(bias.to(DEV), tpos.to(DEV), fpos.to(DEV), dev(g["row_f"]), dev(g["row_t"]), cls.to(DEV),
                                       dist.to(DEV), npe.to(DEV)).cpu()
    assert cols.shape == (g["row_f"].size, P * P) and torch.isfinite(cols).all()
    for r in range(g["row_f"].size):
        c, f, t = int(g["row_clip"][r]), int(g["row_f"][r]), int(g["row_t"][r])
        if f < 0:
            assert not cols[r].any()
            want = (cls if t == 0 else dist).view(D) + npe[0, t]
        else:
            assert torch.equal(cols[r], x[c, 0, f * s:f * s + P, t * s:t * s + P].reshape(-1).to(TD[dt]).float()), r
            want = bias + tpos[0, :, 0, t] + fpos[0, :, f, 0]
        assert torch.allclose(table[r], want, rtol=0, atol=1e-6), r


# ---- 4. front end -------------------------------------------------------------------------------------------------------------------
def _waves():
    w = torch.from_numpy(V.wave_input())
    for i, n in enumerate(V.WAVE_LENGTHS):
        w[i, n:] = float("nan")
    return w.to(DEV)


def test_frontend_varlen(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "varlen_eval.npz")))
    mel = passt_amd.AugmentMelSTFT(**V.MEL_KW).to(DEV).eval()
    w = _waves()
    spec, frames = mel(w, lengths=V.WAVE_LENGTHS)
    torch.cuda.synchronize()
    lib = passt_amd._lib.load()
    assert frames.dtype == torch.int64 and not frames.is_cuda
    assert frames.tolist() == [lib.pa_mel_num_frames(n, 320) for n in V.WAVE_LENGTHS] == gold["mel.frames"].tolist()
    assert spec.shape == (len(V.WAVE_LENGTHS), 128, max(frames.tolist()))
    worst_ref = worst_self = 0.0
    for i, (n, fr) in enumerate(zip(V.WAVE_LENGTHS, frames.tolist())):
        got = spec[i, :, :fr].cpu()
        assert torch.isfinite(got).all(), i
        assert (spec[i, :, fr:] == 0.0).all(), i                                      # exactly 0.0 behind the clip's end
        e_ref = float(np.abs(G.pin_sample(got.numpy(), V.MEL_SAMPLE) - gold[f"mel.{i}"]).max())
        alone = mel(w[i:i + 1, :n].contiguous())[0].cpu()
        e_self = float((got - alone).abs().max())
        worst_ref, worst_self = max(worst_ref, e_ref), max(worst_self, e_self)
        assert e_ref < 1e-3 and e_self < 1e-3, (i, e_ref, e_self)
    record("varlen_frontend", vs_reference=worst_ref, vs_single=worst_self)
    # a tensor of lengths (device or host) is the same call
    spec2, frames2 = mel(w, lengths=torch.tensor(V.WAVE_LENGTHS, device=DEV))
    assert torch.equal(spec, spec2) and torch.equal(frames, frames2)
    with pytest.raises(NotImplementedError):
        mel.train()(w, lengths=V.WAVE_LENGTHS)
    mel.eval()
    with pytest.raises(PasstAmdError, match="clip 1"):
        mel(w, lengths=[320000, 513, 41234, 5120, 640, 320000])                       # len - 1 <= n_fft / 2
    with pytest.raises(ValueError):
        mel(w, lengths=V.WAVE_LENGTHS[:-1])


# ---- 5. / 6. model vs the reference fixture and vs itself ----------------------------------------------------------------------------
def _model_input(case):
    x = torch.from_numpy(V.model_input(case))
    for i, n in enumerate(V.LENGTHS):
        x[i, :, :, n:] = float("nan")
    return x.to(DEV)


def _packed(m, x, lengths):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return m(x, lengths=lengths)


def _single(m, x, i, n):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        lo, fe = m(x[i:i + 1, :, :, :n].contiguous())
    return lo[0], fe[0]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(V.MODELS))
def test_model_varlen_vs_reference_and_single(golden_dir, name, precision):
    gold = dict(np.load(os.path.join(golden_dir, "varlen_eval.npz")))
    case = V.MODELS[name]
    m = build(case, precision).eval()
    x = _model_input(case)
    lim = 1e-3 if precision == "fp32" else BF16_LOGITS
    logits, feat = _packed(m, x, V.LENGTHS)
    torch.cuda.synchronize()
    assert logits.shape == (len(V.LENGTHS), case["cfg"]["num_classes"]) and feat.shape == (len(V.LENGTHS), case["cfg"]["embed_dim"])
    assert logits.grad_fn is None and feat.grad_fn is None and not logits.requires_grad
    assert torch.isfinite(logits).all() and torch.isfinite(feat).all()
    worst = dict(logits=0.0, features=0.0, logits_vs_single=0.0, features_vs_single=0.0)
    for i, n in enumerate(V.LENGTHS):
        e_l, e_f = rel(logits[i].cpu(), gold[name + ".logits"][i]), rel(feat[i].cpu(), gold[name + ".features"][i])
        lo1, fe1 = _single(m, x, i, n)
        s_l, s_f = rel(logits[i].cpu(), lo1.cpu()), rel(feat[i].cpu(), fe1.cpu())
        print(f"{name}[{precision}] clip {i} len {n}: vs reference {e_l:.3e} {e_f:.3e}  vs single {s_l:.3e} {s_f:.3e}")
        for k, v in zip(worst, (e_l, e_f, s_l, s_f)):
            worst[k] = max(worst[k], v)
    record(f"varlen_eval[{precision}]" if name == "d768" else f"varlen_eval_{name}[{precision}]", **worst)
    assert all(v < lim for v in worst.values()), worst


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_varlen_all_full_length_equals_plain_forward(precision):
    case = V.MODELS["small"]
    m = build(case, precision).eval()
    x = torch.from_numpy(V.model_input(case))[:3, :, :, :998].contiguous().to(DEV)
    lim = 1e-3 if precision == "fp32" else BF16_LOGITS
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        l0, f0 = m(x)
    l1, f1 = _packed(m, x, [998] * 3)
    assert rel(l1.cpu(), l0.cpu()) < lim and rel(f1.cpu(), f0.cpu()) < lim
    la, fa = _packed(m, x[:1], [998])                                                 # B = 1 is legal
    assert rel(la.cpu(), l0[:1].cpu()) < lim and rel(fa.cpu(), f0[:1].cpu()) < lim


# ---- 7. order and batch independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_varlen_order_and_split(precision):
    """The attention work-item map is one grid over (sequence, head, block) that does not look at the order of the clips, and every
    other kernel works row by row on the same number of rows: permuting the clips permutes the outputs bit for bit."""
    case = V.MODELS["small"]
    m = build(case, precision).eval()
    x = _model_input(case)
    logits, feat = _packed(m, x, V.LENGTHS)
    perm = [6, 3, 0, 7, 2, 5, 1, 4]
    lp, fp = _packed(m, x[perm].contiguous(), [V.LENGTHS[i] for i in perm])
    assert torch.equal(lp, logits[perm]) and torch.equal(fp, feat[perm])
    la, fa = _packed(m, x[:3].contiguous(), V.LENGTHS[:3])
    lb, fb = _packed(m, x[3:].contiguous(), V.LENGTHS[3:])
    lim = 1e-3 if precision == "fp32" else BF16_LOGITS
    assert rel(torch.cat([la, lb]).cpu(), logits.cpu()) < lim and rel(torch.cat([fa, fb]).cpu(), feat.cpu()) < lim


# ---- 8. contract --------------------------------------------------------------------------------------------------------------------
def test_model_varlen_contract():
    case = V.MODELS["small"]
    m = build(case, "fp32").eval()
    x = _model_input(case)
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        xf = torch.from_numpy(V.model_input(case))[:2, :, :, :998].contiguous().to(DEV)
        l0, f0 = m(xf)
        _packed(m, x, V.LENGTHS)                      # shares the staged weights / scratch caches
        l1, f1 = m(xf)
    assert torch.equal(l0, l1) and torch.equal(f0, f1)
    m.train()
    with pytest.raises(NotImplementedError, match="ragged"):
        m(x, lengths=V.LENGTHS)
    m.eval()
    with pytest.raises(ValueError, match="clip 3"):
        m(x, lengths=[998, 437, 1203, 15, 251, 640, 998, 33])
    with pytest.raises(ValueError):
        m(x, lengths=V.LENGTHS[:-1])
    with pytest.raises(ValueError, match="clip 2"):
        m(x, lengths=[998, 437, 1204, 16, 251, 640, 998, 33])                         # longer than x
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        m(x, lengths=V.LENGTHS)
    assert len([i for i in w if "will be cut" in str(i.message)]) == 1
    # lengths as a tensor, host or device
    a = m(x, lengths=torch.tensor(V.LENGTHS))
    b = m(x, lengths=torch.tensor(V.LENGTHS, device=DEV, dtype=torch.int32))
    c = _packed(m, x, V.LENGTHS)
    assert torch.equal(a[0], c[0]) and torch.equal(b[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(b[1], c[1])
    # inside autocast = the bf16 path
    m2, m3 = build(case, "bf16").eval(), build(case, None).eval()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        d = _packed(m3, x, V.LENGTHS)
    assert torch.equal(d[0], _packed(m2, x, V.LENGTHS)[0])
    # ensemble == mean of its members
    ens = passt_amd.passt.EnsembelerModel([m, build(dict(case, seed=77), "fp32").eval()]).eval()
    e, e2 = _packed(ens, x, V.LENGTHS)
    want = (_packed(ens.models[0], x, V.LENGTHS)[0] + _packed(ens.models[1], x, V.LENGTHS)[0]) / 2
    assert torch.equal(e, want) and e2 is e


# ---- 9. end to end: wave -> mel -> net ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_end_to_end_varlen(precision):
    case = V.MODELS["small"]
    m = build(case, precision).eval()
    mel = passt_amd.AugmentMelSTFT(**V.MEL_KW).to(DEV).eval()
    w = _waves()
    spec, frames = mel(w, lengths=V.WAVE_LENGTHS)
    with pytest.raises(ValueError, match="clip 4"):                                    # 640 samples = 2 frames: below one patch
        _packed(m, spec[:, None], frames)
    keep = [i for i, n in enumerate(V.WAVE_LENGTHS) if n != 640]
    lens = [V.WAVE_LENGTHS[i] for i in keep]
    spec, frames = mel(w[keep].contiguous(), lengths=lens)
    logits, feat = _packed(m, spec[:, None], frames)
    lim = 1e-3 if precision == "fp32" else BF16_LOGITS
    for j, n in enumerate(lens):
        s1 = mel(w[keep[j]:keep[j] + 1, :n].contiguous())
        lo1, fe1 = _single(m, s1[:, None], 0, s1.shape[-1])
        assert rel(logits[j].cpu(), lo1.cpu()) < lim and rel(feat[j].cpu(), fe1.cpu()) < lim, j

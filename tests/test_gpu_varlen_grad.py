"""GPU tests of the gradients through the ragged-batch forward (``net.varlen_grad = True``): the packed attention backward, the packed
patch stage, and the model on top.

Contract, the backward twin of tests/test_gpu_varlen.py's: for a loss that is a sum over clips, ``x.grad[i, ..., :lengths[i]]`` equals
what clip i alone gives at batch size 1, a parameter gradient equals the sum over clips of those batch-1 gradients, and whatever lies
behind ``lengths[i]`` in x is never read (the tests put NaN there).  Reference values: tests/golden/varlen_grad.npz (the real
reference run one clip at a time, tests/golden/make_varlen_grad_golden.py).  Errors in dx are taken per clip, relative to that clip's
own largest entry (the clips' max|dx| span 6e-3 .. 0.19).  Bounds are the project's own: tests.test_gpu_kernels.tol for the kernels, 1e-3
(fp32) and BF16_LOGITS / BF16_GRADS of tests/test_gpu_model.py for the model.
"""
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from passt_amd import _lib, ops  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32  # noqa: E402
from passt_amd.passt import varlen_geometry  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_grad_golden as VG  # noqa: E402
from tests.test_gpu_kernels import TD, _attn_inputs, _attn_ref, rel_err, rnd, tol  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, BF16_LOGITS, build, record, rel  # noqa: E402

DEV = "cuda"
RAGGED = [474, 3, 14, 127, 128, 129, 1190, 35]
PRE, TWO_PASS = ops.ATTN_Q_PRESCALED, ops.ATTN_BWD_TWO_PASS


def _cu(lens):
    return torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=DEV)


def _attn_case(lens, H, dt, pre, full, seed=23):
    """(qkv, fp64 view, o, lse, d_o, cu_tok) of a packed attention problem; o / lse from the packed forward."""
    D, B, total = H * 64, len(lens), sum(lens)
    qkv, qref = _attn_inputs(rnd(total, 3 * D, seed=seed, scale=1.5), dt, D, pre)
    cu = _cu(lens)
    o, lse = ops.attention_fwd_varlen(qkv, cu, B, H, max(lens), 0.125, nq=None if full else 2, flags=pre)
    d_o = rnd(o.shape[0], D, seed=seed + 1).to(TD[dt]).to(DEV)
    return qkv, qref, o, lse, d_o, cu


# ---- 1. packed attention backward vs fp64, per sequence ---------------------------------------------------------------------------
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("H", [2, 12])
@pytest.mark.parametrize("lens", [RAGGED, [300]], ids=["ragged", "single"])
def test_attention_bwd_varlen_vs_fp64(lens, H, full, dt, pre):
    D, B = H * 64, len(lens)
    qkv, qref, o, lse, d_o, cu = _attn_case(lens, H, dt, pre, full)
    dqkv = ops.attention_bwd_varlen(qkv, o, d_o, lse, cu, B, H, max(lens), 0.125, nq=None if full else 2, flags=pre)
    torch.cuda.synchronize()
    assert torch.isfinite(dqkv).all()
    worst = dict(dq=0.0, dk=0.0, dv=0.0)
    off = 0
    for b, n in enumerate(lens):
        if full:
            d_seq = d_o[off:off + n]
        else:                                           # the gradient enters at the first two queries only
            d_seq = torch.zeros(n, D, dtype=torch.float64)
            d_seq[:2] = d_o[2 * b:2 * b + 2].double().cpu()
        _, _, ref = _attn_ref(qref[off:off + n], 1, H, n, 0.125, d_seq)
        got = dqkv[off:off + n].double().cpu()
        if full:                                        # test_attention_fwd_bwd's rule: every third against its own largest entry
            for k, sl in zip(worst, (slice(0, D), slice(D, 2 * D), slice(2 * D, 3 * D))):
                worst[k] = max(worst[k], rel_err(got[:, sl], ref[:, sl]))
        else:                                           # test_attention_prefix_queries' rule: the whole dqkv; Q third zero behind nq
            worst["dq"] = max(worst["dq"], rel_err(got, ref))
            assert float(got[2:, :D].abs().max()) == 0.0 if n > 2 else True
        off += n
    record(f"varlen_attention_bwd[{dt},B{B},H{H},{'full' if full else 'nq2'},pre{pre}]", **worst)
    lim = tol(dt, 5e-5, 4e-2)
    assert all(v < lim for v in worst.values()), worst


# ---- 2. equal lengths reproduce the fixed-length kernel pair bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("B,H,N", [(8, 12, 474), (3, 2, 130)])
@pytest.mark.parametrize("full", [True, False])
def test_attention_bwd_varlen_equal_lengths_bitwise(B, H, N, dt, full):
    D, nq = H * 64, (None if full else 2)
    qkv, _ = _attn_inputs(rnd(B * N, 3 * D, seed=29, scale=1.5), dt, D, 1)
    o, lse = ops.attention_fwd(qkv, B, H, N, 0.125, nq=nq, flags=PRE)
    d_o = rnd(o.shape[0], D, seed=30).to(TD[dt]).to(DEV)
    want = ops.attention_bwd(qkv, o, d_o, lse, B, H, N, 0.125, nq=nq, flags=PRE | TWO_PASS)
    lse_p = lse.view(B, H, N).permute(1, 0, 2).reshape(H, B * N).contiguous() if full else lse
    got = ops.attention_bwd_varlen(qkv, o, d_o, lse_p, _cu([N] * B), B, H, N, 0.125, nq=nq, flags=PRE)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


# ---- 3. neighbours do not leak, nothing is written outside --------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("full", [True, False])
def test_attention_bwd_varlen_neighbours_do_not_leak(dt, full):
    lens, H = RAGGED, 2
    D, B, total = H * 64, len(lens), sum(lens)
    nq = None if full else 2
    qkv, _, o, lse, d_o, cu = _attn_case(lens, H, dt, 1, full)
    lib = _lib.load()
    need = lib.pa_attention_bwd_varlen_ws_floats(total, B, H, max(lens) if full else 2)
    assert need >= 2 * H * (total if full else 2 * B)
    guard = 64
    big = torch.full((total + guard, 3 * D), 7.0, device=DEV, dtype=TD[dt])
    ws = torch.full((need + guard,), 7.0, device=DEV)
    clean = ops.attention_bwd_varlen(qkv, o, d_o, lse, cu, B, H, max(lens), 0.125, nq=nq, flags=PRE, ws=ws, out=big[:total])
    torch.cuda.synchronize()
    assert clean.data_ptr() == big.data_ptr() and torch.isfinite(clean).all()
    assert (big[total:] == 7.0).all() and (ws[need:] == 7.0).all()
    clean = clean.clone()
    off = 0
    for b, n in enumerate(lens):
        q2, o2, d2 = (torch.full_like(t, float("nan")) for t in (qkv, o, d_o))
        q2[off:off + n] = qkv[off:off + n]
        rows = slice(off, off + n) if full else slice(2 * b, 2 * b + 2)
        o2[rows], d2[rows] = o[rows], d_o[rows]
        got = ops.attention_bwd_varlen(q2, o2, d2, lse, cu, B, H, max(lens), 0.125, nq=nq, flags=PRE)
        torch.cuda.synchronize()
        assert torch.equal(got[off:off + n], clean[off:off + n]), b
        off += n


def test_attention_bwd_varlen_argument_checks():
    lib = _lib.load()
    EINVAL, EUNSUPPORTED = -1, -2
    t = torch.zeros(40, 3 * 128, device=DEV)
    o, lse, ws, cu = torch.zeros(40, 128, device=DEV), torch.zeros(2, 40, device=DEV), torch.zeros(4096, device=DEV), _cu([20, 20])
    p = lambda x: x.data_ptr()
    call = lambda *a: lib.pa_attention_bwd_varlen(*a)
    good = [p(t), 384, p(o), p(o), 128, p(lse), p(ws), p(t), 384, p(cu), 2, 2, 20, 20, 0.125, PA_F32, 0, None]
    for i in (0, 2, 3, 5, 6, 7, 9):                     # every pointer
        bad = list(good)
        bad[i] = None
        assert call(*bad) == EINVAL, i
    for i, v in ((10, 0), (11, 0), (12, 0), (13, 0), (15, 7), (16, 64), (1, 380), (8, 128)):
        bad = list(good)
        bad[i] = v
        assert call(*bad) == EINVAL, i
    bad = list(good)
    bad[4] = 130                                        # rows of o not 16-byte aligned
    assert call(*bad) == EUNSUPPORTED
    assert lib.pa_attention_bwd_varlen_ws_floats(0, 2, 2, 2) == 0
    with pytest.raises(_lib.PasstAmdError):
        ops.attention_bwd_varlen(t, o, o, lse, _cu([20, 20, 1])[:2], 2, 2, 20, 0.125)        # cu_tok needs B + 1 entries
    with pytest.raises(_lib.PasstAmdError):
        ops.attention_bwd_varlen(t, o[:4], o[:4], lse, cu, 2, 2, 20, 0.125)                  # all queries need packed o / d_o
    with pytest.raises(_lib.PasstAmdError):
        ops.attention_bwd_varlen(t, o, o, lse, cu, 2, 2, 20, 0.125, ws=ws[:8])


# ---- 4. patch stage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("T_max", [130, 131])
@pytest.mark.parametrize("stride", [(10, 10), (16, 16), (10, 16)])
def test_patch_input_bwd_varlen_vs_torch_fold(stride, T_max, dt):
    """the packed fold against torch.nn.functional.fold per clip in float64; dx is pre-filled with NaN, so an element the kernel does
    not write fails.  One clip is cut by a short time embedding (Tpe = 9), one is exactly one patch column."""
    lens, F, P, Tpe = [T_max, 16, 47, 90, 33], 64, 16, 9
    fs, ts = stride
    Fg, B = (F - P) // fs + 1, len(lens)
    g = varlen_geometry(lens, P, ts, Fg, Tpe, T_max=T_max)
    M = g["row_f"].size
    gen = torch.Generator().manual_seed(100 * fs + ts + T_max)
    dcols = (torch.rand(M, P * P, generator=gen) * 2 - 1).to(TD[dt])
    cu = torch.from_numpy(g["cu_tok"]).to(DEV)
    dx = torch.full((B, 1, F, T_max), float("nan"), device=DEV)
    assert ops.patch_input_bwd_varlen(dcols.to(DEV), cu, B, F, T_max, P, fs, ts, out=dx) is dx
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
    worst = 0.0
    for b, n in enumerate(lens):
        Te, o = g["T_eff"][b], int(g["cu_tok"][b]) + 2
        end = (Te - 1) * ts + P                         # first frame no patch column of this clip covers
        assert end <= n
        full = dcols[o:o + Fg * Te].double().t().reshape(1, P * P, Fg * Te)
        ref = torch.nn.functional.fold(full, output_size=(F, end), kernel_size=P, stride=(fs, ts))[0, 0]
        got = dx[b, 0].double().cpu()
        worst = max(worst, float((got[:, :end] - ref).abs().max() / ref.abs().max()))
        assert float(got[:, end:].abs().max() if end < T_max else 0.0) == 0.0, b       # exactly zero behind the clip / the cut
        assert (got[:, :end][ref == 0] == 0).all(), b
    record(f"patch_input_bwd_varlen[{fs}x{ts},T{T_max},{'f32' if dt == PA_F32 else 'bf16'}]", err=worst)
    assert worst < tol(dt), worst
    dx2 = ops.patch_input_bwd_varlen(dcols.to(DEV), cu, B, F, T_max, P, fs, ts)
    assert dx2.shape == dx.shape and torch.equal(dx, dx2)


def test_patch_bwd_varlen_vs_index_add():
    lens, Fg, P, ts, Tpe, D = [130, 16, 47, 90, 33], 4, 16, 10, 9, 72
    g = varlen_geometry(lens, P, ts, Fg, Tpe)
    M, B = g["row_f"].size, len(lens)
    dtok = rnd(M, D, seed=5)
    rf, rt = torch.from_numpy(g["row_f"]).long(), torch.from_numpy(g["row_t"]).long()
    patch, d64 = rf >= 0, dtok.double()
    want = dict(bias=d64[patch].sum(0), cls=d64[(~patch) & (rt == 0)].sum(0), dist=d64[(~patch) & (rt == 1)].sum(0),
                tpos=torch.zeros(Tpe, D, dtype=torch.float64).index_add_(0, rt[patch], d64[patch]).t(),
                fpos=torch.zeros(Fg, D, dtype=torch.float64).index_add_(0, rf[patch], d64[patch]).t())
    want["npe"] = torch.stack([want["cls"], want["dist"]])

    def run(fill, accumulate=False):
        out = dict(cls=torch.full((1, 1, D), fill), dist=torch.full((1, 1, D), fill), npe=torch.full((1, 2, D), fill), bias=torch.full((D,), fill),
                   tpos=torch.full((1, D, 1, Tpe), fill), fpos=torch.full((1, D, Fg, 1), fill))
        out = {k: v.to(DEV) for k, v in out.items()}
        ops.patch_bwd_varlen(dtok.to(DEV), torch.from_numpy(g["cu_tok"]).to(DEV), B, Tpe, Fg, out["cls"], out["dist"], out["npe"], out["bias"],
                             out["tpos"], out["fpos"], accumulate=accumulate)
        torch.cuda.synchronize()
        return out
    a, b = run(float("nan")), run(3.0)
    for k, v in a.items():
        assert torch.isfinite(v).all() and torch.equal(v, b[k]), k                 # overwritten; repeated calls bit-identical
        e = rel_err(v.reshape(want[k].shape), want[k])
        assert e < 2e-5, (k, e)
    assert float(a["tpos"][0, :, 0, 8].abs().max()) > 0                            # the cut clip reaches the last time slot
    c = run(1.0, accumulate=True)
    for k, v in c.items():
        assert rel_err(v.reshape(want[k].shape), want[k] + 1.0) < 2e-5, k
    # frozen mode: every output NULL is a no-op, a partial set is refused
    lib = _lib.load()
    d, cu = dtok.to(DEV), torch.from_numpy(g["cu_tok"]).to(DEV)
    assert lib.pa_patch_bwd_varlen(d.data_ptr(), M, D, cu.data_ptr(), B, Tpe, Fg, None, None, None, None, None, None, 0, None) == 0
    assert lib.pa_patch_bwd_varlen(d.data_ptr(), M, D, cu.data_ptr(), B, Tpe, Fg, a["cls"].data_ptr(), None, None, None, None, None, 0, None) == -1
    assert lib.pa_patch_input_bwd_varlen(None, PA_F32, cu.data_ptr(), B, 16, 10, 10, 64, 130, None, None) == -1


# ---- 5. model against the reference fixture and against this library's own batch-1 backward ----------------------------------------
def _x(case):
    x, a, b = VG.inputs(case)
    x = torch.from_numpy(x)
    for i, n in enumerate(VG.LENGTHS):
        x[i, :, :, n:] = float("nan")
    return x.to(DEV), torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)


def _net(case, precision, trainable):
    m = build(case, precision).eval().requires_grad_(trainable)
    m.varlen_grad = True
    return m


def _packed_step(m, x, a, b, lengths):
    xg = x.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, feat = m(xg, lengths=lengths)
    VG.loss_of(logits, feat, a, b).backward()
    return logits.detach(), feat.detach(), xg.grad


def _single_steps(case, precision, trainable, x, a, b):
    """this library's fixed-length path, one cropped clip at a time: ([dx_i], [logits_i], [features_i], {parameter: summed gradient})"""
    m = build(case, precision).eval().requires_grad_(trainable)
    m.input_grad = True
    dxs, lo, fe = [], [], []
    for i, n in enumerate(VG.LENGTHS):
        xi = x[i:i + 1, :, :, :n].contiguous().requires_grad_()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            logits, feat = m(xi)
        VG.loss_of(logits, feat, a[i:i + 1], b[i:i + 1]).backward()
        dxs.append(xi.grad)
        lo.append(logits.detach()[0])
        fe.append(feat.detach()[0])
    return dxs, lo, fe, {n: p.grad for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("variant", list(VG.VARIANTS))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(VG.MODELS))
def test_model_varlen_grad_vs_reference_and_single(golden_dir, name, precision, variant):
    """Both models, both precisions, parameters frozen and trainable; every figure is printed per clip and recorded (record(...)).
    No MI355X figures yet: none could be taken when this was written."""
    gold = dict(np.load(os.path.join(golden_dir, "varlen_grad.npz")))
    fwd = dict(np.load(os.path.join(golden_dir, "varlen_eval.npz")))
    case, trainable = VG.MODELS[name], variant == "trainable"
    m = _net(case, precision, trainable)
    x, a, b = _x(case)
    logits, feat, dx = _packed_step(m, x, a, b, VG.LENGTHS)
    torch.cuda.synchronize()
    assert dx is not None and dx.shape == x.shape and dx.dtype == torch.float32 and torch.isfinite(dx).all()
    dxs, lo1, fe1, g1 = _single_steps(case, precision, trainable, x, a, b)
    P, ts, Tpe = case["cfg"]["patch"], case["cfg"]["stride"][1], case["cfg"]["grid"][1]
    w = dict(logits=0.0, features=0.0, logits_vs_single=0.0, features_vs_single=0.0, dx=0.0, dx_norm=0.0, dx_vs_single=0.0)
    for i, n in enumerate(VG.LENGTHS):
        key = f"{name}.{variant}.dx.{i}"
        nrm, scale = (float(v) for v in gold[key + ".stats"])
        got = dx[i:i + 1, :, :, :n].cpu().numpy()
        e = dict(logits=rel(logits[i].cpu(), fwd[name + ".logits"][i]), features=rel(feat[i].cpu(), fwd[name + ".features"][i]),
                 logits_vs_single=rel(logits[i].cpu(), lo1[i].cpu()), features_vs_single=rel(feat[i].cpu(), fe1[i].cpu()),
                 dx=float(np.abs(G.pin_sample(got, VG.DX_SAMPLE) - gold[key]).max()) / scale,
                 dx_norm=abs(float(np.linalg.norm(got.astype(np.float64))) - nrm) / nrm,
                 dx_vs_single=rel(got, dxs[i].cpu().numpy()))
        print(f"{name}[{precision},{variant}] clip {i} len {n}: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
        for k, v in e.items():
            w[k] = max(w[k], v)
        # exactly zero behind the clip's own last patch column (its end, the time cut)
        end = (min((n - P) // ts + 1, Tpe) - 1) * ts + P
        assert float(dx[i, :, :, end:].abs().max() if end < dx.shape[-1] else 0.0) == 0.0, i
        assert float(dx[i, :, :, :end].abs().max()) > 0, i
    params = dict(m.named_parameters())
    if trainable:
        for k in VG.param_grads(case["cfg"]):
            key = f"{name}.{variant}.grad.{k}"
            got = params[k].grad.cpu().numpy()
            w["grad." + k] = float(np.abs(G.pin_sample(got, VG.DX_SAMPLE) - gold[key]).max()) / float(gold[key + ".stats"][1])
        for k, p in params.items():
            if k.startswith("head_dist."):
                assert p.grad is None
            else:
                w["grad_vs_single"] = max(w.get("grad_vs_single", 0.0), rel(p.grad.cpu(), g1[k].cpu()))
    else:
        assert all(p.grad is None for p in params.values())
    record(f"varlen_grad.{name}[{precision},{variant}]", **w)
    print(f"varlen_grad.{name}[{precision},{variant}]", w)
    lim_out, lim_g = (1e-3, 1e-3) if precision == "fp32" else (BF16_LOGITS, BF16_GRADS)
    for k, v in w.items():
        assert v < (lim_out if k.startswith(("logits", "features")) else lim_g), (k, v, w)


# ---- 6. order and split -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_varlen_grad_order_and_split(precision):
    case = VG.MODELS["small"]
    x, a, b = _x(case)
    lim = 1e-3 if precision == "fp32" else BF16_GRADS
    m = _net(case, precision, False)
    _, _, dx = _packed_step(m, x, a, b, VG.LENGTHS)
    perm = [6, 3, 0, 7, 2, 5, 1, 4]
    _, _, dxp = _packed_step(m, x[perm].contiguous(), a[perm], b[perm], [VG.LENGTHS[i] for i in perm])
    assert torch.equal(dxp, dx[perm])                   # frozen network: bit for bit
    _, _, da = _packed_step(m, x[:3].contiguous(), a[:3], b[:3], VG.LENGTHS[:3])
    _, _, db = _packed_step(m, x[3:].contiguous(), a[3:], b[3:], VG.LENGTHS[3:])
    for i in range(len(VG.LENGTHS)):
        assert rel((da[i] if i < 3 else db[i - 3]).cpu(), dx[i].cpu()) < lim, i
    # parameter gradients: the summation order changes, so within the bound only
    mt = _net(case, precision, True)
    _packed_step(mt, x, a, b, VG.LENGTHS)
    g0 = {n: p.grad.clone() for n, p in mt.named_parameters() if p.grad is not None}
    mt.zero_grad()
    _packed_step(mt, x[perm].contiguous(), a[perm], b[perm], [VG.LENGTHS[i] for i in perm])
    g1 = {n: p.grad.clone() for n, p in mt.named_parameters() if p.grad is not None}
    mt.zero_grad()
    _packed_step(mt, x[:3].contiguous(), a[:3], b[:3], VG.LENGTHS[:3])
    _packed_step(mt, x[3:].contiguous(), a[3:], b[3:], VG.LENGTHS[3:])          # accumulates
    for n, p in mt.named_parameters():
        if n in g0:
            assert rel(g1[n].cpu(), g0[n].cpu()) < lim and rel(p.grad.cpu(), g0[n].cpu()) < lim, n


# ---- 7. contract ------------------------------------------------------------------------------------------------------------------
def test_model_varlen_grad_contract():
    case = VG.MODELS["small"]
    x, a, b = _x(case)
    m = build(case, "fp32").eval().requires_grad_(False)
    assert m.varlen_grad is False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo, fe = m(x.clone().requires_grad_(), lengths=VG.LENGTHS)
        assert lo.grad_fn is None and fe.grad_fn is None                # the default stays: no graph
        m.varlen_grad = True
        lo0, fe0, dx0 = _packed_step(m, x, a, b, VG.LENGTHS)
        assert torch.equal(lo, lo0) and torch.equal(fe, fe0)            # the same launch sequence in front of the outputs
        # exactly 0 and finite behind every clip's length although x is NaN there
        assert torch.isfinite(dx0).all()
        for i, n in enumerate(VG.LENGTHS):
            assert float(dx0[i, :, :, n:].abs().max() if n < x.shape[-1] else 0.0) == 0.0
        # a 16-bit leaf and a sliced (non-contiguous) one: the gradient comes back in the caller's shape / dtype / layout
        xh = x.bfloat16().requires_grad_()
        lo, fe = m(xh, lengths=VG.LENGTHS)
        VG.loss_of(lo, fe, a, b).backward()
        assert xh.grad.dtype == torch.bfloat16 and xh.grad.shape == xh.shape and torch.isfinite(xh.grad).all()
        base = torch.full((x.shape[0], 1, x.shape[2], x.shape[3] + 57), float("nan"), device=DEV)
        base[..., 30:30 + x.shape[3]] = x
        base.requires_grad_()
        xs = base[..., 30:30 + x.shape[3]]
        assert not xs.is_contiguous()
        lo, fe = m(xs, lengths=VG.LENGTHS)
        VG.loss_of(lo, fe, a, b).backward()
        assert base.grad.shape == base.shape and torch.equal(base.grad[..., 30:30 + x.shape[3]], dx0)
        assert float(base.grad[..., :30].abs().max()) == 0 and float(base.grad[..., 30 + x.shape[3]:].abs().max()) == 0
        # no_grad: nothing recorded, nothing saved
        with torch.no_grad():
            lo, fe = m(x.clone().requires_grad_(), lengths=VG.LENGTHS)
        assert lo.grad_fn is None and fe.grad_fn is None and torch.equal(lo, lo0)
        from passt_amd.passt import passt_forward_varlen
        assert len(passt_forward_varlen(m, x, VG.LENGTHS)) == 2
        out = passt_forward_varlen(m, x, VG.LENGTHS, save=True)
        assert len(out) == 3 and len(out[2]["saved"]) == len(m.blocks)
        # nothing requires a gradient: the plain path
        lo, fe = m(x, lengths=VG.LENGTHS)
        assert lo.grad_fn is None
        # a second backward on the same graph
        xg = x.clone().requires_grad_()
        lo, fe = m(xg, lengths=VG.LENGTHS)
        VG.loss_of(lo, fe, a, b).backward()
        with pytest.raises(RuntimeError, match="already consumed"):
            VG.loss_of(lo, fe, a, b).backward()
        # training mode keeps raising
        m.train()
        with pytest.raises(NotImplementedError, match="ragged"):
            m(x, lengths=VG.LENGTHS)
        m.eval()
        # an ensemble propagates gradients when its members opt in
        m2 = _net(dict(case, seed=77), "fp32", False)
        ens = passt_amd.passt.EnsembelerModel([m, m2]).eval()
        xg = x.clone().requires_grad_()
        e, _ = ens(xg, lengths=VG.LENGTHS)
        (e * a).sum().backward()
        assert e.grad_fn is not None and xg.grad is not None and float(xg.grad.abs().max()) > 0


def test_bound_optimizer_takes_packed_steps():
    """passt_amd.optim.AdamW binds the model to one flat gradient buffer inside its first step; the second packed step then runs the
    token route.  Parameters after both steps equal the unbound (per-parameter) model's within 2e-6."""
    from passt_amd import optim as pa_optim
    case = VG.MODELS["small"]
    x, a, b = _x(case)

    def run(flat):
        if not flat:
            os.environ["PASST_AMD_NO_FLAT_GRADS"] = "1"
        try:
            net = _net(case, "fp32", True)
            opt = pa_optim.AdamW(net.parameters(), lr=1e-4)
            for _ in range(2):
                opt.zero_grad()
                _packed_step(net, x, a, b, VG.LENGTHS)
                opt.step()
            torch.cuda.synchronize()
            return net
        finally:
            os.environ.pop("PASST_AMD_NO_FLAT_GRADS", None)
    net_u, net_b = run(False), run(True)
    assert net_u._flat is None and net_b._flat is not None
    for (n, pu), (_, pb) in zip(net_u.named_parameters(), net_b.named_parameters()):
        assert float((pu - pb).abs().max()) <= 2e-6, n


# ---- 8. frozen network: no weight-gradient work -----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frozen_network_runs_no_weight_gradient_on_the_packed_path(precision, monkeypatch):
    from tests.test_gpu_input_grad import _Count
    case = VG.MODELS["small"]
    x, a, b = _x(case)
    m = _net(case, precision, False)
    xg = x.clone().requires_grad_()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lo, fe = m(xg, lengths=VG.LENGTHS)
    assert lo.grad_fn is not None and fe.grad_fn is not None
    count = _Count(monkeypatch)
    calls = []
    monkeypatch.setattr(ops, "patch_bwd_varlen", lambda *a_, **k: calls.append(1))
    unflatten = torch._C._nn.unflatten_dense_tensors
    monkeypatch.setattr(torch._C._nn, "unflatten_dense_tensors", lambda *a_, **k: calls.append(2) or unflatten(*a_, **k))
    VG.loss_of(lo, fe, a, b).backward()
    assert count.n == {} and calls == [], (count.n, calls)      # no weight-gradient GEMM, no parameter reduction, no flat buffer
    assert all(p.grad is None for p in m.parameters()) and xg.grad is not None
    monkeypatch.undo()
    count = _Count(monkeypatch)
    m.requires_grad_(True)
    _packed_step(m, x, a, b, VG.LENGTHS)
    assert sum(count.n.values()) > 0                            # the counter sees what it is meant to see


# ---- 9. the use case --------------------------------------------------------------------------------------------------------------
def test_gradient_descent_on_a_ragged_batch_lowers_a_feature_matching_loss():
    """The ragged twin of test_gradient_descent_on_the_input_lowers_a_feature_matching_loss: ten steps of plain gradient descent on a
    ragged batch of spectrograms toward the other clips' feature vectors, step = a tenth of loss / |grad|^2: every step lowers the loss."""
    case = VG.MODELS["small"]
    x, _, _ = _x(case)
    m = _net(case, "fp32", False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            target = m(x, lengths=VG.LENGTHS)[1].flip(0)
        xg = x.clone().requires_grad_()
        losses = []
        for _ in range(11):
            xg.grad = None
            loss = ((m(xg, lengths=VG.LENGTHS)[1] - target) ** 2).sum()
            loss.backward()
            losses.append(float(loss.detach()))
            with torch.no_grad():
                step = 0.1 * loss / (xg.grad ** 2).sum() * xg.grad
                xg -= torch.where(xg.grad == 0, torch.zeros_like(step), step)       # (NaN behind the clips stays where it is)
    record("varlen_grad.descent[fp32]", first=losses[0], last=losses[-1])
    print("descent losses", losses)
    assert all(b_ < a_ for a_, b_ in zip(losses, losses[1:])), losses

"""Per-kernel parity of libpasst_amd.so (through the C ABI) against plain torch fp32/fp64 references
of the same op.  Tolerances: PA_F32 path ~1e-5..1e-4 relative (exact-f32 MFMA, different summation
order); PA_BF16 path checked against a reference computed from the SAME bf16-rounded inputs, so only
f32-accumulation order and the final bf16 rounding (2^-8 relative) remain.

One max-over-max figure per call cannot see a dropped K element, a shifted bias group or a misattributed row: the GEMM family is
checked for those with exact integer operands in guarded buffers by tests/test_gpu_gemm_exact.py (cases: tests/gemm_cases.py), the
attention family with exact operand families, padded leading dimensions and per-element bounds by tests/test_gpu_attention_exact.py
(cases: tests/attention_cases.py).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import ops  # noqa: E402
from passt_amd._lib import (EPI_DGELU, EPI_GELU, EPI_PARTIAL, EPI_RESID, EPI_STORE, PA_BF16,  # noqa: E402
                            PA_F32)

DEV = "cuda"
TD = {PA_F32: torch.float32, PA_BF16: torch.bfloat16}
_METRICS = {}


def record(name, **kw):
    _METRICS[name] = {k: float(v) for k, v in kw.items()}
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "kernel_parity_metrics.json"), "w") as f:
        json.dump(_METRICS, f, indent=1, sort_keys=True)


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def tol(dt, f32=2e-5, bf16=1.2e-2):
    return f32 if dt == PA_F32 else bf16


# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 136, 256), (474 * 2, 384, 128), (1000, 768, 768),
                                   (77, 3072, 192)])
def test_gemm_store_bias(dt, M, N, K):
    A = rnd(M, K, seed=1).to(TD[dt]).to(DEV)
    Bm = rnd(N, K, seed=2).to(TD[dt]).to(DEV)       # asymmetric random operands (transpose-detecting)
    bias = rnd(N, seed=3).to(DEV)
    out = torch.empty(M, N, device=DEV, dtype=TD[dt])
    ops.gemm_nt(A, Bm, dt, EPI_STORE, bias=bias, out_lp=out)
    ref = A.double().cpu() @ Bm.double().cpu().T + bias.double().cpu()
    e = rel_err(out, ref)
    record(f"gemm_store[{dt},{M},{N},{K}]", rel=e)
    assert e < tol(dt), e


@pytest.mark.parametrize("tune", [0, 1, 2, 3, 6, 7, 8, 9, 17, 18])
@pytest.mark.parametrize("M,N,K", [(1000, 768, 768), (300, 264, 128), (2 * 474, 2304, 256)])
def test_gemm_tile_variants(tune, M, N, K):
    """every workgroup-tile / pipeline variant of pa_gemm_nt (pa_gemm_args.tune) computes the same GEMM"""
    dt = PA_BF16
    A = rnd(M, K, seed=50).to(TD[dt]).to(DEV)
    Bm = rnd(N, K, seed=51).to(TD[dt]).to(DEV)
    bias = rnd(N, seed=52).to(DEV)
    resid = rnd(M, N, seed=53).to(DEV)
    ref = A.double().cpu() @ Bm.double().cpu().T + bias.double().cpu()
    old = ops.GEMM_TUNE
    try:
        ops.GEMM_TUNE = tune
        out = torch.empty(M, N, device=DEV, dtype=TD[dt])
        ops.gemm_nt(A, Bm, dt, EPI_STORE, bias=bias, out_lp=out)
        assert rel_err(out, ref) < tol(dt)
        out32 = torch.empty(M, N, device=DEV)
        ops.gemm_nt(A, Bm, dt, EPI_RESID, bias=bias, resid=resid, out_f32=out32)
        assert rel_err(out32, ref + resid.double().cpu()) < 3e-3
    finally:
        ops.GEMM_TUNE = old


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
def test_gemm_epilogues(dt):
    M, N, K = 300, 264, 128
    A = rnd(M, K, seed=4).to(TD[dt]).to(DEV)
    Bm = rnd(N, K, seed=5, scale=0.3).to(TD[dt]).to(DEV)
    bias = rnd(N, seed=6).to(DEV)
    acc = A.double().cpu() @ Bm.double().cpu().T
    # GELU: pre + exact-erf gelu of the stored pre
    pre = torch.empty(M, N, device=DEV, dtype=TD[dt])
    act = torch.empty(M, N, device=DEV, dtype=TD[dt])
    ops.gemm_nt(A, Bm, dt, EPI_GELU, bias=bias, out_lp=pre, out_lp2=act)
    ref_pre = acc + bias.double().cpu()
    assert rel_err(pre, ref_pre) < tol(dt)
    ref_act = torch.nn.functional.gelu(pre.double().cpu())
    e = rel_err(act, ref_act)
    record(f"gemm_gelu[{dt}]", rel=e)
    assert e < tol(dt, 2e-5, 6e-3)
    # RESID plain
    resid = rnd(M, N, seed=7).to(DEV)
    out = torch.empty(M, N, device=DEV)
    ops.gemm_nt(A, Bm, dt, EPI_RESID, bias=bias, resid=resid, out_f32=out)
    assert rel_err(out, ref_pre + resid.double().cpu()) < tol(dt, 2e-5, 3e-3)
    # RESID with the patch-embed row remap
    Np, Ntok, Bb = 100, 102, 3
    table = rnd(Np, N, seed=8).to(DEV)
    tok = torch.full((Bb, Ntok, N), 7.0, device=DEV)
    ops.gemm_nt(A, Bm, dt, EPI_RESID, resid=table, out_f32=tok, row_mod=Np, out_batch_rows=Ntok, out_row_off=2)
    ref_tok = torch.full((Bb, Ntok, N), 7.0, dtype=torch.float64)
    ref_tok[:, 2:, :] = (acc.view(Bb, Np, N) + table.double().cpu())
    assert rel_err(tok, ref_tok) < tol(dt, 2e-5, 3e-3)
    # DGELU
    aux = rnd(M, N, seed=9, scale=2.0).to(TD[dt]).to(DEV)
    dg = torch.empty(M, N, device=DEV, dtype=TD[dt])
    ops.gemm_nt(A, Bm, dt, EPI_DGELU, aux=aux, out_lp=dg)
    a64 = aux.double().cpu()
    gp = 0.5 * (1 + torch.erf(a64 / math.sqrt(2))) + a64 * torch.exp(-0.5 * a64 * a64) / math.sqrt(2 * math.pi)
    e = rel_err(dg, acc * gp)
    record(f"gemm_dgelu[{dt}]", rel=e)
    assert e < tol(dt, 3e-5, 1.2e-2)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
def test_wgrad_splitk_transpose_rowsum(dt):
    """dW = dY^T X through transposes + split-K partials + ordered reduce; db through rowsum."""
    M, N, K = 474 * 3 + 5, 384, 192
    dY = rnd(M, N, seed=10).to(TD[dt]).to(DEV)
    X = rnd(M, K, seed=11).to(TD[dt]).to(DEV)
    Mp = ops.round_up(M, ops.kpad(dt))
    dYt = ops.transpose(dY, dt, Mp)
    Xt = ops.transpose(X, dt, Mp)
    assert torch.equal(dYt[:, :M].float().cpu(), dY.float().cpu().T)
    assert float(dYt[:, M:].float().abs().max()) == 0.0
    dW = torch.full((N, K), 3.0, device=DEV)
    ops.wgrad(dYt, Xt, dW, dt, accumulate=False)
    ref = dY.double().cpu().T @ X.double().cpu()
    e = rel_err(dW, ref)
    record(f"wgrad[{dt}]", rel=e)
    assert e < tol(dt, 3e-5, 1e-4)   # bf16 x bf16 products are exact in f32; only f32 accumulation differs
    ops.wgrad(dYt, Xt, dW, dt, accumulate=True)
    assert rel_err(dW, 2 * ref) < 1e-4
    db = torch.empty(N, device=DEV)
    ops.rowsum(dYt, db, ncols=M)
    assert rel_err(db, dY.double().cpu().sum(0)) < 1e-4


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,N,K", [(474 * 3 + 5, 384, 192), (64, 128, 128), (2000, 768, 256), (333, 136, 3072),
                                   (30336 // 8, 2304, 768)])
def test_wgrad_tn_in_place_and_colsum(dt, M, N, K):
    """dW = dY^T X straight from the row-major operands (transpose-read MFMA fragments), ragged M/N tails."""
    dY = rnd(M, N, seed=40).to(TD[dt]).to(DEV)
    X = rnd(M, K, seed=41).to(TD[dt]).to(DEV)
    dW = torch.full((N, K), 3.0, device=DEV)
    ops.wgrad_tn(dY, X, dW, dt, accumulate=False)
    ref = dY.double().cpu().T @ X.double().cpu()
    e = rel_err(dW, ref)
    record(f"wgrad_tn[{dt},{M},{N},{K}]", rel=e)
    assert e < tol(dt, 3e-5, 1e-4), e
    if dt == PA_BF16:        # the 128x128 kernel (tune=1) must agree with the default role-split 256x256 one
        old, ops.GEMM_TUNE = ops.GEMM_TUNE, 1
        try:
            dW1 = torch.empty((N, K), device=DEV)
            ops.wgrad_tn(dY, X, dW1, dt, accumulate=False)
        finally:
            ops.GEMM_TUNE = old
        assert rel_err(dW1, ref) < 1e-4
    ops.wgrad_tn(dY, X, dW, dt, accumulate=True)
    assert rel_err(dW, 2 * ref) < 1e-4
    db = torch.full((N,), 9.0, device=DEV)
    ops.colsum(dY, db)
    assert rel_err(db, dY.double().cpu().sum(0)) < 1e-4
    ops.colsum(dY, db, accumulate=True)
    assert rel_err(db, 2 * dY.double().cpu().sum(0)) < 1e-4


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", [(37, 128), (1000, 768), (130, 1024), (64, 192)])
def test_layernorm(dt, M, D):
    x = rnd(M, D, seed=12, scale=3.0).to(DEV) + 0.5
    g = (rnd(D, seed=13) * 0.3 + 1).to(DEV)
    b = rnd(D, seed=14).to(DEV)
    y, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-6, dt)
    xr = x.double().cpu().requires_grad_(True)
    gr, br = g.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-6)
    e = rel_err(y, ref.detach())
    assert e < tol(dt, 1e-5, 6e-3), e
    assert rel_err(mean, xr.detach().mean(1)) < 1e-5
    dy = rnd(M, D, seed=15).to(TD[dt]).to(DEV)
    dres = rnd(M, D, seed=16).to(DEV)
    ref.backward(dy.double().cpu())
    dg = torch.empty(D, device=DEV)
    db = torch.empty(D, device=DEV)
    dcol = torch.full((D,), 7.0, device=DEV)
    dx, dx_lp = ops.layernorm_bwd(dy, x, g, mean, rstd, dres, dg, db, True, dcolsum=dcol)
    assert rel_err(dcol, (xr.grad + dres.double().cpu()).sum(0)) < 2e-5
    e1 = rel_err(dx, xr.grad + dres.double().cpu())
    e2, e3 = rel_err(dg, gr.grad), rel_err(db, br.grad)
    record(f"layernorm[{dt},{M},{D}]", fwd=e, dx=e1, dgamma=e2, dbeta=e3)
    assert e1 < 2e-5 and e2 < 2e-5 and e3 < 2e-5, (e1, e2, e3)
    assert rel_err(dx_lp, dx) < tol(dt, 1e-7, 5e-3)


SL2 = 0.125 * 1.4426950408889634


def _attn_inputs(x, dt, D, pre):
    """qkv as the kernels get it and as the fp64 reference reads it.  pre: the q third holds q * scale * log2(e) rounded
    to dt (what the qkv GEMM writes, PA_ATTN_Q_PRESCALED); the reference sees exactly that rounded value divided back."""
    qkv = x.to(TD[dt])
    ref = qkv.double()
    if pre:
        qkv = qkv.clone()
        qkv[:, :D] = (x[:, :D] * SL2).to(TD[dt])
        ref = qkv.double()
        ref[:, :D] = ref[:, :D] / SL2
    return qkv.to(DEV), ref


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,N,K,ncs", [(300, 192, 128, 64), (474 * 2, 2304, 768, 768), (77, 128, 64, 128)])
def test_gemm_store_colscale(dt, M, N, K, ncs):
    """PA_EPI_STORE with colscale_n / colscale: (acc + bias) * c on the first ncs columns, one rounding (the qkv Linear
    writes q * scale * log2(e) for PA_ATTN_Q_PRESCALED); the other columns are bit-identical to the plain store."""
    A = rnd(M, K, seed=4).to(TD[dt]).to(DEV)
    Bm = rnd(N, K, seed=5).to(TD[dt]).to(DEV)
    bias = rnd(N, seed=6).to(DEV)
    out = torch.empty(M, N, device=DEV, dtype=TD[dt])
    plain = torch.empty(M, N, device=DEV, dtype=TD[dt])
    ops.gemm_nt(A, Bm, dt, EPI_STORE, bias=bias, out_lp=out, colscale_n=ncs, colscale=SL2)
    ops.gemm_nt(A, Bm, dt, EPI_STORE, bias=bias, out_lp=plain)
    ref = A.double().cpu() @ Bm.double().cpu().T + bias.double().cpu()
    ref[:, :ncs] *= SL2
    assert rel_err(out[:, :ncs], ref[:, :ncs]) < tol(dt)
    assert torch.equal(out[:, ncs:], plain[:, ncs:])


@pytest.mark.parametrize("M,N,K,splits", [(4236, 768, 3072, 2), (4236, 768, 2304, 2), (24, 768, 3072, 8), (128, 768, 2304, 6),
                                          (200, 520, 2048, 5)])
def test_gemm_split_k_store_and_resid(M, N, K, splits):
    """pa_gemm_nt_splitk: the [M][768] problems of ESC-50 batch sizes and of the prefix-only tail are cut along K (partial
    tiles in a workspace + one finishing pass).  Same results as the one-pass kernel up to the order of the f32 partial sums,
    for both epilogues it covers, incl. the q-prescale columns, an edge tile and a strided output."""
    lib = ops._lib.load()
    assert lib.pa_gemm_nt_splitk_plan(M, N, K, EPI_STORE, PA_BF16) == splits
    A = rnd(M, K, seed=4).bfloat16().to(DEV)
    Bm = rnd(N, K, seed=5).bfloat16().to(DEV)
    bias = rnd(N, seed=6).to(DEV)
    resid = rnd(M, N, seed=7).to(DEV)
    ref = A.double().cpu() @ Bm.double().cpu().T + bias.double().cpu()
    ncs = 64 if N > 64 else 0
    out = torch.full((M, N + 8), 7.0, device=DEV, dtype=torch.bfloat16)
    ops.gemm_nt(A, Bm, PA_BF16, EPI_STORE, bias=bias, out_lp=out[:, :N], colscale_n=ncs, colscale=SL2)
    rs = ref.clone()
    rs[:, :ncs] *= SL2
    assert rel_err(out[:, :N], rs) < tol(PA_BF16)
    assert torch.all(out[:, N:] == 7.0)
    one = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    old, ops.GEMM_TUNE = ops.GEMM_TUNE, 8          # a forced variant never splits: the one-pass result
    try:
        ops.gemm_nt(A, Bm, PA_BF16, EPI_STORE, bias=bias, out_lp=one, colscale_n=ncs, colscale=SL2)
    finally:
        ops.GEMM_TUNE = old
    assert (out[:, :N].float() - one.float()).abs().max() <= 2.0 ** -7 * one.float().abs().max()
    o32 = torch.empty(M, N, device=DEV)
    ops.gemm_nt(A, Bm, PA_BF16, EPI_RESID, bias=bias, resid=resid, out_f32=o32)
    assert rel_err(o32, ref + resid.double().cpu()) < 1e-4          # f32 accumulation of bf16 products: no output rounding
    ops.gemm_nt(A, Bm, PA_BF16, EPI_RESID, bias=bias, resid=resid, out_f32=resid)      # in place on the residual stream
    assert torch.equal(resid, o32)


@pytest.mark.parametrize("M,N,K", [(64 * 474, 768, 768), (2000, 3072, 768), (1999, 2304, 256)])
def test_gemm_one_item_per_workgroup_is_bit_identical(M, N, K):
    """PA_GEMM_NO_PERSIST (what TrainStep sets when it all-reduces next to the backward): the role-split kernels launched
    with one work item per workgroup instead of 256 resident ones -- same items, same arithmetic, same bits, for every epilogue."""
    A = rnd(M, K, seed=41).bfloat16().to(DEV)
    Bm = rnd(N, K, seed=42).bfloat16().to(DEV)
    bias = rnd(N, seed=43).to(DEV)
    resid = rnd(M, N, seed=44).to(DEV)

    def run():
        o1 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        ops.gemm_nt(A, Bm, PA_BF16, EPI_STORE, bias=bias, out_lp=o1)
        o2 = torch.empty(M, N, device=DEV)
        ops.gemm_nt(A, Bm, PA_BF16, EPI_RESID, bias=bias, resid=resid, out_f32=o2)
        pre, act = torch.empty_like(o1), torch.empty_like(o1)
        ops.gemm_nt(A, Bm, PA_BF16, EPI_GELU, bias=bias, out_lp=pre, out_lp2=act)
        return o1, o2, pre, act

    base = run()
    old = ops.GEMM_RESERVED
    ops.GEMM_RESERVED = old | ops._lib.GEMM_NO_PERSIST
    try:
        other = run()
    finally:
        ops.GEMM_RESERVED = old
    for x, y in zip(base, other):
        assert torch.equal(x, y)
    assert rel_err(base[1], A.double().cpu() @ Bm.double().cpu().T + bias.double().cpu() + resid.double().cpu()) < 1e-4


@pytest.mark.parametrize("M,N,K", [(474 * 4, 2304, 768), (3792, 3072, 768), (333, 768, 3072), (77, 192, 128), (1000, 768, 768),
                                   (4236, 768, 2304), (130, 3072, 768)])
def test_gemm_epilogue_v3_equals_v2(M, N, K):
    """The LDS-free epilogues (round 4, opt-in PA_GEMM_EPILOGUE_V3: accumulators computed transposed -- lane = token row --,
    rows stored straight from the registers) against the default v2 epilogues (tile transposed through LDS): same products, same k order
    inside the MFMA, same epilogue arithmetic per element => BIT-identical outputs, for every fused epilogue, on interior
    and edge tiles (M not a multiple of 32, N below one tile).  Values are checked against fp64 once as well."""
    A = rnd(M, K, seed=21).to(torch.bfloat16).to(DEV)
    Bm = rnd(N, K, seed=22, scale=0.05).to(torch.bfloat16).to(DEV)
    bias = rnd(N, seed=23).to(DEV)
    resid = rnd(M, N, seed=24).to(DEV)
    dy = rnd(M, K, seed=25).to(torch.bfloat16).to(DEV)
    outs = {}
    for tag, fl in (("v3", ops._lib.GEMM_EPILOGUE_V3), ("v2", 0)):
        st = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        ops.gemm_nt(A, Bm, PA_BF16, ops.EPI_STORE, bias=bias, out_lp=st, flags=fl, colscale_n=min(N, 128) // 64 * 64, colscale=0.37)
        pre, act = torch.empty_like(st), torch.empty_like(st)
        ops.gemm_nt(A, Bm, PA_BF16, ops.EPI_GELU, bias=bias, out_lp=pre, out_lp2=act, flags=fl)
        dpre = torch.empty_like(st)
        ops.gemm_nt(dy, Bm, PA_BF16, ops.EPI_DGELU, aux=pre, out_lp=dpre, flags=fl)
        res = torch.empty(M, N, device=DEV, dtype=torch.float32)
        ops.gemm_nt(A, Bm, PA_BF16, ops.EPI_RESID, bias=bias, resid=resid, out_f32=res, flags=fl)
        torch.cuda.synchronize()
        outs[tag] = (st, pre, act, dpre, res)
    for name, a, b in zip(("store", "pre", "act", "dgelu", "resid"), outs["v3"], outs["v2"]):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    ref = A.double().cpu() @ Bm.double().cpu().T + bias.double().cpu()
    assert rel_err(outs["v3"][1], ref) < 1e-2
    assert rel_err(outs["v3"][2], torch.nn.functional.gelu(ref)) < 1e-2
    assert rel_err(outs["v3"][4], ref + resid.double().cpu()) < 1e-4


def _attn_ref(qkv, B, H, N, scale, d_o=None):
    D = H * 64
    t = qkv.double().cpu().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    q, k, v = t[0], t[1], t[2]
    att = ((q @ k.transpose(-2, -1)) * scale).softmax(-1)
    o = (att @ v).transpose(1, 2).reshape(B * N, D)
    lse = torch.logsumexp((q @ k.transpose(-2, -1)) * scale, -1)        # (B,H,N)
    dqkv = None
    if d_o is not None:
        o.backward(d_o.double().cpu())
        dqkv = t.grad.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * D)
    return o.detach(), lse.detach(), dqkv


# `pre`: 0 = plain, 1 = PA_ATTN_Q_PRESCALED (backward: the library's choice), 3 = pre-scaled + PA_ATTN_BWD_TWO_PASS (the dQ + dK/dV
# kernel pair), 5 = pre-scaled + PA_ATTN_BWD_SINGLE_PASS (the single-pass kernel: bf16, N <= 512; ignored elsewhere), 9 = pre-scaled +
# PA_ATTN_BWD_SINGLE_PASS_W16 (round 6: the single pass as sixteen waves of 32 keys)
@pytest.mark.parametrize("pre", [0, 1, 3, 5, 9])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("B,H,N", [(2, 2, 67), (1, 3, 474), (2, 12, 130), (1, 2, 1190), (3, 2, 64), (1, 1, 20),
                                   (1, 2, 512), (2, 1, 500), (1, 1, 33), (1, 2, 96), (2, 2, 353)])
def test_attention_fwd_bwd(dt, B, H, N, pre):
    D = H * 64
    x = rnd(B * N, 3 * D, seed=17, scale=1.5)
    # spike one key against one query so the online-softmax max jumps mid-sequence (guide rule 26)
    if N > 70:
        x[N - 3, 0:64] *= 4.0
        x[69, D:D + 64] = x[N - 3, 0:64]
    qkv, qref = _attn_inputs(x, dt, D, pre & 1)
    scale = 0.125
    o, lse = ops.attention_fwd(qkv, B, H, N, scale, flags=pre & 1)
    d_o = rnd(B * N, D, seed=18).to(TD[dt]).to(DEV)
    ro, rlse, rdqkv = _attn_ref(qref, B, H, N, scale, d_o)
    e_o = rel_err(o, ro)
    e_l = float((lse.double().cpu().view(B, H, N) - rlse).abs().max())
    assert e_o < tol(dt, 2e-5, 1.5e-2), e_o
    assert e_l < tol(dt, 2e-5, 2e-2), e_l
    dqkv = ops.attention_bwd(qkv, o, d_o, lse, B, H, N, scale, flags=pre)
    Dq = dqkv.double().cpu()
    e_q, e_k, e_v = (rel_err(Dq[:, :D], rdqkv[:, :D]), rel_err(Dq[:, D:2 * D], rdqkv[:, D:2 * D]),
                     rel_err(Dq[:, 2 * D:], rdqkv[:, 2 * D:]))
    record(f"attention[{dt},{B},{H},{N},pre{pre}]", o=e_o, lse=e_l, dq=e_q, dk=e_k, dv=e_v)
    lim = tol(dt, 5e-5, 4e-2)
    assert e_q < lim and e_k < lim and e_v < lim, (e_q, e_k, e_v)


@pytest.mark.parametrize("pre", [0, 1, 3, 5, 9])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("case", ["rising", "falling", "spikes", "large", "tiny"])
def test_attention_running_max_paths(dt, case, pre):
    """The forward keeps a lazy running max (the reference point of the exponentials only moves when a row would exceed
    2^6, attention.hip RESCALE_LOG2) and takes "score - reference" from the MFMA's C operand.  Inputs that force every
    branch of that logic (guide rule 26: bounded random data never takes them): the row max rising by far more than the
    threshold on every key tile, falling on every tile, isolated spikes in late tiles, uniformly large and uniformly
    tiny score ranges.  Checked against the fp64 softmax of the same inputs, forward and backward."""
    B, H, N = 2, 2, 300
    D = H * 64
    x = rnd(B * N, 3 * D, seed=91, scale=1.0)
    u = torch.ones(64) / 8.0                                     # unit vector; q.u = 8 => extra score = b_n (scale 1/8)
    n = torch.arange(N).repeat(B)
    if case in ("rising", "falling"):
        step = 12.0 if case == "rising" else -12.0
        for h in range(H):
            x[:, h * 64:(h + 1) * 64] += 8.0 * u
            x[:, D + h * 64:D + (h + 1) * 64] += (step * (n // 64).float())[:, None] * u
    elif case == "spikes":
        for (qi, ki, amp) in ((5, 200, 6.0), (37, 299, 9.0), (150, 130, 5.0), (299, 70, 7.0)):
            for b in range(B):
                x[b * N + qi, 0:64] = amp * u * 8.0
                x[b * N + ki, D:D + 64] = amp * u * 8.0
    elif case == "large":
        x[:, :2 * D] *= 5.0
    elif case == "tiny":
        x[:, :2 * D] *= 1e-3
    qkv, qref = _attn_inputs(x, dt, D, pre & 1)
    o, lse = ops.attention_fwd(qkv, B, H, N, 0.125, flags=pre & 1)
    d_o = rnd(B * N, D, seed=92).to(TD[dt]).to(DEV)
    ro, rlse, rdqkv = _attn_ref(qref, B, H, N, 0.125, d_o)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    e_o = rel_err(o, ro)
    e_l = float(((lse.double().cpu().view(B, H, N) - rlse).abs() / (1.0 + rlse.abs())).max())
    dqkv = ops.attention_bwd(qkv, o, d_o, lse, B, H, N, 0.125, flags=pre)
    assert torch.isfinite(dqkv.float()).all()
    Dq = dqkv.double().cpu()
    e_q, e_k, e_v = (rel_err(Dq[:, :D], rdqkv[:, :D]), rel_err(Dq[:, D:2 * D], rdqkv[:, D:2 * D]),
                     rel_err(Dq[:, 2 * D:], rdqkv[:, 2 * D:]))
    record(f"attention_runmax[{dt},{case},pre{pre}]", o=e_o, lse=e_l, dq=e_q, dk=e_k, dv=e_v)
    assert e_o < tol(dt, 2e-5, 2e-2), e_o
    assert e_l < tol(dt, 2e-5, 2e-2), e_l
    lim = tol(dt, 1e-4, 5e-2)
    assert e_q < lim and e_k < lim and e_v < lim, (e_q, e_k, e_v)


@pytest.mark.parametrize("pre", [1, 3, 5, 9])
@pytest.mark.parametrize("N", [3, 20, 45, 70])
def test_attention_bwd_strongly_negative_scores_with_keys_past_n(N, pre):
    """in the single-pass backward the key lanes past N inside a live 32-key block see a zero K row, i.e. the score
    exp2(-lse * log2 e); with every logit strongly negative (scores ~ -128: lse < -88) that is
    inf, and inf in the transposition buffer times the zero K rows of phase 2 would be NaN in dQ of valid queries.  Those lanes no
    longer write T.  Every backward form, against the fp64 reference, finite everywhere."""
    B, H = 2, 2
    D = H * 64
    # keys = 4 in every coordinate + noise, queries = -4 + noise: every score ~ (-64 * 16 +- 50) / 8 = -128 +- 6 (the noise keeps
    # dQ = sum_k dS[k] K[k], with sum_k dS[k] = 0, well conditioned against the bf16 rounding of dS)
    x = rnd(B * N, 3 * D, seed=77, scale=1.5)
    x[:, D:2 * D] += 4.0
    x[:, :D] -= 4.0
    qkv, qref = _attn_inputs(x, PA_BF16, D, 1)
    o, lse = ops.attention_fwd(qkv, B, H, N, 0.125, flags=1)
    assert float(lse.max()) < -100.0
    d_o = rnd(B * N, D, seed=78).to(torch.bfloat16).to(DEV)
    ro, rlse, rdqkv = _attn_ref(qref, B, H, N, 0.125, d_o)
    dqkv = ops.attention_bwd(qkv, o, d_o, lse, B, H, N, 0.125, flags=pre)
    assert torch.isfinite(dqkv.float()).all()
    Dq = dqkv.double().cpu()
    e_q, e_k, e_v = (rel_err(Dq[:, :D], rdqkv[:, :D]), rel_err(Dq[:, D:2 * D], rdqkv[:, D:2 * D]),
                     rel_err(Dq[:, 2 * D:], rdqkv[:, 2 * D:]))
    assert e_q < 5e-2 and e_k < 5e-2 and e_v < 5e-2, (e_q, e_k, e_v)


@pytest.mark.parametrize("pre", [0, 1, 3, 5, 9])
def test_attention_bit_deterministic_at_bench_shape(pre):
    """B = 64, H = 12, N = 474 (BASELINE config #2), bf16: four launches on the same input are bit-identical and finite, and
    eight sampled (clip, head) pairs of the full launch match the fp64 reference in value (forward and backward).  The
    kernels have no atomics, so any difference is a race; round 3 had one that only showed with every CU loaded (a register
    copy of an LDS fragment still in flight, tools/check_lds_asm.py) and passed every small-shape comparison."""
    B, H, N = 64, 12, 474
    D = H * 64
    g = torch.Generator(device=DEV).manual_seed(5)
    qkv = torch.randn(B * N, 3 * D, device=DEV, generator=g).to(torch.bfloat16)
    d_o = torch.randn(B * N, D, device=DEV, generator=g).to(torch.bfloat16)
    ref = None
    for _ in range(4):
        o, lse = ops.attention_fwd(qkv, B, H, N, 0.125, flags=pre & 1)
        dq = ops.attention_bwd(qkv, o, d_o, lse, B, H, N, 0.125, flags=pre)
        assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dq.float()).all()
        cur = (o.clone(), lse.clone(), dq.clone())
        if ref is None:
            ref = cur
        else:
            assert all(torch.equal(a, b) for a, b in zip(ref, cur))
    # VALUES at this size too (the race of round 3 passed every small-shape comparison and showed only with every CU
    # loaded): fp64 softmax attention, forward and backward, of sampled (clip, head) pairs spread over the launch -- first
    # and last workgroups, XCD boundaries of the head-major mapping -- against what the full-size launch produced for them
    o, lse, dq = ref
    worst = {}
    for b, h in ((0, 0), (0, 11), (17, 5), (31, 7), (40, 2), (63, 0), (63, 11), (22, 9)):
        rows = slice(b * N, (b + 1) * N)
        cols = [slice(j * D + h * 64, j * D + (h + 1) * 64) for j in range(3)]
        sub = torch.cat([qkv[rows, c] for c in cols], 1).double().cpu()                 # [N][q|k|v] of this head
        if pre:
            sub[:, :64] /= SL2
        ro, rlse, rdqkv = _attn_ref(sub, 1, 1, N, 0.125, d_o[rows, h * 64:(h + 1) * 64])
        errs = dict(o=rel_err(o[rows, h * 64:(h + 1) * 64], ro),
                    lse=float((lse.double().cpu().view(B, H, N)[b, h] - rlse.view(N)).abs().max()),
                    dq=rel_err(dq[rows, cols[0]], rdqkv[:, :64]), dk=rel_err(dq[rows, cols[1]], rdqkv[:, 64:128]),
                    dv=rel_err(dq[rows, cols[2]], rdqkv[:, 128:]))
        for k_, v_ in errs.items():
            worst[k_] = max(worst.get(k_, 0.0), v_)
        assert errs["o"] < 1.5e-2 and errs["lse"] < 2e-2 and max(errs["dq"], errs["dk"], errs["dv"]) < 4e-2, ((b, h), errs)
    record(f"attention_bench_shape_sampled[pre{pre}]", **worst)


def test_patch_ops_and_head():
    import torch.nn.functional as Fnn
    torch.manual_seed(3)
    B, F, T, D, P, fs, ts = 3, 128, 250, 128, 16, 10, 10
    Fd, Td, Tpe = 12, 24, 25
    x = rnd(B, 1, F, T, seed=19).to(DEV)
    pf = torch.tensor([0, 0, 3, 5, 11, 11], dtype=torch.int32, device=DEV)
    pt = torch.tensor([1, 7, 0, 23, 2, 22], dtype=torch.int32, device=DEV)
    Np = 6
    for dt in (PA_F32, PA_BF16):
        cols = ops.patch_gather(x, pf, pt, P, fs, ts, dt)
        unf = Fnn.unfold(x.cpu(), (P, P), stride=(fs, ts)).view(B, P * P, Fd, Td)
        ref = torch.stack([unf[:, :, int(f), int(t)] for f, t in zip(pf.cpu(), pt.cpu())], 1).reshape(B * Np, P * P)
        assert rel_err(cols, ref) < tol(dt, 1e-7, 4e-3)
    bias, tpe, fpe = rnd(D, seed=20).to(DEV), rnd(1, D, 1, Tpe, seed=21).to(DEV), rnd(1, D, Fd, 1, seed=22).to(DEV)
    cls, dist, npe = rnd(1, 1, D, seed=23).to(DEV), rnd(1, 1, D, seed=24).to(DEV), rnd(1, 2, D, seed=25).to(DEV)
    tok = torch.zeros(B, Np + 2, D, device=DEV)
    toff = 1
    table = ops.patch_pos_table(bias, tpe, fpe, pf, pt, toff, cls, dist, npe, tok)
    ref_t = torch.stack([bias.cpu() + tpe.cpu()[0, :, 0, toff + int(t)] + fpe.cpu()[0, :, int(f), 0]
                         for f, t in zip(pf.cpu(), pt.cpu())])
    assert rel_err(table, ref_t) < 1e-6
    assert rel_err(tok[:, 0], (cls + npe[:, :1]).cpu().expand(B, 1, D)[:, 0]) < 1e-6
    assert rel_err(tok[:, 1], (dist + npe[:, 1:]).cpu().expand(B, 1, D)[:, 0]) < 1e-6
    # backward reductions
    dtok = rnd(B, Np + 2, D, seed=26).to(DEV)
    g = {k: torch.full(s, 5.0, device=DEV) for k, s in dict(cls=(1, 1, D), dist=(1, 1, D), npe=(1, 2, D), b=(D,),
                                                            t=(1, D, 1, Tpe), f=(1, D, Fd, 1)).items()}
    dpatch = ops.patch_bwd(dtok, pf, pt, toff, Tpe, Fd, g["cls"], g["dist"], g["npe"], g["b"], g["t"], g["f"], PA_F32)
    dc = dtok.cpu().double()
    assert rel_err(g["cls"].view(-1), dc[:, 0].sum(0)) < 1e-5
    assert rel_err(g["npe"].view(2, D)[1], dc[:, 1].sum(0)) < 1e-5
    assert rel_err(g["b"], dc[:, 2:].sum((0, 1))) < 1e-5
    rt = torch.zeros(D, Tpe, dtype=torch.float64)
    rf = torch.zeros(D, Fd, dtype=torch.float64)
    for p_, (f, t) in enumerate(zip(pf.cpu(), pt.cpu())):
        rt[:, toff + int(t)] += dc[:, 2 + p_].sum(0)
        rf[:, int(f)] += dc[:, 2 + p_].sum(0)
    assert rel_err(g["t"].view(D, Tpe), rt) < 1e-5 and rel_err(g["f"].view(D, Fd), rf) < 1e-5
    assert rel_err(dpatch, dc[:, 2:].reshape(B * Np, D)) < 1e-6
    # head
    Ntok, C = 9, 37
    xx = rnd(B, Ntok, D, seed=27, scale=2.0).to(DEV)
    ng, nb = (rnd(D, seed=28) * 0.3 + 1).to(DEV), rnd(D, seed=29).to(DEV)
    hg, hb = (rnd(D, seed=30) * 0.3 + 1).to(DEV), rnd(D, seed=31).to(DEV)
    W, bb = rnd(C, D, seed=32, scale=0.2).to(DEV), rnd(C, seed=33).to(DEV)
    feat, hn, stats = ops.head_pre_fwd(xx, ng, nb, 1e-6, hg, hb, 1e-5)
    logits = ops.linear_f32_fwd(hn, W, bb)
    leaf = [t.double().cpu().requires_grad_(True) for t in (xx, ng, nb, hg, hb, W, bb)]
    xn = Fnn.layer_norm(leaf[0], (D,), leaf[1], leaf[2], 1e-6)
    rfeat = (xn[:, 0] + xn[:, 1]) / 2
    rlog = Fnn.linear(Fnn.layer_norm(rfeat, (D,), leaf[3], leaf[4], 1e-5), leaf[5], leaf[6])
    assert rel_err(feat, rfeat.detach()) < 1e-5 and rel_err(logits, rlog.detach()) < 1e-5
    y = (rnd(B, C, seed=34) > 0.7).float().to(DEV)
    loss, dlog = ops.bce_fwd_bwd(logits, y)
    rloss = Fnn.binary_cross_entropy_with_logits(rlog, y.double().cpu(), reduction="none").mean()
    dfeat_extra = rnd(B, D, seed=35).to(DEV)
    (rloss + (rfeat * dfeat_extra.double().cpu()).sum()).backward()
    assert abs(float(loss) - float(rloss.detach())) < 1e-6
    dW, dbb = torch.empty_like(W), torch.empty_like(bb)
    dhn = ops.linear_f32_bwd(dlog, hn, W, dW, dbb)
    dx, part = ops.head_pre_bwd(dhn, dfeat_extra, xx, feat, ng, hg, stats)
    assert rel_err(dW, leaf[5].grad) < 1e-5 and rel_err(dbb, leaf[6].grad) < 1e-5
    assert rel_err(dx, leaf[0].grad) < 2e-5
    sums = torch.empty(4, D, device=DEV)
    for j in range(4):
        ops.colsum_f32(part.view(B, 4, D)[:, j, :], sums[j])
    for j, idx in enumerate((3, 4, 1, 2)):
        assert rel_err(sums[j], leaf[idx].grad) < 2e-5, j


@pytest.mark.parametrize("B,Np,D,Tpe,Fd,toff,structured", [(8, 472, 768, 99, 12, 17, True), (5, 400, 768, 99, 12, 0, False),
                                                             (4, 33, 100, 25, 12, 3, False), (66, 40, 96, 50, 12, 2, False)])
def test_patch_backward_reductions_at_training_shapes(B, Np, D, Tpe, Fd, toff, structured):
    """pa_patch_bwd's parameter gradients at config #2's geometry (8 kept frequency rows x 59 kept time columns, structured
    Patchout) and at an unstructured subset (u_patchout): 16 patch groups per slot meeting in LDS, four clips in flight in
    the batch sum; accumulate on top of existing gradients; odd sizes take the scalar tails"""
    gen = torch.Generator().manual_seed(5)
    if structured:
        fk = torch.randperm(12, generator=gen)[:8].sort().values
        tk = torch.randperm(Tpe - toff, generator=gen)[:59].sort().values
        pf = fk.repeat_interleave(59).to(torch.int32)
        pt = tk.repeat(8).to(torch.int32)
    else:
        pf = torch.randint(0, Fd, (Np,), generator=gen, dtype=torch.int32)
        pt = torch.randint(0, Tpe - toff, (Np,), generator=gen, dtype=torch.int32)
    assert pf.numel() == Np
    dtok = rnd(B, Np + 2, D, seed=71).to(DEV)
    shapes = dict(cls=(1, 1, D), dist=(1, 1, D), npe=(1, 2, D), b=(D,), t=(1, D, 1, Tpe), f=(1, D, Fd, 1))
    dc = dtok.cpu().double()
    gs = dc.sum(0)
    rt = torch.zeros(D, Tpe, dtype=torch.float64)
    rf = torch.zeros(D, Fd, dtype=torch.float64)
    rt.index_add_(1, (pt.long() + toff), gs[2:].t().contiguous())
    rf.index_add_(1, pf.long(), gs[2:].t().contiguous())
    for accumulate, base in ((False, 5.0), (True, 0.25)):
        g = {k: torch.full(sh, base, device=DEV) for k, sh in shapes.items()}
        dpatch = ops.patch_bwd(dtok, pf.to(DEV), pt.to(DEV), toff, Tpe, Fd, g["cls"], g["dist"], g["npe"], g["b"], g["t"], g["f"],
                               PA_F32, accumulate=accumulate)
        off = base if accumulate else 0.0
        assert rel_err(g["cls"].view(-1), gs[0] + off) < 1e-5 and rel_err(g["dist"].view(-1), gs[1] + off) < 1e-5
        assert rel_err(g["npe"].view(2, D), gs[:2] + off) < 1e-5
        assert rel_err(g["b"], gs[2:].sum(0) + off) < 1e-5
        assert rel_err(g["t"].view(D, Tpe), rt + off) < 1e-5 and rel_err(g["f"].view(D, Fd), rf + off) < 1e-5
        assert rel_err(dpatch, dc[:, 2:].reshape(B * Np, D)) < 1e-6


@pytest.mark.parametrize("B,C,D", [(64, 527, 768), (12, 50, 768), (13, 50, 768), (9, 20, 1024), (7, 37, 1100), (21, 10, 64)])
def test_head_linear_forward_shapes(B, C, D):
    """pa_linear_f32_fwd: the model widths (768, 1024) take the four-rows-in-flight kernel (batches that are not a multiple of 16
    included), other widths the plain one"""
    x, W, b = rnd(B, D, seed=81).to(DEV), rnd(C, D, seed=82, scale=0.1).to(DEV), rnd(C, seed=83).to(DEV)
    y = ops.linear_f32_fwd(x, W, b)
    ref = x.cpu().double() @ W.cpu().double().t() + b.cpu().double()
    assert rel_err(y, ref) < 1e-5


def test_mixup_and_optimizers():
    B = 5
    x = rnd(B, 1, 16, 40, seed=36).to(DEV)
    perm = torch.tensor([3, 0, 4, 1, 2], dtype=torch.int32, device=DEV)
    lam = torch.tensor([0.9, 0.5, 0.7, 1.0, 0.6], device=DEV)
    out = ops.mixup(x, perm, lam)
    xc, lc = x.cpu(), lam.cpu().view(B, 1, 1, 1)
    assert rel_err(out, xc * lc + xc[perm.cpu().long()] * (1 - lc)) < 1e-6
    y = rnd(B, 527, seed=39).to(DEV)                       # row length not a multiple of 4
    yc = y.cpu()
    assert rel_err(ops.mixup(y, perm, lam), yc * lam.cpu().view(B, 1) + yc[perm.cpu().long()] * (1 - lam.cpu().view(B, 1))) < 1e-6
    n = 10007
    p0, g = rnd(n, seed=37), rnd(n, seed=38)
    pr = torch.nn.Parameter(p0.clone().double())
    opt = torch.optim.AdamW([pr], lr=2e-3, weight_decay=1e-2, betas=(0.9, 0.999), eps=1e-8)
    p = p0.clone().to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in (1, 2, 3):
        pr.grad = (g * step).double()
        opt.step()
        ops.adamw_update(p, (g * step).to(DEV), m, v, (2e-3, 0.9, 0.999, 1e-8, 1e-2, step), entry="pa_adamw")
    assert rel_err(p, pr.detach()) < 1e-5
    q = p0.clone().to(DEV)
    ops.sgd(q, g.to(DEV), 0.1)
    assert rel_err(q, p0 - 0.1 * g) < 1e-6


def test_ce_mixup_loss():
    """ESC-50 caller loss (ex_esc50.py:159-165) and its logits gradient."""
    import torch.nn.functional as Fnn
    B, C = 12, 50
    z = rnd(B, C, seed=60, scale=3.0)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(61))
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(62))
    lam = torch.rand(B, generator=torch.Generator().manual_seed(63)) * 0.5 + 0.5
    zr = z.double().requires_grad_(True)
    ref = (Fnn.cross_entropy(zr, y, reduction="none") * lam.double()
           + Fnn.cross_entropy(zr, y[perm], reduction="none") * (1 - lam.double())).mean()
    ref.backward()
    loss, dz = ops.ce_mixup_fwd_bwd(z.to(DEV), y.to(torch.int32).to(DEV), y[perm].to(torch.int32).to(DEV), lam.to(DEV))
    assert abs(float(loss) - float(ref.detach())) < 1e-5
    assert rel_err(dz, zr.grad) < 1e-5
    zr.grad = None
    ref2 = Fnn.cross_entropy(zr, y)
    ref2.backward()
    loss2, dz2 = ops.ce_mixup_fwd_bwd(z.to(DEV), y.to(torch.int32).to(DEV))
    assert abs(float(loss2) - float(ref2.detach())) < 1e-5 and rel_err(dz2, zr.grad) < 1e-5


@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("B,H,N,nq", [(3, 2, 474, 2), (2, 3, 130, 70), (2, 2, 67, 1)])
def test_attention_prefix_queries(dt, B, H, N, nq, pre):
    """query-limited attention (the last block only needs the cls/dist rows): compact o/lse, and in the
    backward K/V gradients from nq queries only + a Q gradient that is zero outside the first nq rows."""
    D = H * 64
    qkv, qref = _attn_inputs(rnd(B * N, 3 * D, seed=70, scale=1.5), dt, D, pre)
    o, lse = ops.attention_fwd(qkv, B, H, N, 0.125, nq=nq, flags=pre)
    assert o.shape == (B * nq, D) and lse.shape == (B * H * nq,)
    d_o = rnd(B * nq, D, seed=71).to(TD[dt]).to(DEV)
    # reference: full attention, gradient injected only at the first nq queries of every sequence
    d_full = torch.zeros(B, N, D, dtype=torch.float64)
    d_full[:, :nq] = d_o.double().cpu().view(B, nq, D)
    ro, rlse, rdqkv = _attn_ref(qref, B, H, N, 0.125, d_full.view(B * N, D))
    ro_c = ro.view(B, N, D)[:, :nq].reshape(B * nq, D)
    assert rel_err(o, ro_c) < tol(dt, 2e-5, 1.5e-2)
    assert float((lse.double().cpu().view(B, H, nq) - rlse[:, :, :nq]).abs().max()) < tol(dt, 2e-5, 2e-2)
    dqkv = ops.attention_bwd(qkv, o, d_o, lse, B, H, N, 0.125, nq=nq, flags=pre)
    e = rel_err(dqkv, rdqkv)
    record(f"attention_prefix[{dt},{B},{H},{N},{nq},pre{pre}]", dqkv=e)
    assert e < tol(dt, 5e-5, 4e-2), e
    q_part = dqkv.view(B, N, 3 * D)[:, nq:, :D]
    assert float(q_part.float().abs().max()) == 0.0


def test_gather_scatter_rows():
    x = rnd(50, 96, seed=72).to(DEV)
    idx = torch.tensor([3, 0, 49, 17], dtype=torch.int32, device=DEV)
    g = ops.gather_rows(x, idx)
    assert torch.equal(g.cpu(), x.cpu()[idx.cpu().long()])
    s = ops.scatter_rows_into_zeros(g, idx, 50)
    ref = torch.zeros(50, 96)
    ref[idx.cpu().long()] = g.cpu()
    assert torch.equal(s.cpu(), ref)
    xb = rnd(20, 64, seed=73).to(torch.bfloat16).to(DEV)
    assert torch.equal(ops.gather_rows(xb, idx[:2]).cpu(), xb.cpu()[idx[:2].cpu().long()])


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
def test_stage_weights_batched(dt):
    """One launch refreshes every straight / transposed weight copy: bit-identical to torch's cast + .t()."""
    shapes = [(768, 768), (2304, 768), (70, 130), (64, 64), (527, 768), (3, 5), (768, 256)]
    srcs = [rnd(r, c, seed=11 + i).to(DEV) for i, (r, c) in enumerate(shapes)]
    entries = []
    for i, w in enumerate(srcs):
        dst = torch.full(w.shape, 7.0, device=DEV, dtype=TD[dt]) if i % 3 != 1 else None
        dst_t = torch.full((w.shape[1], w.shape[0]), 7.0, device=DEV, dtype=TD[dt]) if i % 3 != 2 else None
        entries.append((w, dst, dst_t))
    table, n, tiles = ops.make_stage_table(entries, DEV)
    ops.stage_weights(table, n, tiles, dt)
    torch.cuda.synchronize()
    for w, dst, dst_t in entries:
        if dst is not None:
            assert torch.equal(dst, w.to(TD[dt]))
        if dst_t is not None:
            assert torch.equal(dst_t, w.t().contiguous().to(TD[dt]))


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("hyper_on_device", [False, True])
def test_adamw_stage_equals_adamw_then_stage_weights(dt, hyper_on_device):
    """ABI 6: pa_adamw_stage (optimizer update + straight / transposed copies from the registers that hold the updated values) is
    bit-identical -- parameters, both moments, every copy -- to pa_adamw followed by pa_stage_weights, over matrices with both /
    one / no copy, shapes off the 64-tile and off the 4-element grid, a parameter at an odd (unaligned) offset, and with the
    step's scalars by value or in device memory."""
    shapes = [(768, 768), (768,), (2304, 768), (70, 130), (64, 64), (3, 5), (527,), (527, 768), (5000,), (768, 256)]
    copies = ["both", None, "both", "both", "t", "both", None, None, None, "straight"]       # (3, 5) and what follows sit at odd offsets
    offs, off = [], 0
    for sh in shapes:
        offs.append(off)
        off += int(np.prod(sh))
    total = off
    g0 = torch.Generator().manual_seed(5)
    P = (torch.rand(total, generator=g0) * 2 - 1).to(DEV)
    G = ((torch.rand(total, generator=g0) * 2 - 1) * 1e-2).to(DEV)
    Mo = ((torch.rand(total, generator=g0) * 2 - 1) * 1e-2).to(DEV)
    Vo = (torch.rand(total, generator=g0) * 1e-4).to(DEV)
    hp = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=7)
    # (a) separately
    pa, ma, va = P.clone(), Mo.clone(), Vo.clone()
    hyper = (hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], hp["step"])
    ops.adamw_update(pa, G, ma, va, hyper, entry="pa_adamw")
    want = []
    for sh, o, c in zip(shapes, offs, copies):
        w = pa[o:o + int(np.prod(sh))].view(sh[0], -1) if c else None
        want.append((None if c in (None, "t") else w.to(TD[dt]), None if c in (None, "straight") else w.t().contiguous().to(TD[dt])))
    # (b) one launch
    pb, mb, vb = P.clone(), Mo.clone(), Vo.clone()
    entries, outs = [], []
    for sh, o, c in zip(shapes, offs, copies):
        rows = sh[0] if c else 1
        cols = int(np.prod(sh)) // rows
        dst = torch.full((rows, cols), 7.0, device=DEV, dtype=TD[dt]) if c in ("both", "straight") else None
        dst_t = torch.full((cols, rows), 7.0, device=DEV, dtype=TD[dt]) if c in ("both", "t") else None
        entries.append((o, rows, cols, dst, dst_t))
        outs.append((dst, dst_t))
    table = ops.make_adamw_stage_table(entries, DEV)
    if hyper_on_device:
        host = torch.empty(7, dtype=torch.float32)
        ops.adamw_hyper(*hyper, host)
        hyper = host.to(DEV)
    ops.adamw_update(pb, G, mb, vb, hyper, table=table, dtype=dt, entry="pa_adamw_stage")
    torch.cuda.synchronize()
    assert torch.equal(pb, pa) and torch.equal(mb, ma) and torch.equal(vb, va)
    assert float((pb - P).abs().max()) > 1e-3
    for (d, t), (wd_, wt_) in zip(outs, want):
        assert (d is None) == (wd_ is None) and (t is None) == (wt_ is None)
        if d is not None:
            assert torch.equal(d, wd_)
        if t is not None:
            assert torch.equal(t, wt_)


def test_staged_cache_batched_refresh_matches_single():
    """_Staged: after a parameter update the batched refresh yields the same copies as first-use staging."""
    from passt_amd.passt import _Staged
    ps = [torch.nn.Parameter(rnd(96, 160, seed=31 + i).to(DEV)) for i in range(3)]
    st = _Staged()
    first = [(st.get(p, PA_BF16, False), st.get(p, PA_BF16, True)) for p in ps]
    with torch.no_grad():
        for p in ps:
            p.mul_(1.5).add_(0.25)
    again = [(st.get(p, PA_BF16, False), st.get(p, PA_BF16, True)) for p in ps]
    for p, (a, at), (f, ft) in zip(ps, again, first):
        assert a.data_ptr() == f.data_ptr() and at.data_ptr() == ft.data_ptr()     # refreshed in place
        assert torch.equal(a, p.detach().to(torch.bfloat16))
        assert torch.equal(at, p.detach().t().contiguous().to(torch.bfloat16))


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("tune", [0, 1, 6, 7, 8, 17, 18])
@pytest.mark.parametrize("M,N,K", [(300, 264, 128), (2 * 474, 3072, 768), (1000, 768, 256)])
def test_gemm_dgelu_fused_bias_gradient(dt, tune, M, N, K):
    """EPI_DGELU can return the column sums of its output (the fc1.bias gradient) from the same epilogue."""
    if dt == PA_F32 and tune != 0:
        pytest.skip("the f32 parity path has one tile variant")
    A = rnd(M, K, seed=40).to(TD[dt]).to(DEV)
    Bm = rnd(N, K, seed=41, scale=0.3).to(TD[dt]).to(DEV)
    aux = rnd(M, N, seed=42, scale=2.0).to(TD[dt]).to(DEV)
    dg = torch.empty(M, N, device=DEV, dtype=TD[dt])
    db = torch.full((N,), 3.0, device=DEV)
    ws = ops.gemm_colsum_ws(M, N, DEV)
    ops.GEMM_TUNE = tune
    try:
        ops.gemm_nt(A, Bm, dt, EPI_DGELU, aux=aux, out_lp=dg, colsum_out=db, colsum_ws=ws)
        torch.cuda.synchronize()
        a64 = aux.double().cpu()
        gp = 0.5 * (1 + torch.erf(a64 / math.sqrt(2))) + a64 * torch.exp(-0.5 * a64 * a64) / math.sqrt(2 * math.pi)
        ref = (A.double().cpu() @ Bm.double().cpu().T) * gp
        assert rel_err(dg, ref) < tol(dt, 3e-5, 1.2e-2)
        e = rel_err(db, ref.sum(0))
        record(f"gemm_dgelu_colsum[{dt},{tune},{M}x{N}x{K}]", rel=e)
        assert e < tol(dt, 3e-5, 2e-3)
        db2 = db.clone()
        ops.gemm_nt(A, Bm, dt, EPI_DGELU, aux=aux, out_lp=dg, colsum_out=db2, colsum_ws=ws, colsum_accumulate=True)
        assert rel_err(db2, 2 * ref.sum(0)) < tol(dt, 3e-5, 2e-3)
    finally:
        ops.GEMM_TUNE = 0


def test_wave_augment_matches_reference_pipeline():
    """pa_wave_augment (gain, pad/truncate, roll, waveform mixup) vs the golden outputs of the reference's own
    dataset code and vs the oracle on a second, ragged case."""
    from oracle import wave_oracle as W
    from passt_amd.augment import WaveAugment
    from tests.golden import make_golden as G
    c = G.WAVE_CASE
    raws = G.wave_inputs(c)
    g = np.load(os.path.join(os.path.dirname(G.__file__), "wave_augment.npz"))
    B, ldx = len(raws), max(len(r) for r in raws)
    x = torch.zeros(B, ldx)
    for b, r in enumerate(raws):
        x[b, :len(r)] = torch.from_numpy(r)
    aug = WaveAugment(clip_samples=c["L"])
    params = (np.array(c["gain_db"]), np.array(c["shift"]), np.array(c["partner"]), np.array(c["lam"], np.float32))
    wave, tgt = aug(x.to(DEV), torch.eye(B).to(DEV), torch.tensor([len(r) for r in raws], dtype=torch.int32), params)
    assert wave.shape == (B, 1, c["L"])
    e = float((wave[:, 0].cpu() - torch.from_numpy(g["out"])).abs().max())
    record("wave_augment", abs=e)
    assert e < 2e-7
    assert float((tgt.cpu() - torch.from_numpy(g["target"])).abs().max()) < 1e-6
    # drawn parameters, 10 s clips: against the oracle
    torch.manual_seed(5)
    np.random.seed(5)
    aug = WaveAugment(clip_samples=320000)
    raws = [(rnd(n, seed=60 + i, scale=0.3) + 0.01 * i).numpy() for i, n in enumerate([320000, 200000, 400000, 320000])]
    x = torch.zeros(4, 400000)
    for b, r in enumerate(raws):
        x[b, :len(r)] = torch.from_numpy(r)
    p = aug.draw(4)
    wave, _ = aug(x.to(DEV), None, torch.tensor([len(r) for r in raws], dtype=torch.int32), p)
    ref, _ = W.augment_batch(raws, list(p[0]), list(p[1]), list(p[2]), list(p[3]), 320000)
    assert float((wave[:, 0].cpu() - torch.from_numpy(ref)).abs().max()) < 5e-7


@pytest.mark.parametrize("tune", [0, 6, 7, 8, 17, 18])
@pytest.mark.parametrize("M,N,K", [(1, 8, 64), (33, 40, 64), (255, 256, 64), (257, 264, 128), (5000, 8, 192),
                                   (70000, 264, 64), (3 * 474, 2304, 768)])
def test_persistent_gemm_edge_shapes(tune, M, N, K):
    """The persistent role-split kernel at its edges: a single (ragged) tile, one K step, fewer tiles than CUs,
    hundreds of rounds per workgroup (M = 70000: 274+ row tiles x 2 column tiles), partial tiles on both axes;
    every epilogue, including split-K partial slabs with an uneven number of K steps per slice."""
    dt = PA_BF16
    A = rnd(M, K, seed=80).to(TD[dt]).to(DEV)
    Bm = rnd(N, K, seed=81, scale=0.5).to(TD[dt]).to(DEV)
    bias = rnd(N, seed=82).to(DEV)
    resid = rnd(M, N, seed=83).to(DEV)
    aux = rnd(M, N, seed=84, scale=2.0).to(TD[dt]).to(DEV)
    acc = A.double().cpu() @ Bm.double().cpu().T
    ref = acc + bias.double().cpu()
    old = ops.GEMM_TUNE
    try:
        ops.GEMM_TUNE = tune
        out = torch.full((M, N), 9.0, device=DEV, dtype=TD[dt])
        ops.gemm_nt(A, Bm, dt, EPI_STORE, bias=bias, out_lp=out)
        assert rel_err(out, ref) < tol(dt)
        pre, act = torch.empty_like(out), torch.empty_like(out)
        ops.gemm_nt(A, Bm, dt, EPI_GELU, bias=bias, out_lp=pre, out_lp2=act)
        assert rel_err(pre, ref) < tol(dt) and rel_err(act, torch.nn.functional.gelu(pre.double().cpu())) < 6e-3
        out32 = torch.empty(M, N, device=DEV)
        ops.gemm_nt(A, Bm, dt, EPI_RESID, bias=bias, resid=resid, out_f32=out32)
        assert rel_err(out32, ref + resid.double().cpu()) < 3e-3
        dg = torch.empty_like(out)
        ops.gemm_nt(A, Bm, dt, EPI_DGELU, aux=aux, out_lp=dg)
        a64 = aux.double().cpu()
        gp = 0.5 * (1 + torch.erf(a64 / math.sqrt(2))) + a64 * torch.exp(-0.5 * a64 * a64) / math.sqrt(2 * math.pi)
        assert rel_err(dg, acc * gp) < 1.2e-2
        ksteps = K * 2 // 128
        for split in sorted({1, min(2, ksteps), min(3, ksteps)}):
            part = torch.full((split, M, N), 5.0, device=DEV)
            ops.gemm_nt(A, Bm, dt, EPI_PARTIAL, out_f32=part, split_k=split)
            assert rel_err(part.sum(0), acc) < 3e-3, split
    finally:
        ops.GEMM_TUNE = old


def test_blocked_pre_buffer_holds_every_pass_of_every_tile_height():
    """pa_gemm_blocked_pre_elems covers whole 128-, 192- and 256-row tiles (with rows rounded to 256 the last
    32-row passes of a 192-row tile at e.g. M = 474 * 7 were written past the buffer), and the forward GELU GEMM leaves
    a canary behind the buffer untouched."""
    lib = ops._lib.load()
    for M in (474 * 7, 474 * 14, 474 * 41, 353 * 18, 790 * 11, 1000, 1, 768):
        rows = lib.pa_gemm_blocked_pre_elems(M, 64) // 64
        for hgt in (128, 192, 256):
            assert rows >= (M + hgt - 1) // hgt * hgt, (M, hgt, rows)
    M, N, K = 474 * 7, 3072, 768
    record(f"blocked_pre_buffer_ran[{M},{N},{K}]", ran=int(bool(ops.blocked_pre_ok(M, N, K))))
    if not ops.blocked_pre_ok(M, N, K):
        pytest.skip("the library runs this shape on a kernel without the blocked form")
    n = lib.pa_gemm_blocked_pre_elems(M, N)
    big = torch.empty(n + (1 << 16), device=DEV, dtype=torch.bfloat16)
    big[n:] = 123.0
    x = rnd(M, K, seed=31).to(torch.bfloat16).to(DEV)
    W = (rnd(N, K, seed=32) * 0.05).to(torch.bfloat16).to(DEV)
    act = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    ops.gemm_nt(x, W, PA_BF16, EPI_GELU, bias=rnd(N, seed=33).to(DEV), out_lp=big[:n].view(-1, N), out_lp2=act, flags=ops.GEMM_BLOCKED_PRE)
    torch.cuda.synchronize()
    assert bool((big[n:] == 123.0).all())


@pytest.mark.parametrize("M,N,K", [(2304, 3072, 768), (1999, 3072, 768), (30336, 3072, 768), (777, 1024, 256), (4000, 4096, 1024),
                                   (5003, 3072, 768), (8200, 1536, 768), (25280, 4096, 1024), (12345, 3136, 832), (474 * 7, 3072, 768),
                                   (353 * 18, 3072, 768)])
def test_blocked_pre_activation_equals_row_major(M, N, K):
    """PA_GEMM_BLOCKED_PRE: fc1 + GELU writes the pre-activation in the blocked accumulator-order layout and the GELU'
    epilogue of the input-gradient GEMM reads it back: activation, d_pre and the fused fc1.bias column sums are
    BIT-identical to the row-major path (same arithmetic, only the storage of one intermediate differs)."""
    dt = PA_BF16
    record(f"blocked_pre_equals_row_major_ran[{M},{N},{K}]", ran=int(bool(ops.blocked_pre_ok(M, N, K))))
    if not ops.blocked_pre_ok(M, N, K):
        pytest.skip("the library runs this shape on a kernel without the blocked form")
    x = rnd(M, K, seed=31).to(TD[dt]).to(DEV)
    W = (rnd(N, K, seed=32) * 0.05).to(TD[dt]).to(DEV)
    b = rnd(N, seed=33).to(DEV)
    dy = rnd(M, K, seed=34).to(TD[dt]).to(DEV)           # gradient wrt fc2's input has fc1's output shape: dy [M][K2] x Wt [N][K2]
    Wt = (rnd(N, K, seed=35) * 0.05).to(TD[dt]).to(DEV)
    pre_b, act_b = ops.linear_gelu(x, W, b, dt)
    assert isinstance(pre_b, ops.BlockedPre)
    pre_r = torch.empty((M, N), device=DEV, dtype=TD[dt])
    act_r = torch.empty((M, N), device=DEV, dtype=TD[dt])
    ops.gemm_nt(x, W, dt, EPI_GELU, bias=b, out_lp=pre_r, out_lp2=act_r)
    assert torch.equal(act_b, act_r)
    ws = ops.gemm_colsum_ws(M, N, DEV)
    db_b, db_r = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    d_b = ops.dgelu_gemm(dy, Wt, pre_b, dt, colsum_out=db_b, colsum_ws=ws)
    d_r = ops.dgelu_gemm(dy, Wt, pre_r, dt, colsum_out=db_r, colsum_ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(d_b, d_r)
    # a wave tile that sticks out past row M adds and then subtracts the rows past M, whose pre-activation is 0 in the
    # row-major path (outside the descriptor) and a duplicate row in the blocked one: equal up to that rounding
    if M % 768 == 0:                      # whole 128- / 192- / 256-row tiles
        assert torch.equal(db_b, db_r)
    else:
        assert rel_err(db_b, db_r) < 1e-5
    ref = (dy.double().cpu() @ Wt.double().cpu().T)
    xp = pre_r.double().cpu()
    ref = ref * (0.5 * (1 + torch.erf(xp / 2 ** 0.5)) + xp * torch.exp(-xp * xp / 2) / (2 * torch.pi) ** 0.5)
    assert rel_err(d_b, ref) < 1.5e-2


@pytest.mark.parametrize("tokens", [1500, 130, 47, 2 * 474 + 5])
def test_wgrad_tn_batched_fused_bias_gradient(tokens):
    """A problem with db gets colsum(dY) from the batched launch (ninth MFMA per phase in the tiles of the first
    X-column block): == the f64 column sums, for ragged token counts, dY widths that are not tile multiples, with and
    without accumulation; the weight gradients are unchanged."""
    dt = PA_BF16
    shapes = [(tokens, 768, 768, False), (tokens, 2304, 768, True), (tokens, 776, 3072, True), (tokens, 3072, 264, False)]
    probs, refs = [], []
    for i, (M, N, K, with_b) in enumerate(shapes):
        dY = rnd(M, N, seed=190 + i).to(TD[dt]).to(DEV)
        X = rnd(M, K, seed=195 + i).to(TD[dt]).to(DEV)
        acc = i == 2
        out = torch.full((N, K), 0.25 if acc else 7.0, device=DEV)
        db = torch.full((N,), 0.25 if acc else -3.0, device=DEV) if with_b else None
        probs.append((dY, X, out, acc, db))
        refs.append((dY.double().cpu().T @ X.double().cpu() + (0.25 if acc else 0.0),
                     dY.double().cpu().sum(0) + (0.25 if acc else 0.0)))
    ops.wgrad_tn_batched(probs, dt)
    torch.cuda.synchronize()
    for (dY, X, out, acc, db), (ref_w, ref_b) in zip(probs, refs):
        assert rel_err(out, ref_w) < 3e-3
        if db is not None:
            err = (db.double().cpu() - ref_b).abs().max().item() / max(ref_b.abs().max().item(), 1e-6)
            record(f"wgrad_tn_fused_bias_t{tokens}_n{dY.shape[1]}", err=err)
            assert err < 1e-5          # f32 accumulation of exact bf16 values


def test_wgrad_tn_batched_matches_single_launches():
    """pa_gemm_tn_batched + pa_reduce_partials_batched: four weight gradients (different shapes, one with only a few
    token rows, one accumulating) in one launch each == the per-problem path."""
    dt = PA_BF16
    shapes = [(1500, 768, 768), (1500, 2304, 768), (1500, 768, 3072), (130, 3072, 768)]   # (tokens, N, K)
    probs, refs = [], []
    for i, (M, N, K) in enumerate(shapes):
        dY = rnd(M, N, seed=90 + i).to(TD[dt]).to(DEV)
        X = rnd(M, K, seed=95 + i).to(TD[dt]).to(DEV)
        out = torch.full((N, K), 0.5 if i == 1 else 7.0, device=DEV)
        probs.append((dY, X, out, i == 1))
        refs.append(dY.double().cpu().T @ X.double().cpu() + (0.5 if i == 1 else 0.0))
    ops.wgrad_tn_batched(probs, dt)
    torch.cuda.synchronize()
    for (dY, X, out, acc), ref in zip(probs, refs):
        assert rel_err(out, ref) < 3e-3
        single = torch.full_like(out, 0.5 if acc else 7.0)
        db1 = torch.full((dY.shape[1],), 0.5 if acc else 7.0, device=DEV)
        ops.wgrad_tn(dY, X, single, dt, acc, db=db1)          # single launch, bias gradient from the same kernel
        assert rel_err(out, single.double().cpu()) < 1e-5     # same products, different split-K grouping
        assert rel_err(db1, dY.double().cpu().sum(0) + (0.5 if acc else 0.0)) < 1e-5


def test_wrappers_copy_offset_views_before_entries_that_refuse_them():
    """The entries that move 16-byte vectors refuse a base pointer off 16-byte alignment (include/passt_amd.h; the refusals themselves
    are asserted without a device in tests/test_patch_cases_cpu.py).  The ops wrappers give such an entry a copy of an offset view,
    so the caller sees the result of the aligned call, bit for bit; no misaligned pointer reaches a kernel here."""
    def off(t):                                      # the same values one element behind a 16-byte boundary
        buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 and v.is_contiguous()
        return v
    M, D = 10, 260
    rows, a0, a1 = rnd(2, D, seed=1).to(DEV), rnd(M, D, seed=2).to(DEV), rnd(M, D, seed=3).to(DEV)
    idx = torch.tensor([0, 5], dtype=torch.int32, device=DEV)
    want = ops.tail_inject(rows, idx, M, a0, a1, PA_BF16)
    got = ops.tail_inject(off(rows), idx, M, off(a0), off(a1), PA_BF16)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    x = rnd(M, D, seed=4).to(DEV)
    rs = torch.tensor([1.0, 0.5] * (M // 2), device=DEV)
    assert torch.equal(ops.convert(off(x), PA_BF16, rowscale=rs), ops.convert(x, PA_BF16, rowscale=rs))
    assert torch.equal(ops.convert(off(x), PA_BF16), ops.convert(x, PA_BF16))          # pa_convert_f32 reads an offset `in` itself
    B, F, T, P, s = 2, 13, 18, 4, 3
    Fg, Tg = (F - P) // s + 1, (T - P) // s + 1
    pf = torch.arange(Fg, dtype=torch.int32).repeat_interleave(Tg).to(DEV)
    pt = torch.arange(Tg, dtype=torch.int32).repeat(Fg).to(DEV)
    dcols = rnd(B * Fg * Tg, P * P, seed=5).to(torch.bfloat16).to(DEV)
    want = ops.patch_input_bwd(dcols, pf, pt, B, F, T, P, s, s)
    out = off(torch.zeros(B, 1, F, T, device=DEV))
    assert ops.patch_input_bwd(off(dcols), pf, pt, B, F, T, P, s, s, out=out) is out and torch.equal(out, want)
    Np, Dm = Fg * Tg, 16
    dtok = rnd(B, Np + 2, Dm, seed=6).to(DEV)
    assert torch.equal(ops.patch_bwd(off(dtok), pf, pt, 0, Tg, Fg, None, None, None, None, None, None, PA_BF16),
                       ops.patch_bwd(dtok, pf, pt, 0, Tg, Fg, None, None, None, None, None, None, PA_BF16))
    xb = rnd(6, 8, seed=7).to(torch.bfloat16).to(DEV)
    gi = torch.tensor([5, 0, 3], dtype=torch.int32, device=DEV)
    assert torch.equal(ops.gather_rows(off(xb), gi), xb[gi.long()])                    # 2 bytes off: a copy; 4 bytes off: 4-byte words
    xf = rnd(6, 8, seed=8).to(DEV)
    assert torch.equal(ops.gather_rows(off(xf), gi), xf[gi.long()])
    torch.cuda.synchronize()

"""The row-kernel parity suite checks itself (no GPU): every checker of tests/row_kernel_cases.py passes against a plain f32
torch CPU implementation at every listed shape -- a bound nothing could meet would fail here --, the exact-sum inputs really sum
identically in any order, and the shape lists hit the kernel instances and launch geometries they are meant to hit."""
import pytest
import torch

from tests import row_kernel_cases as K
from tests.row_kernel_cases import PA_BF16, PA_F32

IMPL = K.TorchF32()


# ---- reference self-check: layer_norm and autograd -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("D", K.LN_D)
def test_layernorm_widths(dt, D):
    K.check_layernorm(IMPL, K.LN_D_ROWS, D, dt)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M", list(K.LN_M_WORKGROUPS))
def test_layernorm_row_counts(dt, M):
    K.check_layernorm(IMPL, M, K.LN_M_WIDTH, dt)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", K.LN_EXACT)
def test_layernorm_exact_sums(dt, M, D):
    K.check_ln_exact(IMPL, M, D, dt)


@pytest.mark.parametrize("M,D", K.LN_CONDITIONING_SHAPES)
@pytest.mark.parametrize("c,sigma", K.LN_CONDITIONING)
def test_layernorm_conditioning(c, sigma, M, D):
    got, base = K.check_ln_conditioning(IMPL, c, sigma, M, D)
    assert got == base                      # the baseline is this implementation: the bound is 4x its own error


def test_conditioning_bound_rejects_a_one_pass_variance():
    """E[x^2] - mean^2 in f32 at c = 300, sigma = 0.5 misses the measured bound by orders of magnitude"""
    class OnePass(K.TorchF32):
        def ln_fwd(self, x, g, b, eps, dt):
            mean = x.mean(1)
            rstd = ((x * x).mean(1) - mean * mean + K.f32_eps(eps)).clamp_min(1e-12).rsqrt()
            return ((x - mean[:, None]) * rstd[:, None] * g + b).to(K.TD[dt]), mean, rstd
    with pytest.raises(AssertionError):
        K.check_ln_conditioning(OnePass(), 300.0, 0.5, 37, 768)


@pytest.mark.parametrize("D", K.LN_CONSTANT_D)
def test_layernorm_constant_rows(D):
    K.check_ln_constant_rows(IMPL, D)


# ---- the head composition, Linear, the losses ------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Ntok,D", K.HEAD_SHAPES + (K.HEAD_FWD_ONLY,))
def test_head_pre(B, Ntok, D):
    K.check_head(IMPL, B, Ntok, D)


@pytest.mark.parametrize("B,C,D", K.LINEAR_SHAPES)
def test_head_linear(B, C, D):
    K.check_linear(IMPL, B, C, D)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("B,C", K.BCE_SHAPES)
def test_bce(B, C, scale):
    K.check_bce(IMPL, B, C, scale)


@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_bce_extreme_logits(scale):
    K.check_bce_extreme(IMPL, scale)


def test_bce_small_case():
    K.check_bce_small(IMPL)


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("B,C", K.CE_SHAPES)
def test_ce_mixup(B, C, spread):
    K.check_ce(IMPL, B, C, spread)


# ---- .sum ------------------------------------------------------------------------------------------------------------------
def test_reductions_against_plain_sums():
    for n in K.SLAB_N:
        for splits in K.SLAB_SPLITS:
            K.check_reduce_slabs(IMPL, splits, n)
    for splits in K.ROWS_SPLITS:
        for n in K.ROWS_N:
            K.check_reduce_rows(IMPL, splits, n)
    K.check_reduce_rows(IMPL, *K.ROWS_WIDE)
    K.check_reduce_batch(IMPL)
    for R in K.COLSUM_F32_R:
        for C in K.COLSUM_F32_C:
            K.check_colsum_f32(IMPL, R, C)
    for R in K.COLSUM_R:
        for C in K.COLSUM_C:
            K.check_colsum(IMPL, R, C)
    for C in K.ROWSUM_C:
        for R in K.ROWSUM_R:
            K.check_rowsum(IMPL, R, C)


# ---- exact-sum inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,t,dim", K.exact_sum_inputs(), ids=[e[0] for e in K.exact_sum_inputs()])
def test_exact_sum_inputs_sum_identically_in_any_order(name, t, dim):
    t = t if dim == 0 else t.t().contiguous()                       # reduce over dim 0
    assert t.dtype == torch.float32 and K.exact_sum_safe(t, 0)
    assert torch.equal(t.to(torch.bfloat16).float(), t)             # exact in bf16 as well
    want = t.to(torch.int64).sum(0)
    assert int(want.abs().max()) < K.EXACT_LIMIT
    assert torch.equal(t.double().sum(0), want.double())
    g = torch.Generator().manual_seed(1)
    R = t.shape[0]
    for _ in range(3):                                              # random permutations: torch's f32 sum, and one row at a time
        perm = torch.randperm(R, generator=g)
        assert torch.equal(t[perm].sum(0).to(torch.int64), want)
        assert torch.equal(t[perm].cumsum(0)[-1].to(torch.int64), want)
    for blk in (3, 16, 64, 1000):                                   # blocked orders: per-block f32 sums, then their f32 sum
        parts = [c.sum(0) for c in t.split(blk)]
        assert torch.equal(torch.stack(parts).sum(0).to(torch.int64), want)
        assert torch.equal(torch.stack(parts[::-1]).cumsum(0)[-1].to(torch.int64), want)


# ---- shape lists -----------------------------------------------------------------------------------------------------------
def test_layernorm_width_list_hits_every_kernel_instance():
    inst = {}
    for D in K.LN_D:
        assert D % 4 == 0 and D <= 2048
        inst.setdefault(K.ln_instance(D), []).append(D)
    assert set(inst) == {1, 2, 3, 4, 8}
    cols = {-(-D // 256) for D in K.LN_D}
    assert {1, 2, 3, 4} <= cols and len([c for c in cols if 5 <= c <= 8]) >= 2
    for v, ds in inst.items():
        ragged = [D for D in ds if (D // 4) % 64 != 0]
        full = [D for D in ds if (D // 4) % 64 == 0]
        assert ragged and full, (v, ds)                             # a partly filled and a full last vector column
    assert 2048 in K.LN_D and any(12 * D * 4 > 64 * 1024 for D in K.LN_D)


def test_layernorm_row_list_hits_the_workgroup_counts():
    assert [K.ln_bwd_workgroups(M) for M in K.LN_M_WORKGROUPS] == list(K.LN_M_WORKGROUPS.values())
    assert sorted(set(K.LN_M_WORKGROUPS.values())) == [1, 16, 17, 64, 65, 1024]
    assert min(K.LN_M_WORKGROUPS) < 4 and max(K.LN_M_WORKGROUPS) > 8192
    assert max(K.LN_M_WORKGROUPS) % (4 * 1024) != 0                 # a ragged last stride under the workgroup cap


def test_loss_and_reduction_lists_hit_their_loop_boundaries():
    n = [B * C for B, C in K.BCE_SHAPES]
    assert n == [1, 255, 256, 257, 64 * 527, 130 * 527] and -(-n[-1] // 256) > 256
    assert any(C > 64 for _, C in K.CE_SHAPES) and any(B % 4 for B, _ in K.CE_SHAPES)
    assert {15, 16, 17, 63, 64, 65} <= set(K.ROWS_SPLITS) and K.ROWS_WIDE[1] > 2048 * 16
    assert any(n % 4 for n in K.SLAB_N) and 768 * 768 in K.SLAB_N and -(-768 * 768 // 256) > 2048     # batched, unaligned: two trips
    assert max(K.SLAB_N) % 4 and -(-max(K.SLAB_N) // 256) > 4096                                       # pa_reduce_partials: two trips
    assert len(K.mixed_batch()) == 12 and {d["mode"] for d in K.mixed_batch()} == {K.REDUCE_SLABS, K.REDUCE_ROWS}

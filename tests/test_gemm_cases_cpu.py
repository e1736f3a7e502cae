"""The exact GEMM parity suite checks itself (no GPU): every checker of tests/gemm_cases.py passes against TorchGemm -- the f64
product, the header's epilogue in f32, one rounding -- at every listed case, so every torch.equal and every bound is one an honest
implementation meets; every condition on the operands is asserted per case (inside the checkers: nt_conditions / tn_conditions);
and seven deliberate faults of the kind a tile kernel makes are each rejected -- three of them while still passing the rel_err
bound of the random-operand tests, which is why this suite exists."""
from dataclasses import replace

import pytest
import torch

from tests import gemm_cases as G
from tests.gemm_cases import DGELU, GELU, NT, PA_BF16, PA_F32, PARTIAL, RESID, STORE, TN

IMPL = G.TorchGemm()


def run(cases):
    for c in cases:
        G.check_nt(IMPL, c)


# ---- every case of the GPU suite -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tune", G.TUNES)
def test_nt_tile_variants_bf16(tune):
    run(G.nt_variant_cases(tune, PA_BF16))


def test_nt_f32():
    run(G.nt_variant_cases(0, PA_F32))


@pytest.mark.parametrize("tune", G.ROLE_SPLIT)
def test_nt_flags(tune):
    run(G.nt_flag_cases(tune))


@pytest.mark.parametrize("tune,dt", [(t, PA_BF16) for t in G.ROWSCALE_TUNES] + [(0, PA_F32)])
def test_rowscale(tune, dt):
    run(G.rowscale_cases(tune, dt))


@pytest.mark.parametrize("M,N,steps", G.SPLITK_SHAPES + G.SPLITK_UNSPLIT)
def test_splitk(M, N, steps):
    run(G.splitk_cases(M, N, steps))


@pytest.mark.parametrize("M,N,K", [(1, 3072, 1088), (33, 3072, 1088), (129, 1024, 1088), (2689, 3072, 768), (8193, 1024, 768)])
def test_mlp_blocked(M, N, K):
    G.check_mlp_blocked(IMPL, M, N, K)


@pytest.mark.parametrize("dt,tune", G.TN_KERNELS)
@pytest.mark.parametrize("T", G.TN_TOKENS)
def test_tn(dt, tune, T):
    for c in G.tn_cases(dt, tune, T):
        G.check_tn(IMPL, c)


def test_tn_batched():
    G.check_tn_batched(IMPL, G.batch_cases(341, G.TN_BATCH_1))
    G.check_tn_batched(IMPL, G.batch_cases(97, G.TN_BATCH_4), problem_major=True)
    G.check_tn_batched(IMPL, G.batch_cases((341, 97, 48, 1), G.TN_BATCH_MIXED_SPLITS))
    for T, n_long, L in G.TN_PLANS:
        probs = [(M, N, n_long + 1, db) for M, N, _, db in G.TN_BATCH_4]
        G.check_tn_batched(IMPL, G.batch_cases(T, probs, fam_shift=n_long), plan=(n_long, L))


# ---- the lists hold what they are meant to hold ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("tune", G.TUNES)
def test_shape_lists_cover_every_edge(tune, dt):
    tm, tn = G.TILE[tune] if dt == PA_BF16 else (128, 128)
    shapes = G.nt_shapes(tune, dt)
    assert {s[0] for s in shapes} == {1, tm - 1, tm, tm + 1, 2 * tm + 33}
    assert {s[1] for s in shapes} == {8, tn - 8, tn, tn + 8}
    assert {s[2] // G.kelems(dt, 1) for s in shapes} == {1, 2, 3, 7, 17}
    assert (2 * tm + 33, tn + 8, G.kelems(dt, 17)) in shapes
    cases = G.nt_variant_cases(tune, dt)
    assert {c.epi for c in cases} >= {STORE, GELU, RESID, DGELU}
    assert {c.fam for c in cases} == {"ternary", "full", "tag"}
    parts = [c for c in cases if c.epi == PARTIAL]
    if dt == PA_F32 or tune not in G.NO_PARTIAL:
        assert {c.split_k for c in parts} == {1, 2, 3}
        lens = [[k1 - k0 for k0, k1 in G.nt_slices(c)] for c in parts]
        assert any(0 in ln for ln in lens), "a case whose last slice is empty"
        assert any(len(set(ln)) > 1 and 0 not in ln for ln in lens), "a case with uneven slices"


def test_row_factors_change_where_they_must():
    f = G.row_factors(600)
    assert set(f.tolist()) == {0.0, 1.0, 2.0, 0.5}
    assert all(f[b] != f[b - 1] for b in range(32, 600, 32)), "every 32-row pass, wave tile and workgroup tile begins with a new factor"
    assert all(len(set(f[b:b + 32].tolist())) > 1 for b in range(0, 576, 32)), "the factor changes inside every 32-row pass"
    for tune in G.ROWSCALE_TUNES:
        Ms = {c.M for c in G.rowscale_cases(tune, PA_BF16)}
        assert Ms == {1, 33, 257, 2 * G.TILE[tune][0] + 33}


def test_tn_lists():
    for dt, tune in G.TN_KERNELS:
        seen = set()
        for T in G.TN_TOKENS:
            cs = G.tn_cases(dt, tune, T)
            assert {(c.M, c.N) for c in cs} == set(G.TN_SHAPES)
            seen |= {c.split_k for c in cs}
            for c in cs:
                sl = G.tn_slices(c)
                if c.split_k > 2:
                    assert 0 < sl[-1][1] - sl[-1][0] < c.step, "the last slice is a single ragged step"
        assert {1, 2} < seen
    assert G.plan_slices(341, 2, 3) == [(0, 144), (144, 288), (288, 341)] and G.plan_slices(96, 1, 1) == [(0, 48), (48, 96)]


# ---- mutation evidence -----------------------------------------------------------------------------------------------------
# a long K: max|ref| is about 200, one product term 1, a bias step at most 2
M_STORE = NT(dt=PA_BF16, epi=STORE, M=257, N=264, K=4096, small_bias=True)
M_PARTIAL = NT(dt=PA_BF16, epi=PARTIAL, M=129, N=264, K=1088, split_k=2, bias=False)
# a residual stream much larger than the branch (integers up to 2^15, still exact): what hides a branch error from max / max
M_ROWSCALE = NT(dt=PA_BF16, epi=RESID, M=161, N=264, K=192, factors=True, entry="rowscale", small_bias=True, resid_mul=4096)
M_FULL = NT(dt=PA_BF16, epi=STORE, M=129, N=264, K=1088, fam="full")


class DropsLastK(G.TorchGemm):
    """the last K element of the first slice (of the whole K where there is one slice) never reaches the accumulator"""

    def product(self, A, B, c, z=None):
        return super().product(A[:, :-1], B[:, :-1], c, z) if z in (None, 0) else super().product(A, B, c, z)


class ShiftsBias(G.TorchGemm):
    """the last column tile adds bias[n - 8]"""

    def bias_of(self, c, bias):
        n0 = (G.cdiv(c.N, c.tile[1]) - 1) * c.tile[1]
        b = bias.clone()
        b[max(n0, 8):] = bias[max(n0, 8) - 8:c.N - 8]
        return super().bias_of(c, b)


class NeighbourFactor(G.TorchGemm):
    """rows of the last partial tile take the factor of the row below"""

    def factors_of(self, c, f):
        m0 = (c.M - 1) // c.tile[0] * c.tile[0]
        f = f.clone()
        f[m0:c.M - 1] = f[m0 + 1:c.M].clone()
        return f


class WritesRowPastM(G.TorchGemm):
    def write(self, g, v, rows=None, N=None):
        super().write(g, v, rows, N)
        if rows is None:
            g.buf[g.lo + g.n:g.lo + g.n + v.shape[1]] = v[-1]


class SkipsLastColumns(G.TorchGemm):
    def write(self, g, v, rows=None, N=None):
        keep = g.view[:, v.shape[1] - 8:v.shape[1]].clone() if rows is None else None
        super().write(g, v, rows, N)
        if rows is None:
            g.view[:, v.shape[1] - 8:v.shape[1]] = keep


class RoundsTwice(G.TorchGemm):
    """f32 -> 12 significant bits -> bf16"""

    def round_out(self, v, dtype):
        if dtype == torch.bfloat16:
            m, e = torch.frexp(v)
            v = torch.ldexp(torch.round(m * 4096) / 4096, e)
        return v.to(dtype)


class AddsRaggedStepTwice(G.TorchGemm):
    def tn_product(self, dY, X, c, t0, t1, last):
        p = super().tn_product(dY, X, c, t0, t1, last)
        r0 = (c.T - 1) // c.step * c.step
        if last and c.T % c.step and t1 == c.T and r0 >= t0:
            p = p + super().tn_product(dY, X, c, r0, t1, last)
        return p


def rejected(impl, c):
    try:
        G.check_nt(impl, c)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant,case", [(DropsLastK, M_STORE), (ShiftsBias, M_STORE), (NeighbourFactor, M_ROWSCALE)])
def test_faults_the_old_metric_cannot_see(mutant, case):
    """rejected by the exact checker, accepted by max|got - ref| / max|ref| at the bound of the random-operand tests"""
    G.check_nt(IMPL, case)
    assert rejected(mutant(), case)
    rc, o = mutant().nt(case, G.nt_inputs(case))
    assert G.old_metric_passes(case, o), "the fault is meant to be one the old bound lets through"
    assert G.old_metric_passes(case, IMPL.nt(case, G.nt_inputs(case))[1])


@pytest.mark.parametrize("mutant,case", [(DropsLastK, M_PARTIAL), (DropsLastK, M_FULL), (ShiftsBias, replace(M_FULL, M=1, N=136, fam="ternary")),
                                         (NeighbourFactor, replace(M_ROWSCALE, resid_mul=1, inplace=True)),
                                         (WritesRowPastM, M_STORE), (WritesRowPastM, replace(M_ROWSCALE, pad=8)),
                                         (WritesRowPastM, NT(dt=PA_BF16, epi=GELU, M=33, N=136, K=128, scale=0.125)),
                                         (SkipsLastColumns, M_STORE), (SkipsLastColumns, replace(M_ROWSCALE, inplace=False)),
                                         (SkipsLastColumns, NT(dt=PA_F32, epi=DGELU, M=33, N=136, K=64, aux="eighths")),
                                         (RoundsTwice, M_FULL), (RoundsTwice, replace(M_FULL, colscale_n=256, colscale=2.0))])
def test_faults_rejected(mutant, case):
    G.check_nt(IMPL, case)
    assert rejected(mutant(), case)


@pytest.mark.parametrize("c", [TN(PA_BF16, 341, 248, 264, 0, 2, "ternary", colsum=True), TN(PA_BF16, 49, 8, 8, 0, 1, "full"),
                               TN(PA_BF16, 97, 256, 256, 1, 2, "tag"), TN(PA_F32, 47, 264, 776, 0, 2, "ternary")])
def test_ragged_step_added_twice_is_rejected(c):
    G.check_tn(IMPL, c)
    with pytest.raises(AssertionError):
        G.check_tn(AddsRaggedStepTwice(), c)


def test_a_nan_behind_the_tokens_poisons_the_gradient():
    """the point of the NaN guard: one read past the last token and no element of the gradient survives"""
    class ReadsPastTheEnd(G.TorchGemm):
        def tn_product(self, dY, X, c, t0, t1, last):
            p = super().tn_product(dY, X, c, t0, t1, last)
            return p + float("nan") if last else p
    with pytest.raises(AssertionError):
        G.check_tn(ReadsPastTheEnd(), TN(PA_BF16, 49, 8, 8))


def test_inplace_and_remap_leave_the_other_rows_alone():
    c = NT(dt=PA_F32, epi=RESID, M=3 * 37, N=136, K=64, row_mod=37, fam="tag")

    class WritesEveryRow(G.TorchGemm):
        def write(self, g, v, rows=None, N=None):
            super().write(g, v, rows, N)
            g.view[0, :8] = 1.0
    G.check_nt(IMPL, c)
    assert rejected(WritesEveryRow(), c)

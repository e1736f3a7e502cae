"""The checkers of tests/attention_cases.py against plain torch (no GPU): an honest implementation of the specified arithmetic meets
every torch.equal and every bound; the case lists reach every structural edge of the kernels; and each of eight fault models -- plain
torch attention with ONE deliberate defect -- is rejected by the checkers, two of them while the max-over-max bound of
tests/test_gpu_kernels.py::test_attention_fwd_bwd accepts them on that test's own bf16 data."""
import pytest
import torch

from tests import attention_cases as A
from tests.attention_cases import PA_BF16, PA_F32, PRE, SINGLE_PASS, SINGLE_PASS_W16, TWO_PASS, AC, TorchAttention

_WORST = {}


def rec(group, ratio):
    _WORST[group] = max(_WORST.get(group, 0.0), ratio)


# ---- the lists -----------------------------------------------------------------------------------------------------------
def test_sign_codes_are_far_apart():
    codes = A.sign_codes()
    assert codes.shape == (A.NCODES, 64) and A.NCODES >= max(A.N_PAIR_FORMS) and bool((codes.abs() == 1).all())
    assert A.min_hamming(codes) >= A.MIN_HAMMING               # every other score 16 * 12 = 192 below the hot one
    h = A.hadamard()
    assert torch.equal(h @ h.t(), 64 * torch.eye(64))


def test_lists_are_the_specified_ones():
    assert A.N_PAIR_FORMS == (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 257, 511, 512, 513, 1190)
    assert A.N_SINGLE == (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 479, 480, 481, 511, 512) and max(A.N_SINGLE) <= A.FK
    assert A.BHS == ((1, 1), (1, 7), (2, 4), (3, 3), (17, 1), (1, 12))
    assert A.NQ_N == (33, 130, 257) and A.NQS == (1, 2, 31, 32, 33, 127, 128, 129)
    assert A.PACKED[:4] == ((1, 33, 2, 129, 64, 1), (300, 1), (65, 128, 32), (257,)) and A.PACKED[4:] == ((33, 1, 65),)
    assert (A.PAD_QKV, A.PAD_DQKV, A.PAD_O) == (8, 16, 24)      # all different, all 16-byte steps in bf16 and f32
    assert A.EPS == 2.0 ** -14 and A.U == 2.0 ** -8 and A.SCALE == 0.125


def test_coverage_of_the_fixed_length_lists():
    fixed = [c for N in A.N_PAIR_FORMS for c in A.pair_form_cases(N)] + [c for N in A.N_SINGLE for c in A.single_cases(N)]
    for N in set(A.N_PAIR_FORMS) | set(A.N_SINGLE):
        assert any(c.N == N and (c.B * c.H) % 8 for c in fixed), f"N = {N} never runs with B H off a multiple of 8"
    for bh in A.BHS:
        assert any((c.B, c.H) == bh and c.N > 128 for c in fixed), f"(B, H) = {bh} never runs several blocks per head"
    assert all(c.B * c.H <= 3 for c in fixed if c.N == 1190)
    for N in A.N_PAIR_FORMS:
        cs = A.pair_form_cases(N)
        want = set(A.FAMILIES) - ({"pair"} if N < 2 else set())
        for dt in (PA_F32, PA_BF16):
            for pre in (0, PRE):
                got = [c for c in cs if c.dt == dt and c.flags & PRE == pre]
                assert {c.fam for c in got} == want and all(A.bwd_form(c) == "two_pass" for c in got), (N, dt, pre)
                assert any(c.fam == "select" and c.oshift for c in got) and any(c.fam == "select" and not c.oshift for c in got)
        assert all(c.flags & TWO_PASS for c in cs if c.dt == PA_BF16 and c.pre)
    for N in A.N_SINGLE:
        cs = A.single_cases(N)
        assert all(c.dt == PA_BF16 and c.pre for c in cs)
        assert {c.flags & ~PRE for c in cs} == {SINGLE_PASS, SINGLE_PASS_W16, 0}
        assert {A.bwd_form(c) for c in cs if c.flags & SINGLE_PASS} == {"single"}
        assert {A.bwd_form(c) for c in cs if c.flags & SINGLE_PASS_W16} == {"single_w16"}
        assert {A.bwd_form(c) for c in cs if c.flags == PRE} == ({"two_pass", "single"} if N in A.LIBRARY_SINGLE_N else {"two_pass"})
        for f in (SINGLE_PASS, SINGLE_PASS_W16, 0):
            assert {c.fam for c in cs if c.flags & ~PRE == f} == set(A.FAMILIES) - ({"pair"} if N < 2 else set())
    sel = [c for c in fixed if c.fam == "select" and not c.oshift]
    assert 0.4 <= sum(c.many for c in sel) / len(sel) <= 0.6       # one half permutations, one half many-to-one
    assert all(c.B * c.H * c.N * c.N <= 17 * 513 * 513 for c in fixed)      # every case stays small


def test_coverage_of_prefix_and_packed_lists():
    for N in A.NQ_N:
        cs = A.prefix_cases(N)
        assert {c.nq for c in cs} == {q for q in A.NQS + (N - 1,) if q < N}
        assert {c.dt for c in cs} == {PA_F32, PA_BF16} and {c.flags for c in cs} == {0, PRE}
        assert all(not c.all_q and c.o_rows == c.B * c.nq for c in cs)          # compact o, d_o and lse
    for lens in A.PACKED:
        cs = A.packed_cases(lens)
        assert {c.nq for c in cs} == {0, 2} and {c.dt for c in cs} == {PA_F32, PA_BF16} and {c.flags for c in cs} == {0, PRE}
        assert all(c.seq == lens and c.T == sum(lens) for c in cs)
    # a length-1 sequence at the start, in the middle and at the end of a batch
    assert any(l[0] == 1 for l in A.PACKED) and any(l[-1] == 1 and len(l) > 1 for l in A.PACKED)
    assert any(1 in l[1:-1] for l in A.PACKED)
    c = A.packed_cases(A.PACKED[0])[0]
    assert c.fam == "select"
    maps = [i["map"] for i in A.attn_inputs(c)["info"]]
    keys = [A.from_rows(A.attn_inputs(c)["k"], c, b, "tok")[0, 0] for b in range(c.B)]
    assert len(maps) == c.B and not torch.equal(keys[0], keys[5])          # every sequence has its own keys and its own map


@pytest.mark.parametrize("N", (1, 2, 33, 64, 65, 129, 300, 512, 1190))
def test_edge_positions(N):
    e, hot = A.edge_positions(N), A.hot_positions(N)
    assert 0 in e and N - 1 in e and all(t - 1 in e and t in e for t in range(32, N, 32))
    assert set(e) <= set(hot) and len(hot) == min(N, 128) and len(set(hot)) == len(hot)
    m = A.select_map(N, True, torch.Generator().manual_seed(0), 3)
    assert set(m.tolist()) == set(e) or N < len(e)


# ---- an honest implementation passes -------------------------------------------------------------------------------------
def _sample(cases, k):
    return cases[k % 5::5]


@pytest.mark.parametrize("N", A.N_PAIR_FORMS)
def test_torch_passes_forward_and_kernel_pair(N):
    for c in _sample(A.pair_form_cases(N), N):
        A.check_attention(TorchAttention(), c, rec)


@pytest.mark.parametrize("N", A.N_SINGLE)
def test_torch_passes_single_pass_cases(N):
    for c in _sample(A.single_cases(N), N):
        A.check_attention(TorchAttention(), c, rec)


@pytest.mark.parametrize("N", A.NQ_N)
def test_torch_passes_prefix_cases(N):
    for c in _sample(A.prefix_cases(N), N):
        A.check_attention(TorchAttention(), c, rec)


@pytest.mark.parametrize("lens", A.PACKED, ids=lambda x: "-".join(map(str, x)))
def test_torch_passes_packed_cases(lens):
    for c in A.packed_cases(lens)[::2]:
        A.check_attention(TorchAttention(), c, rec)


def test_torch_passes_sibling_cases():
    for c in A.sibling_cases():
        A.check_siblings(TorchAttention(), c, rec)


@pytest.mark.parametrize("N", (33, 128, 300, 512, 1190))
def test_pair_family_is_bit_exact_in_bf16(N):
    """the bf16 emulation reproduces the f64 result rounded once, bit for bit, in o, dq, dk and dv (check_attention uses torch.equal)"""
    for flags in (0, PRE):
        A.check_attention(TorchAttention(), AC(PA_BF16, 1, 2 if N < 1000 else 1, N, "pair", flags, seed=N))


# ---- fault models --------------------------------------------------------------------------------------------------------
class DropLastKey(TorchAttention):
    """the forward drops the last key of the last tile"""
    def n_keys(self, c, b, phase):
        return max(c.seq[b] - 1, 1) if phase == "fwd" else c.seq[b]


class UnmaskedTail(TorchAttention):
    """keys past N are not masked: the rest of the last 64-key tile counts as copies of row N - 1"""
    def keys(self, c, b, k, v, phase):
        extra = -c.seq[b] % 64
        return (torch.cat([k, k[:, -1:].expand(-1, extra, -1)], 1), torch.cat([v, v[:, -1:].expand(-1, extra, -1)], 1))


class NextHeadLastQueryTile(TorchAttention):
    """the rows of the last 32-query tile are taken from the next head"""
    def queries(self, c, b, qkv3, phase):
        q = qkv3[0][:, :c.nq_b(b)].clone()
        t0 = (c.nq_b(b) - 1) // 32 * 32
        q[:, t0:] = q.roll(-1, 0)[:, t0:]
        return q


class OReadWithLdqkv(TorchAttention):
    """the backward reads o with ldqkv"""
    def o_for_delta(self, c, o_dense, o_f32, b):
        flat = torch.cat([torch.nan_to_num(o_dense.float()).reshape(-1), torch.zeros(2 * o_dense.numel())])
        rows = (torch.arange(c.o_rows) * 3 * c.D)[:, None] + torch.arange(c.D)[None, :]
        return A.from_rows(flat[rows], c, b, "o")


class DvLastBlockNotWritten(TorchAttention):
    """dV of the last 32-key block is not written"""
    def dv_rows(self, c, b):
        return (c.seq[b] - 1) // 32 * 32


class KeyCountFromNq(TorchAttention):
    """the key count is taken from nq in the prefix form"""
    def n_keys(self, c, b, phase):
        return c.nq_b(b)


class FlushSmallP(TorchAttention):
    """probabilities below 2^-9 are flushed in bf16"""
    def p_lp(self, P, td):
        return A.lp(torch.where(P < 2.0 ** -9, torch.zeros_like(P), P), td)


class DeltaFromF32O(TorchAttention):
    """delta is formed from the forward's own f32 o instead of the stored one"""
    def o_for_delta(self, c, o_dense, o_f32, b):
        return o_f32[b]


_B = PA_BF16
# (model, cases of the lists' kinds that must reject it)
FAULTS = (
    (DropLastKey, (AC(_B, 1, 3, 65, "select", PRE), AC(_B, 1, 3, 65, "uniform"), AC(PA_F32, 1, 3, 474, "graded"))),
    (UnmaskedTail, (AC(_B, 1, 3, 65, "uniform", PRE), AC(PA_F32, 1, 3, 65, "select", many=True), AC(_B, 1, 3, 474, "graded"))),
    (NextHeadLastQueryTile, (AC(_B, 1, 7, 65, "select"), AC(PA_F32, 1, 7, 65, "pair", PRE))),
    (OReadWithLdqkv, (AC(_B, 1, 3, 33, "select", oshift=True), AC(_B, 1, 3, 65, "pair"))),
    (DvLastBlockNotWritten, (AC(_B, 1, 3, 65, "select"), AC(PA_F32, 1, 3, 64, "pair"))),
    (KeyCountFromNq, (AC(_B, 1, 3, 33, "select", nq=2), AC(PA_F32, 2, 1, 33, "uniform", nq=31))),
    (FlushSmallP, (AC(_B, 1, 1, 1190, "uniform"), AC(_B, 1, 3, 513, "graded", PRE))),
    (DeltaFromF32O, (AC(_B, 1, 3, 65, "select", oshift=True), AC(PA_F32, 1, 3, 65, "select", PRE, oshift=True))),
)
# the models the per-call max-over-max bound of test_attention_fwd_bwd lets through on its own bf16 data, (B, H, N) = (1, 3, 474)
# (the unwritten dV rows are 0.03 of max|dV|, which the spiked key sets; the lost key moves one row of o by 1.7e-2, just over the old
# 1.5e-2, and is accepted at most other seeds; KeyCountFromNq needs a prefix, which that test does not have)
OLD_BOUND_ACCEPTS = {"DvLastBlockNotWritten", "DeltaFromF32O"}


@pytest.mark.parametrize("model,cases", FAULTS, ids=lambda x: x.__name__ if isinstance(x, type) else "")
def test_fault_model_is_rejected(model, cases):
    for c in cases:
        A.check_attention(TorchAttention(), c)                 # the case itself is one an honest implementation passes
        with pytest.raises(AssertionError):
            A.check_attention(model(), c)


def _dense(impl, c):
    """o and dqkv of one forward + backward as the old test saw them: dense, unwritten elements 0"""
    i = A.attn_inputs(c)
    _, f = impl.fwd(c, i["qkv"])
    o = f["o"].view[:, :c.D].clone()
    lse = f["lse"].view.clone()
    _, g = impl.bwd(c, i["qkv"], o, i["d_o"], lse)
    d = g["dqkv"].view[:, :3 * c.D].clone()
    d[d == A.SENTINEL] = 0
    return o, d


def test_old_bound_accepts_what_the_new_checkers_reject():
    c = AC(PA_BF16, 1, 3, 474, "graded", PRE | TWO_PASS)
    assert A.old_metric_passes(c, *_dense(TorchAttention(), c))
    accepted = set()
    for model, _ in FAULTS:
        if model is not KeyCountFromNq and A.old_metric_passes(c, *_dense(model(), c)):
            accepted.add(model.__name__)
    assert accepted == OLD_BOUND_ACCEPTS, accepted
    for name in ("DvLastBlockNotWritten",):      # ... and the per-element bounds reject them on the very same data
        with pytest.raises(AssertionError):
            A.check_attention(dict((m.__name__, m) for m, _ in FAULTS)[name](), c)


def test_worst_ratios_of_the_emulation_stay_below_one():
    """runs last in this file: every got / bound the emulation reached (profiles/attention_exact_parity.txt keeps the figures)"""
    assert all(0 <= v <= 1 for v in _WORST.values()), _WORST

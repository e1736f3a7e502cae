"""The 16x16x32 K loop of the role-split NT kernels on the device, through ops.gemm_nt, on the forced role-split tunes and the
default pick.

One-hot operands: A[m][k] = 1 iff k == (7 m + 3) % K, B[n][k] = ((5 n + 3 k) % 17) - 8, so out[m][n] = B[n][(7 m + 3) % K] exactly
in bf16 -- and again with the roles of A and B exchanged.  A misplaced row, column or k-block (a wrong LDS swizzle, a wrong half of
the four-MFMA decomposition, the other pairing of the lane swap) shows as a wrong integer.  Then the exact-integer operand families
of tests/gemm_cases.py through every epilogue.  Every call is made twice and the two results compared bit for bit."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib, ops  # noqa: E402
from tests import gemm_cases as G  # noqa: E402
from tests.gemm_cases import DGELU, GELU, PA_BF16, PA_OK, RESID, STORE, TD, GuardedOut  # noqa: E402

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
TUNES = (6, 7, 8, 17, 18, 0)              # 0: the default pick
# one partial tile, two K-tiles | odd K-tile count through the three-slot A ring | single K-tile (C = 0 start, A3 fallback, edge
# column tile) | 276 items at TM = 3: some workgroups walk a second item (cross-item DMA hand-over)
SHAPES = ((77, 192, 128), (333, 768, 192), (517, 520, 64), (4236, 3072, 128))
V3 = _lib.GEMM_EPILOGUE_V3


# ---- one-hot operands ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def onehot(M, N, K):
    """(A, B, expected) for both role assignments, on the device"""
    def hot(R):
        t = torch.zeros(R, K)
        t[torch.arange(R), (7 * torch.arange(R) + 3) % K] = 1
        return t

    def pat(R):
        return ((5 * torch.arange(R)[:, None] + 3 * torch.arange(K)[None, :]) % 17 - 8).float()

    out = []
    A, B = hot(M), pat(N)
    out.append((A, B, B[:, (7 * torch.arange(M) + 3) % K].t().contiguous()))
    A, B = pat(M), hot(N)
    out.append((A, B, A[:, (7 * torch.arange(N) + 3) % K].contiguous()))
    return [(a.to(BF16).to(DEV), b.to(BF16).to(DEV), e.to(DEV)) for a, b, e in out]


def unblock(buf, M, N):
    """row-major [M][N] of a blocked pre-activation (csrc/gemm.hip, V2Aux: one 4 KiB block per 32-row x 64-column pass, in the
    accumulator layout: [q][lane][dword][half] = register 2 (4 (q & 1) + dword) + half of column block q >> 1)"""
    R, C = (M + 31) // 32, N // 64
    t = buf.view(-1)[:R * C * 2048].view(R, C, 4, 64, 4, 2)
    q, lane, d, e = torch.meshgrid(torch.arange(4), torch.arange(64), torch.arange(4), torch.arange(2), indexing="ij")
    reg = 2 * (4 * (q & 1) + d) + e
    row = ((reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)).to(DEV)
    col = (32 * (q >> 1) + (lane & 31)).to(DEV)
    out = torch.empty(R, C, 32, 64, dtype=buf.dtype, device=DEV)
    out[:, :, row, col] = t
    return out.permute(0, 2, 1, 3).reshape(R * 32, N)[:M]


def twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two launches of one call differ"
    return a


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("tune", TUNES)
def test_onehot(tune, M, N, K):
    for role, (A, B, want) in enumerate(onehot(M, N, K)):
        what = f"tune {tune}, {M}x{N}x{K}, role {role}"
        for flags in (0, V3):
            def store():
                o = torch.full((M, N), 99.0, device=DEV, dtype=BF16)
                ops.gemm_nt(A, B, PA_BF16, ops.EPI_STORE, out_lp=o, tune=tune, flags=flags)
                return (o,)

            def resid():
                o = torch.full((M, N), 99.0, device=DEV)
                ops.gemm_nt(A, B, PA_BF16, ops.EPI_RESID, resid=torch.zeros(M, N, device=DEV), out_f32=o, tune=tune, flags=flags)
                return (o,)

            def gelu():
                pre, act = torch.full((M, N), 99.0, device=DEV, dtype=BF16), torch.empty(M, N, device=DEV, dtype=BF16)
                ops.gemm_nt(A, B, PA_BF16, ops.EPI_GELU, out_lp=pre, out_lp2=act, tune=tune, flags=flags)
                return pre, act

            assert torch.equal(twice(store)[0].float(), want), f"STORE, {what}, flags {flags:#x}"
            assert torch.equal(twice(resid)[0], want), f"RESID, {what}, flags {flags:#x}"
            assert torch.equal(twice(gelu)[0].float(), want), f"GELU pre, {what}, flags {flags:#x}"
        # blocked pre-activation: the forced role-split tunes have the form for N % 64 == 0, the default pick where the library says so
        if N % 64 == 0 and (tune or ops.blocked_pre_ok(M, N, K)):
            n = _lib.load().pa_gemm_blocked_pre_elems(M, N)

            def blocked():
                buf, act = torch.full((n,), 99.0, device=DEV, dtype=BF16), torch.empty(M, N, device=DEV, dtype=BF16)
                ops.gemm_nt(A, B, PA_BF16, ops.EPI_GELU, out_lp=buf.view(-1, N), out_lp2=act, tune=tune or None, flags=ops.GEMM_BLOCKED_PRE)
                return buf[:(M + 31) // 32 * 32 * N], act
            assert torch.equal(unblock(twice(blocked)[0], M, N).float(), want), f"GELU blocked pre, {what}"


# ---- exact-integer operands through every epilogue ---------------------------------------------------------------------------
class OpsGemm:
    """ops.gemm_nt behind the calling convention of gemm_cases.check_nt: guarded outputs; every call made twice"""
    name = "ops"

    def nt(self, c, i):
        td = TD[c.dt]
        A, B = i["A"].to(DEV), i["B"].to(DEV)
        bias = i["bias"].to(DEV) if i["bias"] is not None else None
        kw = dict(bias=bias, tune=c.tune or None, flags=c.flags)
        if c.entry == "splitk":
            assert not c.tune and ops._splitk_ws_floats(c.M, c.N, c.K, c.epi, c.dt) > 0, "the case must reach the split-K entry"
        runs = []
        for _ in range(2):
            outs = {}
            if c.epi == STORE:
                outs["out_lp"] = G.new_out(c.M, c.N, 0, td, DEV)
                ops.gemm_nt(A, B, c.dt, c.epi, out_lp=outs["out_lp"].view, colscale_n=c.colscale_n, colscale=c.colscale, **kw)
            elif c.epi == GELU:
                outs["out_lp"], outs["out_lp2"] = G.new_out(c.M, c.N, 0, td, DEV), G.new_out(c.M, c.N, 0, td, DEV)
                ops.gemm_nt(A, B, c.dt, c.epi, out_lp=outs["out_lp"].view, out_lp2=outs["out_lp2"].view, **kw)
            elif c.epi == RESID:
                outs["out_f32"] = G.new_out(c.M, c.N, 0, F32, DEV)
                ops.gemm_nt(A, B, c.dt, c.epi, resid=i["resid"].to(DEV), out_f32=outs["out_f32"].view,
                            rowscale=i["rowscale"].to(DEV) if c.factors else None, **kw)
            else:
                outs["out_lp"] = G.new_out(c.M, c.N, 0, td, DEV)
                outs["colsum"] = GuardedOut(c.N, F32, DEV)
                ops.gemm_nt(A, B, c.dt, c.epi, aux=i["aux"].to(DEV), out_lp=outs["out_lp"].view, colsum_out=outs["colsum"].view,
                            colsum_ws=ops.gemm_colsum_ws(c.M, c.N, DEV), **kw)
            runs.append(outs)
        torch.cuda.synchronize()
        for k in runs[0]:
            assert torch.equal(runs[0][k].buf, runs[1][k].buf), f"{c.name}: two launches of one call differ in {k}"
        return PA_OK, runs[0]


def exact_cases(tune, M, N, K):
    base = dict(dt=PA_BF16, M=M, N=N, K=K, tune=tune)
    return [G.NT(epi=STORE, colscale_n=64, colscale=0.5, **base), G.NT(epi=STORE, fam="full", **base),
            G.NT(epi=GELU, scale=0.125, **base),
            G.NT(epi=DGELU, colsum="set", **base),
            G.NT(epi=RESID, fam="full", factors=True, entry="rowscale", **base), G.NT(epi=RESID, fam="tag", **base)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("tune", TUNES)
def test_exact_integers_every_epilogue(tune, M, N, K):
    impl = OpsGemm()
    for c in exact_cases(tune, M, N, K):
        G.check_nt(impl, c)
        if tune:                          # the LDS-free epilogues (transposed accumulators) where the variant has them
            G.check_nt(impl, G.replace(c, flags=G.EPILOGUE_V3))


def test_exact_integers_splitk_entry():
    impl = OpsGemm()
    base = dict(dt=PA_BF16, M=128, N=768, K=2304, entry="splitk")
    for c in (G.NT(epi=STORE, colscale_n=64, colscale=0.5, **base), G.NT(epi=RESID, **base),
              G.NT(epi=RESID, factors=True, **base)):
        G.check_nt(impl, c)

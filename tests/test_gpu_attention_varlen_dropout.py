"""pa_attention_fwd_varlen_dropout / pa_attention_bwd_varlen_dropout on the device, through the C ABI, against the FIXED dropout entries.

The mask rule does not depend on N, and the packed kernels run the fixed kernels' tile loop per sequence with s = b*H + h and q, k local
to the sequence.  So sequence b of a packed launch must equal, bit for bit, sequence b of pa_attention_fwd_dropout /
pa_attention_bwd_dropout run at B = b + 1, N = N_b with the clip's rows in slot b under the same seed / site / t: o, lse and the three
thirds of dqkv are compared with torch.equal, no tolerance.  A wrong s, a q or k taken from the packed row index, or a row read from a
neighbour all break the equality (the other slots of the fixed batch hold different data).

Buffers: every operand has NaN rows behind its last row (behind cu_tok[B] for the packed ones) and NaN in the gap columns of a padded
leading dimension; every output and the workspace start as NaN, rows behind the last one included.  After a launch everything the
header promises is finite and everything else is still NaN.

Every test fails on the parent commit at the missing symbol pa_attention_fwd_varlen_dropout."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from tests import attention_cases as A  # noqa: E402
from tests import attention_dropout_cases as DR  # noqa: E402
from tests.attention_cases import PA_BF16, PA_EINVAL, PA_F32, PA_OK, PRE, SCALE, TD  # noqa: E402

DEV = "cuda"
LENS = (1, 33, 64, 65, 130, 257)      # one token; both sides of the 64-row tile; both sides of the 128-row block; several blocks
H, D = 2, 2 * A.HD
B, TOTAL, MAX_N = len(LENS), sum(LENS), max(LENS)
CU = [0]
for _n in LENS:
    CU.append(CU[-1] + _n)
TS = (64, 128)
SITE = 3
TAIL = 4                              # NaN rows behind every 2-D buffer
NAN = float("nan")


def seed_words(seed=DR.SEED):
    return torch.tensor([v - 2 ** 32 if v >= 2 ** 31 else v for v in seed], dtype=torch.int32, device=DEV)


def nan_rows(rows, cols, pad, td, data=None):
    """[rows + TAIL][cols + pad] of NaN on the device, rows [0, rows) x [0, cols) holding ``data`` when given"""
    buf = torch.full((rows + TAIL, cols + pad), NAN, dtype=td)
    if data is not None:
        buf[:rows, :cols] = data.to(td)
    return buf.to(DEV)


def nan_flat(n, data=None):
    buf = torch.full((n + 64,), NAN, dtype=torch.float32)
    if data is not None:
        buf[:n] = data
    return buf.to(DEV)


def bits(x):
    """the raw words of a tensor: equality that also holds for NaN"""
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def operands(dt, nq_full):
    """qkv [TOTAL][3D] and d_o ([TOTAL][D], or compact [2 B][D]) in the launch's type, as CPU tensors"""
    g = torch.Generator().manual_seed(1000 + dt + 2 * nq_full)
    qkv = torch.randn(TOTAL, 3 * D, generator=g).to(TD[dt])
    d_o = torch.randn(TOTAL if nq_full else 2 * B, D, generator=g).to(TD[dt])
    return qkv, d_o


class Run:
    def __init__(self):
        self.lib = _lib.load()
        self.st = torch.cuda.current_stream().cuda_stream
        self.cu = torch.tensor(CU, dtype=torch.int32, device=DEV)
        self.seed = seed_words()

    # ---- packed ----------------------------------------------------------------------------------------------------------
    def packed_fwd(self, dt, flags, t, nq, qkv, plain=False, seed="own", site=SITE, cu="own"):
        full = nq >= MAX_N
        q = nan_rows(TOTAL, 3 * D, A.PAD_QKV, TD[dt], qkv)
        o = nan_rows(TOTAL if full else B * nq, D, A.PAD_O, TD[dt])
        lse = nan_flat(H * TOTAL if full else B * H * nq)
        cu = self.cu.data_ptr() if cu == "own" else cu
        if plain:
            rc = self.lib.pa_attention_fwd_varlen(q.data_ptr(), 3 * D + A.PAD_QKV, o.data_ptr(), D + A.PAD_O, lse.data_ptr(), cu, B, H, MAX_N, nq,
                                                  SCALE, dt, flags, self.st)
        else:
            sd = self.seed.data_ptr() if seed == "own" else seed
            rc = self.lib.pa_attention_fwd_varlen_dropout(q.data_ptr(), 3 * D + A.PAD_QKV, o.data_ptr(), D + A.PAD_O, lse.data_ptr(), cu, B, H,
                                                          MAX_N, nq, SCALE, dt, flags, sd, site, t, self.st)
        torch.cuda.synchronize()
        return rc, q, o.cpu(), lse.cpu()

    def packed_bwd(self, dt, flags, t, nq, q, o, lse, d_o, seed="own", site=SITE):
        full = nq >= MAX_N
        rows = TOTAL if full else B * nq
        od, dod = o.to(DEV), nan_rows(rows, D, A.PAD_O, TD[dt], d_o)
        lsed = lse.to(DEV)
        need = self.lib.pa_attention_bwd_varlen_ws_floats(TOTAL, B, H, nq)
        ws = nan_flat(need)
        g = nan_rows(TOTAL, 3 * D, A.PAD_DQKV, TD[dt])
        sd = self.seed.data_ptr() if seed == "own" else seed
        rc = self.lib.pa_attention_bwd_varlen_dropout(q.data_ptr(), 3 * D + A.PAD_QKV, od.data_ptr(), dod.data_ptr(), D + A.PAD_O, lsed.data_ptr(),
                                                      ws.data_ptr(), g.data_ptr(), 3 * D + A.PAD_DQKV, self.cu.data_ptr(), B, H, MAX_N, nq, SCALE,
                                                      dt, flags, sd, site, t, self.st)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws[need:]).all()), "a write behind the workspace"
        return rc, g.cpu()

    # ---- the fixed entries at B = b + 1, N = N_b, the clip in slot b ------------------------------------------------------------
    def fixed(self, dt, flags, t, nq, b, qkv, d_o):
        """(o [nq_b][D], lse [H][nq_b], dqkv [N_b][3D]) of slot b"""
        N, Bf = LENS[b], b + 1
        nqb = min(nq, N)
        g = torch.Generator().manual_seed(77 + b)
        qf = torch.randn(Bf * N, 3 * D, generator=g)                 # the other slots: other data
        qf[b * N:] = qkv[CU[b]:CU[b + 1]].float()
        dof = torch.randn(Bf * nqb, D, generator=g)
        dof[b * nqb:] = (d_o[CU[b]:CU[b + 1]] if nq >= MAX_N else d_o[b * nq:b * nq + nqb]).float()
        q = nan_rows(Bf * N, 3 * D, A.PAD_QKV, TD[dt], qf)
        o = nan_rows(Bf * nqb, D, A.PAD_O, TD[dt])
        lse = nan_flat(Bf * H * nqb)
        rc = self.lib.pa_attention_fwd_dropout(q.data_ptr(), 3 * D + A.PAD_QKV, o.data_ptr(), D + A.PAD_O, lse.data_ptr(), Bf, H, N, nqb, SCALE, dt,
                                               flags, self.seed.data_ptr(), SITE, t, self.st)
        assert rc == PA_OK
        dod = nan_rows(Bf * nqb, D, A.PAD_O, TD[dt], dof)
        ws = nan_flat(self.lib.pa_attention_bwd_ws_floats(Bf, H, nqb))
        # the fixed entry leaves the Q third of rows q >= nq to its caller (pa_zero2d); the packed one writes zero there
        dq = torch.zeros((Bf * N + TAIL, 3 * D + A.PAD_DQKV), dtype=TD[dt], device=DEV)
        rc = self.lib.pa_attention_bwd_dropout(q.data_ptr(), 3 * D + A.PAD_QKV, o.data_ptr(), dod.data_ptr(), D + A.PAD_O, lse.data_ptr(), ws.data_ptr(),
                                               dq.data_ptr(), 3 * D + A.PAD_DQKV, Bf, H, N, nqb, SCALE, dt, flags, self.seed.data_ptr(), SITE, t,
                                               self.st)
        assert rc == PA_OK
        torch.cuda.synchronize()
        return (o.cpu()[b * nqb:Bf * nqb, :D], lse.cpu()[:Bf * H * nqb].view(Bf, H, nqb)[b], dq.cpu()[b * N:Bf * N, :3 * D])


@pytest.fixture(scope="module")
def run():
    return Run()


def owned_fwd(nq, o, lse, what):
    """the packed forward's o / lse split per sequence after the buffer checks: owned finite, everything else still NaN"""
    full = nq >= MAX_N
    rows = TOTAL if full else B * nq
    assert bool(torch.isnan(o[rows:]).all()), f"{what}: o written behind its last row"
    assert bool(torch.isnan(o[:, D:]).all()), f"{what}: o written in the gap columns"
    n_lse = H * TOTAL if full else B * H * nq
    assert bool(torch.isnan(lse[n_lse:]).all()), f"{what}: lse written behind its end"
    out = []
    for b, N in enumerate(LENS):
        nqb = min(nq, N)
        if full:
            ob, lb = o[CU[b]:CU[b + 1], :D], lse[:n_lse].view(H, TOTAL)[:, CU[b]:CU[b + 1]]
        else:
            ob, lb = o[b * nq:b * nq + nqb, :D], lse[:n_lse].view(B, H, nq)[b, :, :nqb]
            assert bool(torch.isnan(o[b * nq + nqb:(b + 1) * nq]).all()) and bool(torch.isnan(lse[:n_lse].view(B, H, nq)[b, :, nqb:]).all()), \
                f"{what}: rows of a sequence shorter than nq written"
        assert bool(torch.isfinite(ob.float()).all()) and bool(torch.isfinite(lb).all()), f"{what}: sequence {b} not finite"
        out.append((ob, lb))
    return out


def owned_bwd(g, what):
    assert bool(torch.isnan(g[TOTAL:].float()).all()), f"{what}: dqkv written at or behind row cu_tok[B]"
    assert bool(torch.isnan(g[:, 3 * D:].float()).all()), f"{what}: dqkv written in the gap columns"
    assert bool(torch.isfinite(g[:TOTAL, :3 * D].float()).all()), f"{what}: an owned element of dqkv is not finite"
    return [g[CU[b]:CU[b + 1], :3 * D] for b in range(B)]


@pytest.mark.parametrize("pre", (0, PRE), ids=("plainq", "prescaled"))
@pytest.mark.parametrize("dt", (PA_F32, PA_BF16), ids=("f32", "bf16"))
def test_every_sequence_equals_the_fixed_entry(run, dt, pre):
    for nq in (MAX_N, 2):
        qkv, d_o = operands(dt, nq >= MAX_N)
        for t in TS:
            what = f"dt{dt} pre{pre} nq{nq} t{t}"
            rc, q, o, lse = run.packed_fwd(dt, pre, t, nq, qkv)
            assert rc == PA_OK, what
            fwd = owned_fwd(nq, o, lse, what)
            rc, g = run.packed_bwd(dt, pre, t, nq, q, o, lse, d_o)
            assert rc == PA_OK, what
            bwd = owned_bwd(g, what)
            for b in range(B):
                fo, fl, fg = run.fixed(dt, pre, t, nq, b, qkv, d_o)
                assert torch.equal(fwd[b][0], fo), f"{what}: o of sequence {b}"
                assert torch.equal(fwd[b][1], fl), f"{what}: lse of sequence {b}"
                for third, name in enumerate(("dq", "dk", "dv")):
                    assert torch.equal(bwd[b][:, third * D:(third + 1) * D], fg[:, third * D:(third + 1) * D]), f"{what}: {name} of sequence {b}"
            # dropout is active: the output is not the plain entry's
            _, _, o0, _ = run.packed_fwd(dt, pre, t, nq, qkv, plain=True)
            assert not torch.equal(bits(o), bits(o0))


@pytest.mark.parametrize("pre", (0, PRE), ids=("plainq", "prescaled"))
@pytest.mark.parametrize("dt", (PA_F32, PA_BF16), ids=("f32", "bf16"))
def test_lse_is_the_plain_packed_entrys_bit_for_bit(run, dt, pre):
    """Dropout does not touch lse: it must equal pa_attention_fwd_varlen's lse on the same operands, bit for bit -- with the pre-scaled
    q and without it.  (Without it the plain instances form score * scale - max of their first key tile with one rounding; the dropout
    instances do the same, csrc/attention.hip "RAW".)"""
    for nq in (MAX_N, 2):
        qkv, _ = operands(dt, nq >= MAX_N)
        for t in TS:
            rc, _, _, lse = run.packed_fwd(dt, pre, t, nq, qkv)
            rc0, _, _, lse0 = run.packed_fwd(dt, pre, t, nq, qkv, plain=True)
            assert rc == PA_OK and rc0 == PA_OK
            n = H * TOTAL if nq >= MAX_N else B * H * nq
            a, b = lse[:n], lse0[:n]
            own = ~torch.isnan(b)
            ndiff = int((a[own] != b[own]).sum())
            worst = float((a[own] - b[own]).abs().max())
            print(f"lse vs pa_attention_fwd_varlen dt{dt} pre{pre} nq{nq} t{t}: {ndiff} of {int(own.sum())} entries differ, largest difference {worst:.3e}")
            assert torch.equal(bits(lse), bits(lse0)), f"dt{dt} pre{pre} nq{nq} t{t}: {ndiff} entries of lse differ from pa_attention_fwd_varlen's"


@pytest.mark.parametrize("nq", (MAX_N, 2))
def test_two_runs_are_bit_identical(run, nq):
    qkv, d_o = operands(PA_BF16, nq >= MAX_N)
    outs = []
    for _ in range(2):
        rc, q, o, lse = run.packed_fwd(PA_BF16, PRE, 64, nq, qkv)
        rc2, g = run.packed_bwd(PA_BF16, PRE, 64, nq, q, o, lse, d_o)
        assert rc == PA_OK and rc2 == PA_OK
        outs.append((o, lse, g))
    for x, y in zip(*outs):
        assert torch.equal(bits(x), bits(y))


def test_refusals_launch_nothing(run):
    """PA_EINVAL for what either parent entry refuses, and every output keeps its NaN"""
    qkv, d_o = operands(PA_F32, True)
    rc, q, o, lse = run.packed_fwd(PA_F32, 0, 64, MAX_N, qkv)
    assert rc == PA_OK
    for kw in (dict(t=0), dict(t=256), dict(t=-1), dict(seed=None), dict(site=65536), dict(cu=None), dict(flags=2), dict(nq=0)):
        a = dict(dt=PA_F32, flags=0, t=64, nq=MAX_N, qkv=qkv)
        a.update(kw)
        rc, _, o1, lse1 = run.packed_fwd(**a)
        assert rc == PA_EINVAL, kw
        assert bool(torch.isnan(o1).all()) and bool(torch.isnan(lse1).all()), (kw, "the forward wrote")
    for kw in (dict(t=0), dict(t=256), dict(seed=None), dict(site=65536), dict(flags=16)):
        a = dict(dt=PA_F32, flags=0, t=64, nq=MAX_N, q=q, o=o, lse=lse, d_o=d_o)
        a.update(kw)
        rc, g = run.packed_bwd(**a)
        assert rc == PA_EINVAL, kw
        assert bool(torch.isnan(g).all()), (kw, "the backward wrote")

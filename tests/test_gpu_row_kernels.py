"""Edge-shape and exact-sum parity of the row kernels -- LayerNorm, the head, the two losses and the partial-sum reductions --
through the C ABI, in guarded buffers (tests/row_kernel_cases.py holds the shapes, inputs, bounds and checkers; the same checkers
pass against plain f32 torch in tests/test_row_kernels_cpu.py).  Every measured figure goes to row_kernel_parity_metrics.json
in $PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root); profiles/row_kernel_parity.txt keeps the worst per
group."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from tests import row_kernel_cases as K  # noqa: E402
from tests.row_kernel_cases import PA_BF16, PA_F32, TD, GuardedOut  # noqa: E402

DEV = "cuda"
F32 = torch.float32
_METRICS = {}


def record(name, **kw):
    _METRICS[name] = {k: float(v) for k, v in kw.items()}
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_metrics")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "row_kernel_parity_metrics.json"), "w") as f:
        json.dump(_METRICS, f, indent=1, sort_keys=True)


def p(t):
    return None if t is None else t.data_ptr()


class Hip:
    """The C entries of libpasst_amd.so behind the calling conventions of row_kernel_cases.TorchF32: CPU tensors in, CPU
    tensors out, every device buffer guarded.  One instance per test: inputs are uploaded once per tensor."""
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self.st = torch.cuda.current_stream().cuda_stream
        self._up = {}

    def gin(self, t, offset=0):
        if t is None:
            return None
        k = (id(t), offset)
        if k not in self._up:
            self._up[k] = (t, K.guarded_in(t, DEV, offset))       # keeps `t` alive: ids stay unique
        return self._up[k][1]

    def ok(self, rc, what):
        assert rc == 0, f"{what}: code {rc} {self.lib.pa_last_hip_error().decode() if rc == -3 else ''}"

    # ---- LayerNorm
    def ln_fwd(self, x, g, b, eps, dt):
        M, D = x.shape
        y, mean, rstd = GuardedOut((M, D), TD[dt], DEV), GuardedOut(M, F32, DEV), GuardedOut(M, F32, DEV)
        self.ok(self.lib.pa_layernorm_fwd(p(self.gin(x)), p(self.gin(g)), p(self.gin(b)), y.ptr(), dt, mean.ptr(), rstd.ptr(), M, D, eps,
                                          self.st), "pa_layernorm_fwd")
        return y.take("y"), mean.take("mean"), rstd.take("rstd")

    def ln_bwd(self, dy, x, g, mean, rstd, dres, dres2, dt, eps=1e-6, partial=False, accumulate=False, start=None, want_dcol=True):
        lib, M, D = self.lib, x.shape[0], x.shape[1]
        rows = lib.pa_layernorm_bwd_rows(M)
        assert lib.pa_layernorm_bwd_ws_floats(M, D) == rows * 3 * D
        ws = GuardedOut(rows * 3 * D, F32, DEV)
        dx, lp = GuardedOut((M, D), F32, DEV), GuardedOut((M, D), TD[dt], DEV)
        init = (lambda j: start[j]) if accumulate else (lambda j: None)
        dg, db = GuardedOut(D, F32, DEV, init(0)), GuardedOut(D, F32, DEV, init(1))
        dcol = GuardedOut(D, F32, DEV, init(2)) if want_dcol else None
        a = [p(self.gin(dy)), dt, p(self.gin(x)), p(self.gin(g)), p(self.gin(mean)), p(self.gin(rstd)), p(self.gin(dres))]
        two = dres2 is not None
        if two:
            a.append(p(self.gin(dres2)))
        a += [dx.ptr(), lp.ptr()]
        if partial:
            fn = lib.pa_layernorm_bwd2_partial if two else lib.pa_layernorm_bwd_partial
            self.ok(fn(*a, ws.ptr(), M, D, self.st), "pa_layernorm_bwd*_partial")
            outs = [o for o in (dg, db, dcol)]
            descs = (_lib.ReduceDesc * 3)()
            n = 0
            for j, o in enumerate(outs):
                if o is not None:
                    descs[n] = _lib.ReduceDesc(ws.ptr() + 4 * j * D, o.ptr(), D, rows, int(accumulate), 3 * D, K.REDUCE_ROWS, 0)
                    n += 1
            self.ok(lib.pa_reduce_partials_batched(descs, n, self.st), "pa_reduce_partials_batched")
        else:
            fn = lib.pa_layernorm_bwd2 if two else lib.pa_layernorm_bwd
            self.ok(fn(*a, dg.ptr(), db.ptr(), dcol.ptr() if dcol else None, int(accumulate), ws.ptr(), M, D, self.st), "pa_layernorm_bwd*")
        ws.take("ws")
        return dict(dx=dx.take("dx"), dx_lp=lp.take("dx_lp"), dg=dg.take("dgamma"), db=db.take("dbeta"),
                    dcol=dcol.take("dcolsum") if dcol else None)

    # ---- head
    def head_fwd(self, x, ng, nb, hg, hb, eps_n=1e-6, eps_h=1e-5):
        B, Ntok, D = x.shape
        feat, hn, stats = GuardedOut((B, D), F32, DEV), GuardedOut((B, D), F32, DEV), GuardedOut((B, 6), F32, DEV)
        self.ok(self.lib.pa_head_pre_fwd(p(self.gin(x)), B, Ntok, D, p(self.gin(ng)), p(self.gin(nb)), eps_n, p(self.gin(hg)), p(self.gin(hb)),
                                         eps_h, feat.ptr(), hn.ptr(), stats.ptr(), self.st), "pa_head_pre_fwd")
        return feat.take("feat"), hn.take("hn"), stats.take("stats")

    def _head_bwd(self, dhn, dfeat, x, feat, ng, hg, stats):
        B, Ntok, D = x.shape
        dx, part = GuardedOut((B, Ntok, D), F32, DEV), GuardedOut((B, 4, D), F32, DEV)
        rc = self.lib.pa_head_pre_bwd(p(self.gin(dhn)), p(self.gin(dfeat)), p(self.gin(x)), p(self.gin(feat)), B, Ntok, D, p(self.gin(ng)),
                                      p(self.gin(hg)), p(self.gin(stats)), dx.ptr(), part.ptr(), self.st)
        return rc, dx, part

    def head_bwd(self, dhn, dfeat, x, feat, ng, hg, stats):
        rc, dx, part = self._head_bwd(dhn, dfeat, x, feat, ng, hg, stats)
        self.ok(rc, "pa_head_pre_bwd")
        return dx.take("dx"), part.take("part")

    def head_bwd_rc(self, dhn, dfeat, x, feat, ng, hg, stats):
        rc, dx, part = self._head_bwd(dhn, dfeat, x, feat, ng, hg, stats)
        dx.take("dx", written=0), part.take("part", written=0)          # a refused call writes nothing
        return rc

    # ---- head Linear
    def linear_fwd(self, x, W, b):
        B, D = x.shape
        C = W.shape[0]
        y = GuardedOut((B, C), F32, DEV)
        self.ok(self.lib.pa_linear_f32_fwd(p(self.gin(x)), p(self.gin(W)), p(self.gin(b)), y.ptr(), B, C, D, self.st), "pa_linear_f32_fwd")
        return y.take("y")

    def linear_bwd(self, dy, x, W, accumulate=False, start=None, want_dw=True):
        B, C = dy.shape
        D = x.shape[1]
        dx = GuardedOut((B, D), F32, DEV)
        dW = GuardedOut((C, D), F32, DEV, start[0] if accumulate else None) if want_dw else None
        db = GuardedOut(C, F32, DEV, start[1] if accumulate else None) if want_dw else None
        self.ok(self.lib.pa_linear_f32_bwd(p(self.gin(dy)), p(self.gin(x)), p(self.gin(W)), dx.ptr(), dW.ptr() if dW else None,
                                           db.ptr() if db else None, int(accumulate), B, C, D, self.st), "pa_linear_f32_bwd")
        return dx.take("dx"), dW.take("dW") if dW else None, db.take("db") if db else None

    # ---- losses
    def bce(self, z, y, scale):
        B, C = z.shape
        nblk = (B * C + 255) // 256
        loss, dz, ws = GuardedOut(1, F32, DEV), GuardedOut((B, C), F32, DEV), GuardedOut(1 + nblk, F32, DEV)
        self.ok(self.lib.pa_bce_fwd_bwd(p(self.gin(z)), p(self.gin(y)), B, C, scale, loss.ptr(), dz.ptr(), ws.ptr(), self.st), "pa_bce_fwd_bwd")
        ws.take("ws", written=nblk)
        return loss.take("loss"), dz.take("dlogits")

    def ce(self, z, t, t2, lam, scale):
        B, C = z.shape
        loss, dz, ws = GuardedOut(1, F32, DEV), GuardedOut((B, C), F32, DEV), GuardedOut(B, F32, DEV)
        self.ok(self.lib.pa_ce_mixup_fwd_bwd(p(self.gin(z)), p(self.gin(t)), p(self.gin(t2)), p(self.gin(lam)), B, C, scale, loss.ptr(), dz.ptr(),
                                             ws.ptr(), self.st), "pa_ce_mixup_fwd_bwd")
        ws.take("ws")
        return loss.take("loss"), dz.take("dlogits")

    # ---- reductions
    def reduce(self, descs, single=False, offsets=None):
        offsets = offsets or [(0, 0)] * len(descs)
        outs = [GuardedOut(d["n"], F32, DEV, d["start"] if d["accumulate"] else None, offset=o[0]) for d, o in zip(descs, offsets)]
        parts = [self.gin(d["partial"], o[1]) for d, o in zip(descs, offsets)]
        if single:
            (d,), (o,), (pt,) = descs, outs, parts
            assert d["mode"] == K.REDUCE_SLABS
            self.ok(self.lib.pa_reduce_partials(p(pt), d["splits"], d["n"], o.ptr(), d["accumulate"], self.st), "pa_reduce_partials")
        else:
            arr = (_lib.ReduceDesc * len(descs))()
            for j, (d, o, pt) in enumerate(zip(descs, outs, parts)):
                arr[j] = _lib.ReduceDesc(p(pt), o.ptr(), d["n"], d["splits"], d["accumulate"], d["pitch"], d["mode"], 0)
            self.ok(self.lib.pa_reduce_partials_batched(arr, len(descs), self.st), "pa_reduce_partials_batched")
        return [o.take("out") for o in outs]

    def colsum_f32(self, a, C, accumulate, start):
        out = GuardedOut(C, F32, DEV, start if accumulate else None)
        self.ok(self.lib.pa_colsum_f32(p(self.gin(a)), a.shape[0], C, a.shape[1], out.ptr(), accumulate, self.st), "pa_colsum_f32")
        return out.take("out")

    def _colsum(self, a, C, dt, accumulate, start):
        R, ld = a.shape
        out = GuardedOut(C, F32, DEV, start if accumulate else None)
        ws = GuardedOut(max(1, self.lib.pa_colsum_ws_floats(R, C)), F32, DEV)
        return self.lib.pa_colsum(p(self.gin(a)), dt, R, C, ld, out.ptr(), accumulate, ws.ptr(), self.st), out, ws

    def colsum(self, a, C, dt, accumulate, start):
        rc, out, ws = self._colsum(a, C, dt, accumulate, start)
        self.ok(rc, "pa_colsum")
        ws.take("ws")
        return out.take("out")

    def colsum_rc(self, a, C, dt):
        rc, out, ws = self._colsum(a, C, dt, 0, None)
        out.take("out", written=0), ws.take("ws", written=0)
        return rc

    def rowsum(self, a, C, dt, accumulate, start):
        R, ld = a.shape
        out = GuardedOut(R, F32, DEV, start if accumulate else None)
        self.ok(self.lib.pa_rowsum(p(self.gin(a)), dt, R, C, ld, out.ptr(), accumulate, self.st), "pa_rowsum")
        return out.take("out")


BASE = K.TorchF32()


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("D", K.LN_D)
def test_layernorm_every_instance_and_ragged_vector_column(dt, D):
    """instances 1, 2, 3, 4 and 8 float4 per lane, each with a full and a partly filled last vector column, forward and every
    backward entry; D >= 1368 needs more than 64 KiB of dynamic LDS in the backward"""
    K.check_layernorm(Hip(), K.LN_D_ROWS, D, dt, record)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M", list(K.LN_M_WORKGROUPS))
def test_layernorm_row_counts(dt, M):
    """idle waves (M < 4), the 16 / 17 and 64 / 65 partial-row boundaries of the finishing loop, the 1024-workgroup cap with a
    ragged last stride.  The workgroup count is asserted, so a change of launch geometry fails here instead of silently
    losing the coverage."""
    assert _lib.load().pa_layernorm_bwd_rows(M) == K.LN_M_WORKGROUPS[M]
    K.check_layernorm(Hip(), M, K.LN_M_WIDTH, dt, record)


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("M,D", K.LN_EXACT)
def test_layernorm_exact_sums(dt, M, D):
    K.check_ln_exact(Hip(), M, D, dt, record)


@pytest.mark.parametrize("M,D", K.LN_CONDITIONING_SHAPES)
@pytest.mark.parametrize("c,sigma", K.LN_CONDITIONING)
def test_layernorm_conditioning(c, sigma, M, D):
    K.check_ln_conditioning(Hip(), c, sigma, M, D, record, BASE)


@pytest.mark.parametrize("D", K.LN_CONSTANT_D)
def test_layernorm_constant_rows(D):
    K.check_ln_constant_rows(Hip(), D, record)


# ---- head ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Ntok,D", K.HEAD_SHAPES)
def test_head_pre(B, Ntok, D):
    """partly filled element slots (D = 64, 1100), full ones, Ntok = 2 (no rows to zero: the guard behind row 1 must hold)"""
    K.check_head(Hip(), B, Ntok, D, record)


def test_head_pre_width_not_a_multiple_of_four():
    impl = Hip()
    B, Ntok, D = K.HEAD_FWD_ONLY
    i, feat, hn, stats = K.check_head_fwd(impl, B, Ntok, D, record)
    assert impl.head_bwd_rc(i["dhn"], None, i["x"], feat, i["ng"], i["hg"], stats) == K.PA_EUNSUPPORTED


@pytest.mark.parametrize("B,C,D", K.LINEAR_SHAPES)
def test_head_linear(B, C, D):
    """C < 4 (idle class waves), D % 64 != 0, the two register-row forward instances (768, 1024) and the generic one"""
    K.check_linear(Hip(), B, C, D, record)


# ---- losses --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("B,C", K.BCE_SHAPES)
def test_bce(B, C, scale):
    """one element .. 268 partials (the second trip of the finishing loop), soft targets, a gradient scale"""
    K.check_bce(Hip(), B, C, scale, record, BASE)


@pytest.mark.parametrize("scale", [1.0, 0.125])
def test_bce_extreme_logits(scale):
    K.check_bce_extreme(Hip(), scale, record, BASE)


def test_bce_small_case_keeps_its_absolute_bound():
    K.check_bce_small(Hip(), record, BASE)


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("B,C", K.CE_SHAPES)
def test_ce_mixup(B, C, spread):
    """C > 64 (a second trip of the per-lane loops), B % 4 != 0, logits over +-80, lam = 0 and 1, coinciding targets"""
    K.check_ce(Hip(), B, C, spread, record, BASE)


# ---- reductions: exact sums, torch.equal -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.SLAB_N)
def test_reduce_slabs(n):
    for splits in K.SLAB_SPLITS:
        K.check_reduce_slabs(Hip(), splits, n)


@pytest.mark.parametrize("splits", K.ROWS_SPLITS)
def test_reduce_rows(splits):
    for n in K.ROWS_N:
        K.check_reduce_rows(Hip(), splits, n)


def test_reduce_rows_wider_than_the_grid():
    K.check_reduce_rows(Hip(), *K.ROWS_WIDE)


def test_reduce_batch_of_twelve_mixed_descriptors():
    K.check_reduce_batch(Hip())


@pytest.mark.parametrize("R", K.COLSUM_F32_R)
def test_colsum_f32(R):
    for C in K.COLSUM_F32_C:
        K.check_colsum_f32(Hip(), R, C)


@pytest.mark.parametrize("R", K.COLSUM_R)
def test_colsum(R):
    for C in K.COLSUM_C:
        K.check_colsum(Hip(), R, C)


def test_colsum_refuses_a_width_that_is_no_multiple_of_eight():
    for dt in (PA_F32, PA_BF16):
        assert Hip().colsum_rc(K.small_ints(5, 12, dtype=TD[dt]), 12, dt) == K.PA_EUNSUPPORTED


@pytest.mark.parametrize("C", K.ROWSUM_C)
def test_rowsum(C):
    for R in K.ROWSUM_R:
        K.check_rowsum(Hip(), R, C)

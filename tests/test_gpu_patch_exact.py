"""Exact-operand and guarded-buffer parity of the patch stage -- pa_patch_gather, pa_patch_pos_table, pa_patch_bwd, pa_patch_input_bwd
and their packed (_varlen) and packed-with-Patchout (_rows) forms -- and of the movers and casts beside it (pa_gather_rows,
pa_scatter_rows, pa_tail_inject, pa_zero2d, pa_transpose, pa_stage_weights, pa_convert_f32, pa_convert_f32_rowscale, pa_convert_to_f32)
through the C ABI, so that the test owns every buffer (tests/patch_cases.py holds the case lists, operand families, references and
checkers; the same checkers pass against plain f32 torch in tests/test_patch_cases_cpu.py).  Every copy, cast, integer sum and
ordered sum is compared with torch.equal; the worst got / bound of the one family that carries a bound (graded parameter-gradient
sums) goes to patch_exact_parity_metrics.json in $PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root);
profiles/patch_exact_parity.txt keeps them."""
import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from tests import patch_cases as P  # noqa: E402
from tests.patch_cases import I32, PA_BF16, PA_EINVAL, PA_F32, PA_OK, SENTINEL, TD  # noqa: E402
from tests.row_kernel_cases import GuardedOut, guarded_in  # noqa: E402

DEV = "cuda"
F32 = torch.float32
_METRICS = {}


def record(group, ratio):
    _METRICS[group] = max(_METRICS.get(group, 0.0), float(ratio))
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_metrics")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "patch_exact_parity_metrics.json"), "w") as f:
        json.dump({k: {"worst_got_over_bound": v} for k, v in _METRICS.items()}, f, indent=1, sort_keys=True)


def gin(t, offset=0):
    """`t` on the device inside a guarded allocation (guarded_in).  The tensor goes in flat and padded to a multiple of 8 elements, so
    the guard on either side is as long as the WHOLE operand (at least 256 elements) -- an access one row, one image plane, one clip
    or one patch off stays inside the allocation whatever the shape -- and the view is 16-byte aligned (plus `offset` elements)."""
    if t is None:
        return None
    n = t.numel()
    pad = -n % 8
    flat = t.reshape(-1)
    if pad:
        flat = torch.cat([flat, torch.full((pad,), float("nan") if t.is_floating_point() else 0, dtype=t.dtype)])
    return guarded_in(flat.view(1, -1), DEV, offset)[0, :n].view(t.shape)


class Out:
    """a GuardedOut of `shape`, laid out like gin(): flat, padded to a multiple of 8, guards as long as the output itself"""

    def __init__(self, shape, dtype, init=None, offset=0):
        self.shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        self.n = 1
        for d in self.shape:
            self.n *= d
        n8 = self.n + (-self.n % 8)
        full = None
        if init is not None:
            full = torch.full((1, n8), SENTINEL, dtype=dtype)
            full[0, :self.n] = init.reshape(-1)
        self.g = GuardedOut((1, n8), dtype, DEV, init=full, offset=offset)

    def ptr(self):
        return self.g.ptr()

    def take(self, what):
        """completely written, nothing outside it touched"""
        return self.g.take(what, written=self.n).reshape(-1)[:self.n].view(self.shape)

    def peek(self, what):
        """an output the entry writes only partly (or a workspace): the guards are checked, the contents returned as they are"""
        buf = self.g.buf.cpu()
        lo, n = self.g.lo, self.g.n
        assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + n:] == SENTINEL).all()), f"{what}: a write outside the buffer"
        assert bool((buf[lo + self.n:lo + n] == SENTINEL).all()), f"{what}: a write past the promised extent"
        return buf[lo:lo + self.n].view(self.shape).clone()

    def untouched(self, what):
        assert bool((self.g.buf == SENTINEL).all()), f"{what}: a refused call wrote"


def ptr(t):
    return None if t is None else t.data_ptr()


class Hip:
    """The C entries of libpasst_amd.so behind the calling conventions of patch_cases.TorchPatch: CPU tensors in, CPU tensors out.
    Every operand, index arrays and descriptor tables included, is a view into a larger allocation (NaN around floats, index 0
    around integers), every output and workspace a GuardedOut filled with the sentinel.  Nothing goes through passt_amd/ops.py."""
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self.st = torch.cuda.current_stream().cuda_stream

    def done(self):
        torch.cuda.synchronize()

    # -- the patch stage
    def gather(self, x, pf, pt, Pp, fs, ts, dt):
        B, F, T = x.shape
        Np = pf.numel()
        xd, pfd, ptd = gin(x), gin(pf), gin(pt)
        out = Out((B * Np, Pp * Pp), TD[dt])
        rc = self.lib.pa_patch_gather(ptr(xd), B, F, T, ptr(pfd), ptr(ptd), Np, Pp, fs, ts, out.ptr(), dt, self.st)
        self.done()
        return rc, out.take("cols")

    def gather_varlen(self, x, lay, Pp, fs, ts, dt):
        B, F, T = x.shape
        M = lay["M"]
        xd, rc_, rf, rt = gin(x), gin(lay["row_clip"]), gin(lay["row_f"]), gin(lay["row_t"])
        out = Out((M, Pp * Pp), TD[dt])
        rc = self.lib.pa_patch_gather_varlen(ptr(xd), B, F, T, ptr(rc_), ptr(rf), ptr(rt), M, Pp, fs, ts, out.ptr(), dt, self.st)
        self.done()
        return rc, out.take("cols")

    def _weights(self, w):
        return {k: gin(v) for k, v in w.items()}

    def pos_table(self, w, pf, pt, toff, B, Ntok):
        D, Tpe, Fpe = w["bias"].numel(), w["tpos"].shape[1], w["fpos"].shape[1]
        d, pfd, ptd = self._weights(w), gin(pf), gin(pt)
        table, tok = Out((pf.numel(), D), F32), Out((B, Ntok, D), F32)
        rc = self.lib.pa_patch_pos_table(ptr(d["bias"]), ptr(d["tpos"]), Tpe, ptr(d["fpos"]), Fpe, ptr(pfd), ptr(ptd), pf.numel(), toff, D,
                                         table.ptr(), ptr(d["cls"]), ptr(d["dist"]), ptr(d["npe"]), tok.ptr(), B, Ntok, self.st)
        self.done()
        return rc, table.take("table"), tok.peek("tok")

    def pos_table_varlen(self, w, row_f, row_t):
        D, Tpe, Fpe = w["bias"].numel(), w["tpos"].shape[1], w["fpos"].shape[1]
        d, rf, rt = self._weights(w), gin(row_f), gin(row_t)
        M = row_f.numel()
        table = Out((M, D), F32)
        rc = self.lib.pa_patch_pos_table_varlen(ptr(d["bias"]), ptr(d["tpos"]), Tpe, ptr(d["fpos"]), Fpe, ptr(rf), ptr(rt), M, D, table.ptr(),
                                                ptr(d["cls"]), ptr(d["dist"]), ptr(d["npe"]), self.st)
        self.done()
        return rc, table.take("table")

    def _grad_outs(self, D, Tpe, Fpe, start, acc):
        return {k: Out(shp, F32, init=start[k] if acc else None) for k, shp in P.grad_shapes(D, Tpe, Fpe).items()}

    def patch_bwd(self, dtok, pf, pt, c, start):
        B, Ntok, D = dtok.shape
        Np = pf.numel()
        dd, pfd, ptd = gin(dtok), gin(pf), gin(pt)
        dpatch = Out((B * Np, D), TD[c.dt])
        if c.rows_only:
            rc = self.lib.pa_patch_bwd(ptr(dd), B, Ntok, D, ptr(pfd), ptr(ptd), Np, c.toff, c.Tpe, c.Fpe, None, None, None, None, None, None, None,
                                       c.acc, dpatch.ptr(), c.dt, self.st)
            self.done()
            return rc, dict(dpatch=dpatch.take("dpatch"))
        gsum = Out((Ntok, D), F32)
        o = self._grad_outs(D, c.Tpe, c.Fpe, start, c.acc)
        rc = self.lib.pa_patch_bwd(ptr(dd), B, Ntok, D, ptr(pfd), ptr(ptd), Np, c.toff, c.Tpe, c.Fpe, gsum.ptr(), *[o[k].ptr() for k in P.GRAD_KEYS],
                                   c.acc, dpatch.ptr(), c.dt, self.st)
        self.done()
        res = {k: o[k].take(k) for k in P.GRAD_KEYS}
        res.update(gsum=gsum.take("gsum"), dpatch=dpatch.take("dpatch"))
        return rc, res

    def bwd_varlen(self, dtok, lay, B, Tpe, Fpe, start, acc, none=False):
        M, D = dtok.shape
        dd, cu = gin(dtok), gin(lay["cu_tok"])
        if none:
            rc = self.lib.pa_patch_bwd_varlen(ptr(dd), M, D, ptr(cu), B, Tpe, Fpe, None, None, None, None, None, None, acc, self.st)
            self.done()
            return rc, None
        o = self._grad_outs(D, Tpe, Fpe, start, acc)
        rc = self.lib.pa_patch_bwd_varlen(ptr(dd), M, D, ptr(cu), B, Tpe, Fpe, *[o[k].ptr() for k in P.GRAD_KEYS], acc, self.st)
        self.done()
        return rc, {k: o[k].take(k) for k in P.GRAD_KEYS}

    def bwd_rows(self, dtok, lay, toff, B, Tpe, Fpe, start, acc, none=False):
        M, D = dtok.shape
        Tg = lay["slot"].shape[2]
        dd, cu, sl, to = gin(dtok), gin(lay["cu_tok"]), gin(lay["slot"]), gin(toff)
        if none:
            rc = self.lib.pa_patch_bwd_rows(ptr(dd), M, D, ptr(sl), ptr(cu), ptr(to), B, Tg, Tpe, Fpe, None, None, None, None, None, None, acc, self.st)
            self.done()
            return rc, None
        o = self._grad_outs(D, Tpe, Fpe, start, acc)
        rc = self.lib.pa_patch_bwd_rows(ptr(dd), M, D, ptr(sl), ptr(cu), ptr(to), B, Tg, Tpe, Fpe, *[o[k].ptr() for k in P.GRAD_KEYS], acc, self.st)
        self.done()
        return rc, {k: o[k].take(k) for k in P.GRAD_KEYS}

    def fold(self, dcols, g, pf, pt):
        dt = PA_BF16 if dcols.dtype == torch.bfloat16 else PA_F32
        dc, pfd, ptd = gin(dcols), gin(pf), gin(pt)
        cells = self.lib.pa_patch_input_bwd_ws_ints(g.F, g.T, g.P, g.fs, g.ts)
        assert cells == g.Fg * g.Tg
        ws, dx = Out((cells,), F32), Out((g.B, g.F, g.T), F32)        # (the int32 table in a 4-byte sentinel buffer)
        rc = self.lib.pa_patch_input_bwd(ptr(dc), dt, g.B, pf.numel(), ptr(pfd), ptr(ptd), g.P, g.fs, g.ts, g.F, g.T, ws.ptr(), dx.ptr(), self.st)
        self.done()
        ws.peek("grid_ws")
        return rc, dx.take("dx")

    def fold_varlen(self, dcols, g, lay):
        dt = PA_BF16 if dcols.dtype == torch.bfloat16 else PA_F32
        dc, cu = gin(dcols), gin(lay["cu_tok"])
        dx = Out((g.B, g.F, g.T), F32)
        rc = self.lib.pa_patch_input_bwd_varlen(ptr(dc), dt, ptr(cu), g.B, g.P, g.fs, g.ts, g.F, g.T, dx.ptr(), self.st)
        self.done()
        return rc, dx.take("dx")

    def fold_rows(self, dcols, g, slot):
        dt = PA_BF16 if dcols.dtype == torch.bfloat16 else PA_F32
        dc, sl = gin(dcols), gin(slot)
        dx = Out((g.B, g.F, g.T), F32)
        rc = self.lib.pa_patch_input_bwd_rows(ptr(dc), dt, dcols.shape[0], ptr(sl), g.B, slot.shape[2], g.P, g.fs, g.ts, g.F, g.T, dx.ptr(), self.st)
        self.done()
        return rc, dx.take("dx")

    # -- movers and casts
    def gather_rows(self, inp, idx, offset=0):
        src, ix = gin(inp, offset), gin(idx)
        out = Out((idx.numel(), inp.shape[1]), F32, offset=offset)
        rc = self.lib.pa_gather_rows(ptr(src), ptr(ix), idx.numel(), inp.shape[1] * 4, out.ptr(), self.st)
        self.done()
        return rc, out.take("out").view(I32)

    def scatter_rows(self, inp, idx, n_rows, offset=0):
        src, ix = gin(inp, offset), gin(idx)
        out = Out((n_rows, inp.shape[1]), F32, offset=offset)
        rc = self.lib.pa_scatter_rows(ptr(src), ptr(ix), idx.numel(), inp.shape[1] * 4, out.ptr(), self.st)
        self.done()
        return rc, out.peek("out").view(I32)

    def tail_inject(self, rows, idx, add0, add1, M, D, lp):
        r, ix, a0, a1 = gin(rows if rows.numel() else None), gin(idx if idx.numel() else None), gin(add0), gin(add1)
        dx = Out((M, D), F32)
        dx_lp = None if lp is None else Out((M, D), TD[lp])
        rc = self.lib.pa_tail_inject(ptr(r), ptr(ix), idx.numel(), ptr(a0), ptr(a1), dx.ptr(), None if lp is None else dx_lp.ptr(),
                                     PA_BF16 if lp is None else lp, M, D, self.st)
        self.done()
        return rc, dx.take("dx"), (None if lp is None else dx_lp.take("dx_lp"))

    def transpose(self, inp, R, Cc, out_dt, ldo):
        in_dt = PA_BF16 if inp.dtype == torch.bfloat16 else PA_F32
        src = gin(inp)
        out = Out((Cc, ldo), TD[out_dt])
        rc = self.lib.pa_transpose(ptr(src), in_dt, R, Cc, inp.shape[1], out.ptr(), out_dt, ldo, self.st)
        self.done()
        return rc, out.take("out")

    def stage(self, srcs, dt, which):
        """every destination a guarded allocation of its own; every fourth entry's destinations one element off alignment, which the
        kernel answers with its scalar path"""
        arr = (_lib.StageDesc * len(srcs))()
        keep, outs, tiles = [], [], 0
        for j, (d, s, w) in enumerate(zip(arr, srcs, which)):
            r, c = s.shape
            off = 1 if j % 4 == 3 else 0
            sd = gin(s)
            dst = Out((r, c), TD[dt], offset=off) if "d" in w else None
            dst_t = Out((c, r), TD[dt], offset=off) if "t" in w else None
            keep.append(sd)
            outs.append((dst, dst_t))
            d.src, d.dst, d.dst_t = ptr(sd), (dst.ptr() if dst else None), (dst_t.ptr() if dst_t else None)
            d.rows, d.cols, d.tile_begin = r, c, tiles
            tiles += P.cdiv(r, 64) * P.cdiv(c, 64)
        table = gin(torch.frombuffer(bytearray(bytes(arr)), dtype=I32).clone())
        rc = self.lib.pa_stage_weights(ptr(table), len(srcs), tiles, dt, self.st)
        self.done()
        return rc, [(a.take("dst") if a else None, b.take("dst_t") if b else None) for a, b in outs]

    def zero2d(self, rows, width, pitch, offset=0):
        assert pitch % 4 == 0 and offset % 4 == 0
        buf = Out((rows, pitch // 4), F32, offset=offset // 4)
        rc = self.lib.pa_zero2d(buf.ptr(), pitch, width, rows, self.st)
        self.done()
        return rc, buf.peek("zero2d").view(torch.uint8)

    def convert(self, x, dt, in_offset=0):
        src = gin(x, in_offset)
        out = Out(x.shape, TD[dt])
        rc = self.lib.pa_convert_f32(ptr(src), out.ptr(), x.numel(), dt, self.st)
        self.done()
        return rc, out.take("out")

    def convert_rowscale(self, x, rs, dt):
        src, r = gin(x), gin(rs, 1)                  # rowscale: one float per row, any alignment
        out = Out(x.shape, TD[dt])
        rc = self.lib.pa_convert_f32_rowscale(ptr(src), ptr(r), out.ptr(), x.shape[0], x.shape[1], dt, self.st)
        self.done()
        return rc, out.take("out")

    def convert_to_f32(self, x, in_offset=0):
        src = gin(x, in_offset)
        out = Out(x.shape, F32)
        rc = self.lib.pa_convert_to_f32(ptr(src), PA_BF16 if x.dtype == torch.bfloat16 else PA_F32, out.ptr(), x.numel(), self.st)
        self.done()
        return rc, out.take("out")


@pytest.fixture(scope="module")
def hip():
    return Hip()


@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("geom", P.GEOMS, ids=str)
def test_folds(hip, geom, form):
    """pa_patch_input_bwd / _varlen / _rows: bit-equal to the f32 sum in (frequency row, time column) order, exact on integers, +0 at
    every pixel no kept patch covers, NaN under the prefix rows of the packed dcols never read"""
    P.run_folds(hip, geom, form)


@pytest.mark.parametrize("geom", P.GEOMS, ids=str)
def test_gathers_and_tables(hip, geom):
    """pa_patch_gather(_varlen): every element the right pixel (distinct integers), zero prefix rows, 0 outside x, bf16 by
    round-to-nearest-even; pa_patch_pos_table(_varlen): (bias + tpos) + fpos in f32, the prefix rows, nothing else of tok written"""
    P.run_gathers(hip, geom)
    P.run_tables(hip, geom)


@pytest.mark.parametrize("c", P.pg_cases(), ids=lambda c: c.name)
def test_patch_bwd(hip, c):
    """pa_patch_bwd: gsum, the six gradients (exact on integers, inside the derived bound and repeatable on graded operands), dpatch
    the exact cast of the patch rows"""
    P.check_patch_bwd(hip, c, record)


@pytest.mark.parametrize("form", ("varlen", "rows"))
@pytest.mark.parametrize("geom", P.GEOMS, ids=str)
def test_packed_gradients(hip, geom, form):
    P.run_packed_grads(hip, geom, form, record)


def test_cross_entry_equalities_noop_and_tie_dpatch(hip):
    """packed with equal lengths == fixed, rows with a full table == packed, every clip == that clip alone; the all-NULL no-op; dpatch
    on the tie family"""
    P.run_cross_entry(hip)
    P.run_noop(hip)
    P.run_tie_dpatch(hip)


@pytest.mark.parametrize("which", P.MOVERS)
def test_movers(hip, which):
    P.run_movers(hip, which)


@pytest.mark.parametrize("entry,args", P.SECOND_TRIP, ids=[e for e, _ in P.SECOND_TRIP])
def test_second_trips(hip, entry, args):
    """one call per capped grid whose stride loop takes a second trip"""
    P.check_second_trip(hip, entry, args)


def test_refusals_write_nothing(hip):
    """pa_patch_bwd with an unknown dtype and non-NULL gradients: PA_EINVAL and gsum, the six gradients and dpatch keep the sentinel
    (the entry used to launch two kernels first); aligned device pointers, so only the dtype is at fault"""
    c = P.PG(17, 16, 3, 0, 7, 0, 0, PA_BF16, "integer")
    pf, pt = P.pg_patches(c)
    dd, pfd, ptd = gin(P.pg_dtok(c)), gin(pf), gin(pt)
    outs = {k: Out(shp, F32) for k, shp in P.grad_shapes(c.D, c.Tpe, c.Fpe).items()}
    gsum, dpatch = Out((c.Ntok, c.D), F32), Out((c.B * c.Np, c.D), torch.bfloat16)
    rc = hip.lib.pa_patch_bwd(ptr(dd), c.B, c.Ntok, c.D, ptr(pfd), ptr(ptd), c.Np, 0, c.Tpe, c.Fpe, gsum.ptr(), *[outs[k].ptr() for k in P.GRAD_KEYS],
                              0, dpatch.ptr(), 7, hip.st)
    torch.cuda.synchronize()
    assert rc == PA_EINVAL != PA_OK
    for k, o in list(outs.items()) + [("gsum", gsum), ("dpatch", dpatch)]:
        o.untouched(k)
    table, tok = Out((4, 8), F32), Out((1, 6, 8), F32)
    w = {k: gin(v) for k, v in P.table_weights(8, 3, 3).items()}
    rc = hip.lib.pa_patch_pos_table(ptr(w["bias"]), ptr(w["tpos"]), 3, ptr(w["fpos"]), 3, ptr(pfd), ptr(ptd), 0, 0, 8, table.ptr(), ptr(w["cls"]),
                                    ptr(w["dist"]), ptr(w["npe"]), tok.ptr(), 0, 6, hip.st)
    torch.cuda.synchronize()
    assert rc == PA_EINVAL
    table.untouched("table")
    tok.untouched("tok")

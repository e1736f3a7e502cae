"""Shapes, operand families, references and checkers of the exact parity suite of the patch stage (the twelve launching entries of
patch.hip in their fixed, packed and packed-with-Patchout forms) and of the data movers and casts beside it (pa_gather_rows,
pa_scatter_rows, pa_tail_inject, pa_zero2d, pa_transpose, pa_stage_weights, pa_convert_f32, pa_convert_f32_rowscale,
pa_convert_to_f32).

Used by tests/test_gpu_patch_exact.py (the HIP kernels, through the C ABI, every operand and output in a guarded buffer of
tests/row_kernel_cases.py) and tests/test_patch_cases_cpu.py (the same checkers against `TorchPatch`, plain f32 torch).  A checker
takes an `impl` object, hands it CPU tensors and gets CPU tensors back; it neither knows nor cares where the arithmetic ran.  Where
an entry writes only part of a buffer (the two prefix rows of tok, the rows a scatter names, the width of a pitched zero fill) the
impl returns the whole buffer and everything else must still hold SENTINEL.

Operand families -- almost everything here is a copy, a cast or a sum of a few hundred terms, so every check but one is exact:

  code      every source element a distinct integer (below 2^24 in f32, |v| <= 256 where the destination is bf16, then distinct
            within a row and rows told apart by their first elements): a copy, gather, scatter or transpose is compared with
            torch.equal, and a misplaced element cannot equal the right one.
  integer   ((row * 131 + k * 7) mod 255) - 127: every partial sum stays below 2^24, a reduction in ANY order is exact; compared
            with torch.equal against an f64 (= exact integer) sum.  All parameter-gradient sums, gsum, the folds, accumulate = 1.
  order     non-integer f32 (bf16 for bf16 dcols) for the folds, whose order the header promises (frequency row, then time column):
            the reference adds in f32 in exactly that order; torch.equal.
  graded    non-integer f32 with row scale 2^(m mod 7 - 3) for the parameter-gradient sums, whose order is fixed but not part of the
            header: |got - f64 sum| <= (n - 1) 2^-24 sum|terms| per element (n = number of terms, the accumulate start value
            included) -- the first-order bound of ANY summation tree of n terms, derived, not measured.  Each entry is called
            twice and must repeat itself bit for bit (the header says deterministic).
  tie       f32 values around the bf16 rounding: exact ties with even and odd kept mantissa and one ulp on either side, +-0, +-inf,
            the largest finite f32 (rounds to inf), the smallest normal, subnormals, NaN.  Bit-equal to torch's CPU cast; NaN
            compared with isnan.
"""
import math
from dataclasses import dataclass

import torch

from tests.row_kernel_cases import EXACT_LIMIT, PA_BF16, PA_F32, SENTINEL, TD, rnd, row_scales  # noqa: F401

PA_OK, PA_EINVAL, PA_EUNSUPPORTED = 0, -1, -2
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
DTS = (PA_F32, PA_BF16)


def cdiv(a, b):
    return -(-a // b)


def equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got.float())
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ, first at {idx}: "
                             f"got {float(got[tuple(idx)])}, want {float(want[tuple(idx)])}")


def ok(rc, what):
    assert rc == PA_OK, f"{what}: code {rc} for a case of the positive list"


# ---- operand families ------------------------------------------------------------------------------------------------------
def integer_fam(rows, cols, dtype=F32):
    r, k = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    return (((r * 131 + k * 7) % 255) - 127).to(dtype)


def code_f32(*shape, base=1):
    n = math.prod(shape)
    assert base + n < EXACT_LIMIT
    return (torch.arange(n) + base).float().view(shape)


def code_bf16(rows, cols):
    """|v| <= 256, distinct within a row; row r starts at a different phase, so neighbouring rows differ in every column"""
    assert cols <= 513
    r, k = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    v = ((r * 37 + k) % 513 - 256).float()
    assert torch.equal(v.to(BF16).float(), v)
    return v


def graded_fam(rows, cols, seed):
    return rnd(rows, cols, seed=seed, scale=2.0) * row_scales(rows)


def _bits(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=I32).view(F32)


_TIE_POS = (0x3F808000, 0x3F818000,                         # exact ties: kept mantissa even (down), odd (up to even)
            0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # one ulp on either side of them
            0x3FFF8000, 0x407F8000,                         # ties that carry into the exponent
            0x00000000, 0x7F800000,                         # 0, inf
            0x7F7FFFFF, 0x7F7F7FFF, 0x7F7F8000,              # the largest finite f32 -> inf; just below the last tie; the tie -> inf
            0x00800000,                                     # the smallest normal
            0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x00400000, 0x007F8000)      # subnormals
_TIE_NAN = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FA00000)   # quiet, negative, and two whose payload truncation would turn into inf
TIE_CLASSES = dict(tie=(0, 8), zero_inf=(8, 10), overflow=(10, 13), normal_min=(13, 14), subnormal=(14, 21))


def tie_values():
    """the tie family, positive then negative, then the NaNs: 46 values (a length that is no multiple of a vector width, so a tiled
    tensor shows every value to every lane of a 2-, 4- and 8-element vector)"""
    v = torch.cat([_bits(_TIE_POS), _bits([w | 0x80000000 for w in _TIE_POS]), _bits(_TIE_NAN)])
    assert v.numel() == 46 and int(torch.isnan(v).sum()) == 4
    return v


def tie_tensor(*shape):
    v = tie_values()
    n = math.prod(shape)
    return v.repeat(cdiv(n, v.numel()) + 1)[:n].clone().view(shape)


def rne_bf16(x):
    """torch's CPU f32 -> bf16 cast: round to nearest even, NaN stays NaN"""
    return x.to(BF16)


def check_cast(got, src, dt, what):
    """got (TD[dt]) against the cast of src (f32): finite and infinite results bit for bit, NaN by isnan"""
    want = src if dt == PA_F32 else rne_bf16(src)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    nan = torch.isnan(want.float())
    assert torch.equal(torch.isnan(got.float()), nan), f"{what}: NaN must stay NaN and nothing else may become one"
    it = torch.int16 if want.dtype == BF16 else I32
    g, w = got.contiguous().view(it)[~nan], want.contiguous().view(it)[~nan]
    if not torch.equal(g, w):
        j = int((g != w).nonzero()[0])
        raise AssertionError(f"{what}: {int((g != w).sum())} casts differ in their bits, first: source {float(src[~nan][j])!r} "
                             f"(0x{int(src.contiguous().view(I32)[~nan][j]) & 0xFFFFFFFF:08X}) gave 0x{int(g[j]) & 0xFFFF:04X}, want 0x{int(w[j]) & 0xFFFF:04X}")


# ---- geometry --------------------------------------------------------------------------------------------------------------
GEOMS = ((4, 3, 3), (4, 4, 4), (4, 6, 5), (3, 2, 2), (16, 10, 10))       # (P, fstride, tstride)
MODEL_GEOM = (16, 10, 10)


def grid_dims(F, T, P, fs, ts):
    return (F - P) // fs + 1, (T - P) // ts + 1


@dataclass(frozen=True)
class Geo:
    P: int
    fs: int
    ts: int
    F: int
    T: int
    B: int
    pattern: str = "full"          # full | random | one | empty_row | empty_col | outside (fixed form) | odd (rows form: -1, -2, M)
    teff: tuple = ()               # packed forms: patch columns per clip

    @property
    def Fg(self):
        return grid_dims(self.F, self.T, self.P, self.fs, self.ts)[0]

    @property
    def Tg(self):
        return grid_dims(self.F, self.T, self.P, self.fs, self.ts)[1]

    @property
    def name(self):
        return f"P{self.P}s{self.fs}x{self.ts},F{self.F},T{self.T},B{self.B},{self.pattern}" + (f",teff{list(self.teff)}" if self.teff else "")


def geo_cases(P, fs, ts):
    """the shapes of one (P, fstride, tstride): T % 4 = 0 .. 3, B F T % 4 != 0, more than one workgroup (B F T > 1024), a strip of two
    or more pixels behind the last patch row and column, every Patchout pattern, B in {1, 3}"""
    if (P, fs, ts) == MODEL_GEOM:
        return [Geo(P, fs, ts, 36, 50, 1, "full"), Geo(P, fs, ts, 36, 50, 3, "random"), Geo(P, fs, ts, 36, 50, 1, "one"),
                Geo(P, fs, ts, 36, 50, 3, "empty_row"), Geo(P, fs, ts, 36, 50, 1, "empty_col")]
    out = []
    # the strip behind the last patch is (F - P) mod fstride pixels: two where the stride allows it, else stride - 1
    F = next(f for f in range(P + 2 * fs, P + 9 * fs) if (f - P) % fs >= strip_min(fs) and f % 4)      # F % 4 != 0: B F T % 4 != 0 for odd T
    pats = ("full", "random", "one", "empty_row", "empty_col", "random")

    def width(r, lo):
        for need in (strip_min(ts), 1, 0):             # (tstride 4: the strip is T % 4 itself)
            hit = [t for t in range(lo, lo + 8 * ts + 8) if t % 4 == r and (t - P) % ts >= need]
            if hit:
                return hit[0]
    for r in range(4):
        out.append(Geo(P, fs, ts, F, width(r, P + 2 * ts), (1, 3)[r % 2], pats[r]))
    big = cdiv(1025, 3 * F)
    out.append(Geo(P, fs, ts, F, width(1, big), 3, "empty_col"))     # B F T > 1024: a second workgroup, T % 4 = 1
    out.append(Geo(P, fs, ts, F, width(3, big), 3, "random"))        # T % 4 = 3
    return out


def strip_min(stride):
    return min(2, stride - 1)


def kept_patches(g, seed=0):
    """(patch_f, patch_t) int32 of the kept patches in a shuffled order (the slot index must not follow the grid order)"""
    Fg, Tg = g.Fg, g.Tg
    gen = torch.Generator().manual_seed(50 + seed)
    cells = [(f, t) for f in range(Fg) for t in range(Tg)]
    if g.pattern == "random":
        keep = torch.randperm(len(cells), generator=gen)[:max(1, (2 * len(cells)) // 3)].tolist()
        cells = [cells[k] for k in keep]
    elif g.pattern == "one":
        cells = [cells[len(cells) // 2]]
    elif g.pattern == "empty_row":
        cells = [c for c in cells if c[0] != Fg // 2]
    elif g.pattern == "empty_col":
        cells = [c for c in cells if c[1] != Tg // 2]
    order = torch.randperm(len(cells), generator=gen).tolist()
    cells = [cells[k] for k in order]
    return torch.tensor([c[0] for c in cells], dtype=I32), torch.tensor([c[1] for c in cells], dtype=I32)


def packed_layout(g, teff, seed=0, patchout=False):
    """the packed token matrix of clips with teff[b] patch columns: cu_tok, row_clip / row_f / row_t, and the slot table
    [B][Fg][Tg_max].  patchout: every clip keeps a random two thirds of its patches, in a shuffled order."""
    Fg, Tgm = g.Fg, max(max(teff), 1)
    gen = torch.Generator().manual_seed(70 + seed)
    cu, rc, rf, rt = [0], [], [], []
    slot = torch.full((len(teff), Fg, Tgm), -1, dtype=I32)
    for b, te in enumerate(teff):
        cells = [(f, t) for f in range(Fg) for t in range(te)]
        if patchout and cells:
            keep = torch.randperm(len(cells), generator=gen)[:max(1, (2 * len(cells)) // 3)].tolist()
            cells = [cells[k] for k in keep]
        rc += [b] * (2 + len(cells))
        rf += [-1, -1] + [c[0] for c in cells]
        rt += [0, 1] + [c[1] for c in cells]
        for j, (f, t) in enumerate(cells):
            slot[b, f, t] = cu[-1] + 2 + j
        cu.append(cu[-1] + 2 + len(cells))
    t = lambda v: torch.tensor(v, dtype=I32)      # noqa: E731
    return dict(cu_tok=t(cu), row_clip=t(rc), row_f=t(rf), row_t=t(rt), slot=slot, M=cu[-1], Tg=Tgm)


def cover_candidates(c, P, stride, G):
    """per coordinate the grid positions [lo, hi] whose patch [g stride, g stride + P) holds it (hi < lo: none)"""
    c = torch.as_tensor(c)
    lo = torch.where(c >= P, (c - P) // stride + 1, torch.zeros_like(c))
    hi = torch.minimum(c // stride, torch.full_like(c, G - 1))
    return lo, hi


def fold_paths(g, dt):
    """which of the fold kernels' code paths the shape reaches: inside (four pixels of one row), straddle (T % 4 != 0), tail
    (B F T % 4 != 0), pair (the bf16 4-byte read), nopair (bf16 without it), multi (more than one workgroup), strip, gaps, overlap"""
    n = g.B * g.F * g.T
    paths = {"inside"}
    if g.T % 4:
        paths.add("straddle")
    if n % 4:
        paths.add("tail")
    if n > 1024:
        paths.add("multi")
    if dt == PA_BF16:
        for t0 in (range(g.T - 3) if g.T % 4 else range(0, g.T - 3, 4)):      # T % 4 != 0: a row starts at any residue
            for gt in range(g.Tg):
                j0 = t0 - gt * g.ts
                if -4 < j0 < g.P:                        # the four pixels meet the patch
                    paths.add("pair" if (j0 >= 0 and j0 + 4 <= g.P and (j0 | g.P) % 2 == 0) else "nopair")
    if g.F - ((g.Fg - 1) * g.fs + g.P) >= strip_min(g.fs) and g.T - ((g.Tg - 1) * g.ts + g.P) >= strip_min(g.ts):
        paths.add("strip")
    if g.fs > g.P or g.ts > g.P:
        paths.add("gaps")
    if g.fs < g.P or g.ts < g.P:
        paths.add("overlap")
    return paths


# ---- references ------------------------------------------------------------------------------------------------------------
def ref_fold(dcols, table, g, Tg):
    """gather form of the header: pixel (b, f, t) adds dcols[table[b][gf][gt]][(f - gf fs) P + (t - gt ts)] over the covering grid
    positions with a valid row, in (gf, gt) order, in f32.  table: [B][Fg][Tg] rows of dcols, anything outside [0, rows) = none."""
    B, F, T, P = g.B, g.F, g.T, g.P
    Fg = g.Fg
    rows = dcols.shape[0]
    d = dcols.float()
    f = torch.arange(F)[None, :, None].expand(B, F, T)
    t = torch.arange(T)[None, None, :].expand(B, F, T)
    b = torch.arange(B)[:, None, None].expand(B, F, T)
    flo, fhi = cover_candidates(f, P, g.fs, Fg)
    tlo, thi = cover_candidates(t, P, g.ts, Tg)
    dx = torch.zeros(B, F, T, dtype=F32)
    terms = torch.zeros(B, F, T, dtype=torch.int64)
    for a in range(cdiv(P, g.fs)):
        for c in range(cdiv(P, g.ts)):
            gf, gt = flo + a, tlo + c
            valid = (gf <= fhi) & (gt <= thi)
            r = table[b, gf.clamp(0, Fg - 1), gt.clamp(0, max(Tg, 1) - 1)].long() if Tg > 0 else torch.full_like(b, -1)
            valid &= (r >= 0) & (r < rows)
            col = (f - gf * g.fs) * P + (t - gt * g.ts)
            v = d[r.clamp(0, rows - 1), col.clamp(0, P * P - 1)]
            dx = torch.where(valid, dx + v, dx)
            terms += valid
    return dx, terms


def fixed_table(g, pf, pt):
    """[B][Fg][Tg] rows of dcols[B Np][.] for the fixed form; pairs outside the grid are ignored"""
    Np = pf.numel()
    tab = torch.full((g.B, g.Fg, g.Tg), -1, dtype=I32)
    for p in range(Np):
        f, t = int(pf[p]), int(pt[p])
        if 0 <= f < g.Fg and 0 <= t < g.Tg:
            for b in range(g.B):
                tab[b, f, t] = b * Np + p
    return tab


def ref_gather(x, clip, pf, pt, P, fs, ts):
    """cols[r][i P + j] = x[clip[r]][pf[r] fs + i][pt[r] ts + j]; 0 outside x, a zero row where pf < 0"""
    B, F, T = x.shape
    i, j = torch.arange(P)[:, None].expand(P, P).reshape(-1), torch.arange(P)[None, :].expand(P, P).reshape(-1)
    f, t = pf.long()[:, None] * fs + i[None], pt.long()[:, None] * ts + j[None]
    inside = (pf.long()[:, None] >= 0) & (f < F) & (t >= 0) & (t < T) & (clip.long()[:, None] >= 0) & (clip.long()[:, None] < B)
    v = x[clip.long()[:, None].clamp(0, B - 1), f.clamp(0, F - 1), t.clamp(0, T - 1)]
    return torch.where(inside, v, torch.zeros_like(v))


def ref_param_grads(dtok2, prefix, triples, D, Tpe, Fpe):
    """f64 sums, sums of |terms| and term counts of the six gradients.  dtok2: [rows][D]; prefix: [(cls row, dist row)];
    triples: (bias rows, rows, f, tp) int64 tensors: every patch row (the conv bias), and the rows that have a place in the patch grid
    with their frequency and time position slots."""
    d = dtok2.double()
    out = {}
    brows, rows, f, tp = triples
    for key, src in (("sum", d), ("abs", d.abs()), ("cnt", torch.ones_like(d))):
        cls = sum((src[c] for c, _ in prefix), torch.zeros(D, dtype=torch.float64))
        dist = sum((src[k] for _, k in prefix), torch.zeros(D, dtype=torch.float64))
        bias = src[brows].sum(0)
        tpos = torch.zeros(Tpe, D, dtype=torch.float64).index_add_(0, tp, src[rows]).t().contiguous()
        fpos = torch.zeros(Fpe, D, dtype=torch.float64).index_add_(0, f, src[rows]).t().contiguous()
        out[key] = dict(d_cls=cls, d_dist=dist, d_npe=torch.stack([cls, dist]), d_bias=bias, d_tpos=tpos, d_fpos=fpos)
    return out


GRAD_KEYS = ("d_cls", "d_dist", "d_npe", "d_bias", "d_tpos", "d_fpos")


def grad_shapes(D, Tpe, Fpe):
    return dict(d_cls=(D,), d_dist=(D,), d_npe=(2, D), d_bias=(D,), d_tpos=(D, Tpe), d_fpos=(D, Fpe))


def grad_start(D, Tpe, Fpe, fam, seed=0):
    out = {}
    for j, (k, shp) in enumerate(grad_shapes(D, Tpe, Fpe).items()):
        n = math.prod(shp)
        out[k] = (integer_fam(1, n).view(shp) + j) if fam == "integer" else rnd(*shp, seed=900 + seed + j, scale=2.0)
    return out


def check_grads(got, ref, start, acc, fam, what, rec=None, group=None):
    """the six gradients against the reference: torch.equal (integer) or the derived bound (graded); returns nothing"""
    for k in GRAD_KEYS:
        s, a, n = ref["sum"][k], ref["abs"][k], ref["cnt"][k]
        if acc:
            s, a, n = s + start[k].double(), a + start[k].double().abs(), n + 1
        if fam == "integer":
            assert float(a.max()) < EXACT_LIMIT, (what, k, "the exactness condition of the integer family")
            equal(got[k], s.float(), f"{what} {k}")
        else:
            bound = (n - 1).clamp_min(0) * 2.0 ** -24 * a
            err = (got[k].double() - s).abs()
            err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
            assert bool((err <= bound).all()), (what, k, "worst error / bound", float((err / bound.clamp_min(1e-300)).max()))
            nz = bound > 0
            if rec is not None and bool(nz.any()):
                rec(group or "param_grads", float((err[nz] / bound[nz]).max()))


# ---- case lists ------------------------------------------------------------------------------------------------------------
PG_NP = (1, 15, 16, 17, 31, 32, 33, 49)
PG_D = (5, 16, 24, 100)
PG_B = (1, 3, 4, 5, 9)
PG_GRID = (7, 7)                     # 49 cells: Np = 49 is the full grid


@dataclass(frozen=True)
class PG:
    """one pa_patch_bwd call"""
    Np: int
    D: int
    B: int
    toff: int
    Tpe: int
    extra: int                       # Ntok = Np + 2 + extra
    acc: int
    dt: int
    fam: str
    rows_only: bool = False
    Fpe: int = 7

    @property
    def Ntok(self):
        return self.Np + 2 + self.extra

    @property
    def name(self):
        return f"Np{self.Np},D{self.D},B{self.B},toff{self.toff},Tpe{self.Tpe},Ntok{self.Ntok},acc{self.acc},dt{self.dt},{self.fam}" + \
            (",rows_only" if self.rows_only else "")


def pg_cases():
    out = []
    j = 0
    for fam in ("integer", "graded"):
        for k, Np in enumerate(PG_NP):
            for s in (0, 1):
                D, B = PG_D[(k + 2 * s + j) % 4], PG_B[(k + 3 * s + j) % 5]
                toff = (0, 3)[(k + s) % 2]
                # toff + max(patch_t) == Tpe - 1 on every other case (pg_patches puts a patch into the last column)
                Tpe = toff + PG_GRID[1] + (0 if (k + s) % 2 == 0 or toff == 3 and k % 4 == 1 else 2)
                out.append(PG(Np, D, B, toff, Tpe, (0, 5)[(k + s) % 2], (k + s + j) % 2, DTS[(k // 2 + s) % 2], fam))
        j += 1
    out.append(PG(17, 16, 3, 3, 12, 0, 0, PA_BF16, "integer", rows_only=True))
    out.append(PG(33, 5, 4, 0, 7, 5, 0, PA_F32, "integer", rows_only=True))
    return out


def pg_patches(c):
    Fg, Tg = PG_GRID
    gen = torch.Generator().manual_seed(300 + c.Np + c.D)
    cells = [(f, t) for f in range(Fg) for t in range(Tg)]
    perm = torch.randperm(len(cells), generator=gen).tolist()
    cells = [(Fg // 2, Tg - 1)] + [cells[k] for k in perm if cells[k] != (Fg // 2, Tg - 1)]
    cells = cells[:c.Np]
    return torch.tensor([x[0] for x in cells], dtype=I32), torch.tensor([x[1] for x in cells], dtype=I32)


def pg_paths(c):
    """paths of batch_sum_kernel / patch_param_grads_kernel / patch_rows_kernel the case reaches"""
    p = set()
    p.add("sum_vec" if (c.Ntok * c.D) % 4 == 0 else "sum_scalar")
    p.add(f"sum_rem{c.B % 4}" if c.B >= 4 else f"sum_only_rem{c.B}")
    p.add("pairs" if c.Np > 16 else "no_pairs")
    p.add("remainder" if (c.Np - 1) % 32 < 16 else "no_remainder")
    p.add("rows_vec" if c.D % 8 == 0 else "rows_scalar")
    p.add("d_mask" if c.D % 16 else "d_full")
    if c.toff + PG_GRID[1] == c.Tpe:
        p.add("toff_edge")
    return p


# capped grids: the second trip of the stride loop (elements per trip, from the launch lines of the entries)
TRIP = dict(patch_rows_vec=8192 * 256 * 8, patch_rows_scalar=8192 * 256, convert_f32=4096 * 1024, convert_to_f32=4096 * 2048,
            convert_rowscale=4096 * 256 * 4, zero2d=8192 * 256 * 16)
# (entry, arguments): every one is a copy or a cast checked exactly, well under a second of device time
SECOND_TRIP = (("patch_rows_vec", dict(B=2, Np=1025, D=8192)),                 # B Np D = 16 793 600 > 16 777 216, D % 8 == 0
               ("patch_rows_scalar", dict(B=3, Np=141, D=4959)),              # 2 097 657 > 2 097 152, D % 8 != 0
               ("convert_f32", dict(n=4096 * 1024 + 5)),
               ("convert_to_f32", dict(n=4096 * 2048 + 3)),
               ("convert_rowscale", dict(M=1025, D=4096)),                    # M D / 4 = 1 049 600 > 1 048 576
               ("zero2d", dict(rows=4097, width=8192, pitch=8192 + 32)))      # rows width / 16 = 2 097 664 > 2 097 152

ROW_BYTES = (4, 12, 16, 2044, 2048, 4112)
TRANSPOSE_RC = (1, 63, 64, 65, 130)
DT_PAIRS = ((PA_F32, PA_F32), (PA_F32, PA_BF16), (PA_BF16, PA_BF16), (PA_BF16, PA_F32))


# ---- the plain torch implementation ----------------------------------------------------------------------------------------
class TorchPatch:
    """Every entry in plain f32 torch on the CPU with the kernels' calling conventions.  The small methods are the places a kernel
    goes wrong; the fault models of tests/test_patch_cases_cpu.py override them one at a time."""
    name = "torch"

    # -- hooks
    def cast(self, v, dt):
        return v.to(TD[dt])

    def kept(self, r, rows):
        return 0 <= r < rows

    def fold_order(self, cells):
        return sorted(cells)

    def cover_lo(self, c, P, stride):
        return (c - P) // stride + 1 if c >= P else 0

    def fold_finish(self, dx):
        return dx

    def gather_strides(self, fs, ts):
        return fs, ts

    def table_toff(self, toff):
        return toff

    def rows_toff(self, toff):
        return toff

    def grad_patches(self, Np):
        return Np

    def start_of(self, start, acc):
        return start if acc else None

    def dpatch_first(self):
        return 2

    def prefix_cols(self, v):
        return torch.zeros_like(v)

    def transpose_fill(self, out, R):
        out[:, R:] = 0

    # -- the patch stage
    def _fold(self, dcols, table, g, Tg):
        """scatter form: the patches in (gf, gt) order, each added onto its window in f32 (per pixel the same order of additions
        as the gather form)"""
        d = dcols.float()
        P = g.P
        dx = torch.zeros(g.B, g.F, g.T, dtype=F32)
        rows = dcols.shape[0]
        for b in range(g.B):
            cells = self.fold_order([(gf, gt) for gf in range(g.Fg) for gt in range(Tg)])
            for gf, gt in cells:
                r = int(table[b, gf, gt])
                if not self.kept(r, rows):
                    continue
                f0, t0 = gf * g.fs, gt * g.ts
                # the window through cover_lo: pixel c is inside when cover_lo(c) <= g
                fsel = [f for f in range(f0, f0 + P) if self.cover_lo(f, P, g.fs) <= gf]
                tsel = [t for t in range(t0, t0 + P) if self.cover_lo(t, P, g.ts) <= gt]
                if fsel and tsel:
                    blk = d[r].view(P, P)[fsel[0] - f0:fsel[-1] - f0 + 1, tsel[0] - t0:tsel[-1] - t0 + 1]
                    dx[b, fsel[0]:fsel[-1] + 1, tsel[0]:tsel[-1] + 1] += blk
        return self.fold_finish(dx)

    def fold(self, dcols, g, pf, pt):
        return PA_OK, self._fold(dcols, fixed_table(g, pf, pt), g, g.Tg)

    def fold_varlen(self, dcols, g, lay):
        tab = torch.full((g.B, g.Fg, lay["Tg"]), -1, dtype=I32)
        cu = lay["cu_tok"].tolist()
        for b in range(g.B):
            te = max((cu[b + 1] - cu[b] - 2) // g.Fg, 0)
            for f in range(g.Fg):
                for t in range(te):
                    tab[b, f, t] = cu[b] + 2 + f * te + t
        return PA_OK, self._fold(dcols, tab, g, lay["Tg"])

    def fold_rows(self, dcols, g, slot):
        return PA_OK, self._fold(dcols, slot, g, slot.shape[2])

    def gather(self, x, pf, pt, P, fs, ts, dt):
        B, Np = x.shape[0], pf.numel()
        fs, ts = self.gather_strides(fs, ts)
        clip = torch.arange(B, dtype=I32).repeat_interleave(Np)
        return PA_OK, self.cast(ref_gather(x, clip, pf.repeat(B), pt.repeat(B), P, fs, ts), dt)

    def gather_varlen(self, x, lay, P, fs, ts, dt):
        fs, ts = self.gather_strides(fs, ts)
        v = ref_gather(x, lay["row_clip"], lay["row_f"], lay["row_t"], P, fs, ts)
        pre = lay["row_f"] < 0
        v[pre] = self.prefix_cols(v[pre])
        return PA_OK, self.cast(v, dt)

    def pos_table(self, w, pf, pt, toff, B, Ntok):
        D = w["bias"].numel()
        table = (w["bias"][None, :] + w["tpos"].t()[self.table_toff(toff) + pt.long()]) + w["fpos"].t()[pf.long()]
        tok = torch.full((B, Ntok, D), SENTINEL)
        tok[:, 0], tok[:, 1] = w["cls"] + w["npe"][0], w["dist"] + w["npe"][1]
        return PA_OK, table, tok

    def pos_table_varlen(self, w, row_f, row_t):
        pre = row_f < 0
        f, t = row_f.long().clamp_min(0), torch.where(pre, torch.zeros_like(row_t), row_t).long()
        table = (w["bias"][None, :] + w["tpos"].t()[t]) + w["fpos"].t()[f]
        table[pre] = torch.where((row_t[pre] == 0)[:, None], (w["cls"] + w["npe"][0])[None], (w["dist"] + w["npe"][1])[None])
        return PA_OK, table

    def _grads(self, dtok2, prefix, triples, D, Tpe, Fpe, start, acc):
        brows, rows, f, tp = triples
        d = dtok2
        z = torch.zeros(D)
        cls = sum((d[c] for c, _ in prefix), z.clone())
        dist = sum((d[k] for _, k in prefix), z.clone())
        out = dict(d_cls=cls, d_dist=dist, d_npe=torch.stack([cls, dist]), d_bias=d[brows].sum(0),
                   d_tpos=torch.zeros(Tpe, D).index_add_(0, tp, d[rows]).t().contiguous(),
                   d_fpos=torch.zeros(Fpe, D).index_add_(0, f, d[rows]).t().contiguous())
        st = self.start_of(start, acc)
        return {k: (st[k] + v if st is not None else v) for k, v in out.items()}

    def patch_bwd(self, dtok, pf, pt, c, start):
        B, Ntok, D = dtok.shape
        Np = pf.numel()
        first = self.dpatch_first()
        dpatch = self.cast(dtok[:, first:first + Np].reshape(B * Np, D), c.dt)
        if c.rows_only:
            return PA_OK, dict(dpatch=dpatch)
        gsum = dtok.sum(0)
        n = self.grad_patches(Np)
        tri = (2 + torch.arange(n), 2 + torch.arange(n), pf.long()[:n], self.table_toff(c.toff) + pt.long()[:n])
        out = self._grads(gsum, [(0, 1)], tri, D, c.Tpe, c.Fpe, start, c.acc)
        out.update(gsum=gsum, dpatch=dpatch)
        return PA_OK, out

    def bwd_varlen(self, dtok, lay, B, Tpe, Fpe, start, acc, none=False):
        if none:
            return PA_OK, None
        return PA_OK, self._grads(dtok, *packed_triples(lay, None), dtok.shape[1], Tpe, Fpe, start, acc)

    def bwd_rows(self, dtok, lay, toff, B, Tpe, Fpe, start, acc, none=False):
        if none:
            return PA_OK, None
        toff = torch.tensor([self.rows_toff(int(v)) for v in toff], dtype=I32)
        return PA_OK, self._grads(dtok, *packed_triples(lay, toff), dtok.shape[1], Tpe, Fpe, start, acc)

    # -- movers and casts
    def gather_rows(self, inp, idx, offset=0):
        return PA_OK, inp[idx.long()].clone()

    def scatter_rows(self, inp, idx, n_rows, offset=0):
        out = torch.full((n_rows, inp.shape[1]), SENTINEL).view(inp.dtype)
        out[idx.long()] = inp
        return PA_OK, out

    def tail_inject(self, rows, idx, add0, add1, M, D, lp):
        dx = torch.zeros(M, D)
        for a in (add0, add1):
            if a is not None:
                dx = dx + a
        if idx.numel():
            dx[idx.long()] += rows
        return PA_OK, dx, (None if lp is None else self.cast(dx, lp))

    def transpose(self, inp, R, C, out_dt, ldo):
        out = torch.full((C, ldo), SENTINEL, dtype=TD[out_dt])
        out[:, :R] = self.cast(inp[:R, :C].float().t(), out_dt)
        self.transpose_fill(out, R)
        return PA_OK, out

    def stage(self, srcs, dt, which):
        """srcs: [f32 [R][C]]; which[e]: "d" | "t" | "dt" -> [(dst or None, dst_t or None)]"""
        return PA_OK, [(self.cast(s, dt) if "d" in w else None, self.cast(s.t().contiguous(), dt) if "t" in w else None) for s, w in zip(srcs, which)]

    def zero2d(self, rows, width, pitch, offset=0):
        """the [rows][pitch] buffer as bytes; it starts as f32 SENTINEL values (pitch % 4 == 0) and keeps them where untouched"""
        buf = torch.full((rows, pitch // 4), SENTINEL).view(torch.uint8)
        buf[:, :width] = 0
        return PA_OK, buf

    def convert(self, x, dt, in_offset=0):
        return PA_OK, self.cast(x, dt)

    def convert_rowscale(self, x, rs, dt):
        return PA_OK, self.cast(x * rs[:, None], dt)

    def convert_to_f32(self, x, in_offset=0):
        return PA_OK, x.float()


def packed_triples(lay, toff):
    """(prefix rows, (bias rows, rows, f, tp)) of a packed layout.  toff None: the regular layout of pa_patch_bwd_varlen, positions
    from the rows' own coordinates.  toff [B]: pa_patch_bwd_rows -- the conv bias takes every patch row of cu_tok, a positional slot
    only the rows the slot table names (an entry outside [0, M) counts as none), time position = column + the clip's offset."""
    cu = lay["cu_tok"].tolist()
    prefix = [(cu[b], cu[b] + 1) for b in range(len(cu) - 1) if cu[b + 1] - cu[b] >= 2]
    patch = (lay["row_f"] >= 0).nonzero().flatten()
    if toff is None:
        return prefix, (patch, patch, lay["row_f"].long()[patch], lay["row_t"].long()[patch])
    slot = lay["slot"].long()
    b, f, t = ((slot >= 0) & (slot < lay["M"])).nonzero(as_tuple=True)
    return prefix, (patch, slot[b, f, t], f, t + toff.long()[b])


# ---- checkers: folds -------------------------------------------------------------------------------------------------------
def fold_dcols(rows, PP, dt, fam, seed=0):
    v = integer_fam(rows, PP) if fam == "integer" else graded_fam(rows, PP, 400 + seed)
    return v.to(TD[dt])


def _check_fold_result(dx, dcols, table, g, Tg, fam, what):
    want, terms = ref_fold(dcols, table, g, Tg)
    assert int(terms.max()) <= cdiv(g.P, g.fs) * cdiv(g.P, g.ts)
    if fam == "integer":
        assert float(torch.nan_to_num(dcols.float()).abs().max()) * int(terms.max()) < EXACT_LIMIT
    equal(dx, want, what)
    zero = terms == 0
    assert bool((dx[zero] == 0).all()) and not bool(torch.signbit(dx[zero]).any()), f"{what}: an uncovered pixel is not exactly +0"
    return int(zero.sum())


def check_fold_fixed(impl, g, dt, fam):
    pf, pt = kept_patches(g)
    if g.pattern == "outside":                       # Np stays the grid size: the last pair moves outside the grid and is ignored
        pf, pt = pf.clone(), pt.clone()
        pf[-1], pt[-1] = g.Fg, 0
    dcols = fold_dcols(g.B * pf.numel(), g.P * g.P, dt, fam)
    rc, dx = impl.fold(dcols, g, pf, pt)
    ok(rc, g.name)
    return _check_fold_result(dx, dcols, fixed_table(g, pf, pt), g, g.Tg, fam, f"fold {g.name} dt{dt} {fam}")


def varlen_teff(g, k):
    """patch columns per clip: 0, 1, 2 and Tg all occur over k = 0 .. 2"""
    Tg = g.Tg
    return ((Tg,), (1,), (2,))[k % 3] if g.B == 1 else ((Tg, 0, 1), (2, Tg, 0), (1, 2, Tg))[k % 3]


def nan_prefix(dcols, lay):
    d = dcols.clone()
    cu = lay["cu_tok"].long()[:-1]
    d[cu] = float("nan")
    d[cu + 1] = float("nan")
    return d


def check_fold_varlen(impl, g, dt, fam, k=0):
    teff = varlen_teff(g, k)
    lay = packed_layout(g, teff)
    dcols = nan_prefix(fold_dcols(lay["M"], g.P * g.P, dt, fam, seed=k), lay)       # "the rows under the prefix tokens are never read"
    rc, dx = impl.fold_varlen(dcols, g, lay)
    ok(rc, g.name)
    what = f"fold_varlen {g.name} teff{teff} dt{dt} {fam}"
    _check_fold_result(dx, dcols, lay["slot"], g, lay["Tg"], fam, what)
    for b, te in enumerate(teff):                                                 # exactly 0 at and behind the clip's own end
        end = (te - 1) * g.ts + g.P if te else 0
        assert bool((dx[b, :, end:] == 0).all()), what
    return teff


def rows_layout(g, k=0):
    lay = packed_layout(g, varlen_teff(g, k), seed=k, patchout=True)
    slot = lay["slot"].clone()
    if g.pattern == "odd":                           # entries the header says count as -1
        free = (slot < 0).nonzero()
        for n, bad in enumerate((-2, lay["M"], lay["M"] + 7)):
            if n < len(free):
                slot[tuple(free[n])] = bad
    elif g.pattern == "empty_row":
        slot[:, g.Fg // 2, :] = -1
    elif g.pattern == "empty_col":
        slot[:, :, slot.shape[2] // 2] = -1
    elif g.pattern == "one":
        first = (slot >= 0).nonzero()[0]
        keep = int(slot[tuple(first)])
        slot[:] = -1
        slot[tuple(first)] = keep
    elif g.pattern == "full":
        lay = packed_layout(g, varlen_teff(g, k), seed=k)
        slot = lay["slot"]
    lay["slot"] = slot
    return lay


def check_fold_rows(impl, g, dt, fam, k=0):
    lay = rows_layout(g, k)
    dcols = nan_prefix(fold_dcols(lay["M"], g.P * g.P, dt, fam, seed=k), lay)
    rc, dx = impl.fold_rows(dcols, g, lay["slot"])
    ok(rc, g.name)
    _check_fold_result(dx, dcols, lay["slot"], g, lay["Tg"], fam, f"fold_rows {g.name} dt{dt} {fam}")


# ---- checkers: gathers and tables --------------------------------------------------------------------------------------------
def gather_x(g, dt, fam):
    if fam == "tie":
        return tie_tensor(g.B, g.F, g.T)
    if dt == PA_BF16:
        return code_bf16(g.B * g.F, g.T).view(g.B, g.F, g.T)
    return code_f32(g.B, g.F, g.T)


def check_gather_fixed(impl, g, dt, fam="code"):
    pf, pt = kept_patches(g)
    x = gather_x(g, dt, fam)
    rc, cols = impl.gather(x, pf, pt, g.P, g.fs, g.ts, dt)
    ok(rc, g.name)
    clip = torch.arange(g.B, dtype=I32).repeat_interleave(pf.numel())
    check_cast(cols, ref_gather(x, clip, pf.repeat(g.B), pt.repeat(g.B), g.P, g.fs, g.ts), dt, f"gather {g.name} dt{dt} {fam}")


def check_gather_varlen(impl, g, dt, fam="code", k=0, outside=False):
    lay = rows_layout(g, k) if g.pattern != "full" else packed_layout(g, varlen_teff(g, k))
    lay = {key: (v.clone() if torch.is_tensor(v) else v) for key, v in lay.items()}
    if outside and lay["M"] > 2:                    # coordinates outside x read as 0: the last row far to the right, and below
        lay["row_t"][-1] = g.Tg + 3
        if lay["M"] > 3:
            lay["row_f"][-2] = g.Fg + 2
    x = gather_x(g, dt, fam)
    rc, cols = impl.gather_varlen(x, lay, g.P, g.fs, g.ts, dt)
    ok(rc, g.name)
    want = ref_gather(x, lay["row_clip"], lay["row_f"], lay["row_t"], g.P, g.fs, g.ts)
    what = f"gather_varlen {g.name} dt{dt} {fam}"
    check_cast(cols, want, dt, what)
    pre = lay["row_f"] < 0
    assert bool((cols[pre].float() == 0).all()), f"{what}: a prefix row is not all zeros"
    return lay, cols


def table_weights(D, Tpe, Fpe, seed=0):
    return dict(bias=rnd(D, seed=500 + seed), tpos=rnd(D, Tpe, seed=501 + seed), fpos=rnd(D, Fpe, seed=502 + seed), cls=rnd(D, seed=503 + seed),
                dist=rnd(D, seed=504 + seed), npe=rnd(2, D, seed=505 + seed))


def ref_table(w, f, t):
    return (w["bias"][None, :] + w["tpos"].t()[t.long()]) + w["fpos"].t()[f.long()]       # f32, (bias + tpos) + fpos in that order


def check_pos_table(impl, g, D, toff, extra):
    pf, pt = kept_patches(g)
    Tpe, Fpe = g.Tg + toff + (0 if extra else 2), g.Fg
    w = table_weights(D, Tpe, Fpe)
    Ntok = pf.numel() + 2 + extra
    rc, table, tok = impl.pos_table(w, pf, pt, toff, g.B, Ntok)
    ok(rc, g.name)
    what = f"pos_table {g.name} D{D} toff{toff}"
    equal(table, ref_table(w, pf, toff + pt), what)
    equal(tok[:, 0], (w["cls"] + w["npe"][0]).expand(g.B, D), what + " cls row")
    equal(tok[:, 1], (w["dist"] + w["npe"][1]).expand(g.B, D), what + " dist row")
    assert bool((tok[:, 2:] == SENTINEL).all()), what + ": a write into the patch rows of tok"


def check_pos_table_varlen(impl, g, D, k=0, toffs=None):
    lay = packed_layout(g, varlen_teff(g, k), seed=k, patchout=toffs is not None)
    row_t = lay["row_t"].clone()
    patch = lay["row_f"] >= 0
    if toffs is not None:                            # training on a packed batch: row_t + the clip's offset (in range: the caller's duty)
        row_t[patch] += torch.tensor(toffs, dtype=I32)[lay["row_clip"].long()[patch]]
    Tpe, Fpe = lay["Tg"] + (max(toffs) if toffs else 0), g.Fg
    w = table_weights(D, Tpe, Fpe, seed=k)
    rc, table = impl.pos_table_varlen(w, lay["row_f"], row_t)
    ok(rc, g.name)
    what = f"pos_table_varlen {g.name} D{D}"
    equal(table[patch], ref_table(w, lay["row_f"][patch], row_t[patch]), what)
    cu = lay["cu_tok"].long()[:-1]
    equal(table[cu], (w["cls"] + w["npe"][0]).expand(len(cu), D), what + " cls rows")
    equal(table[cu + 1], (w["dist"] + w["npe"][1]).expand(len(cu), D), what + " dist rows")
    return lay, w, table


# ---- checkers: parameter gradients ---------------------------------------------------------------------------------------------
def pg_dtok(c):
    rows = c.B * c.Ntok
    v = integer_fam(rows, c.D) if c.fam == "integer" else graded_fam(rows, c.D, 600 + c.Np)
    return v.view(c.B, c.Ntok, c.D)


def check_patch_bwd(impl, c, rec=None):
    pf, pt = pg_patches(c)
    assert int(pt.max()) + c.toff < c.Tpe and int(pf.max()) < c.Fpe, "in range: the caller's duty"
    dtok = pg_dtok(c)
    Fpe = c.Fpe
    start = grad_start(c.D, c.Tpe, Fpe, c.fam)
    rc, o = impl.patch_bwd(dtok, pf, pt, c, start)
    ok(rc, c.name)
    want_rows = dtok[:, 2:2 + c.Np].reshape(c.B * c.Np, c.D)
    check_cast(o["dpatch"], want_rows, c.dt, c.name + " dpatch")
    if c.rows_only:
        assert set(o) == {"dpatch"}
        return
    g64 = dtok.double().sum(0)
    if c.fam == "integer":
        assert float(dtok.double().abs().sum(0).max()) * c.Np < EXACT_LIMIT
        equal(o["gsum"], g64.float(), c.name + " gsum")
    else:
        bound = (c.B - 1) * 2.0 ** -24 * dtok.double().abs().sum(0)
        err = (o["gsum"].double() - g64).abs()
        assert bool((err <= bound).all()), (c.name, "gsum")
        if rec is not None and c.B > 1:
            rec("gsum", float((err / bound.clamp_min(1e-300)).max()))
    b = torch.arange(c.B)[:, None] * c.Ntok
    rows = (b + 2 + torch.arange(c.Np)[None, :]).reshape(-1)
    tri = (rows, rows, pf.long().repeat(c.B), (c.toff + pt.long()).repeat(c.B))
    ref = ref_param_grads(dtok.reshape(-1, c.D), [(int(x), int(x) + 1) for x in b[:, 0]], tri, c.D, c.Tpe, Fpe)
    check_grads(o, ref, start, c.acc, c.fam, c.name, rec, "patch_bwd")
    if c.fam == "graded":
        rc2, o2 = impl.patch_bwd(dtok, pf, pt, c, start)
        for k in GRAD_KEYS + ("gsum", "dpatch"):
            assert torch.equal(o[k], o2[k]), (c.name, k, "not deterministic")


PACKED_D = (5, 16, 24, 100)


def packed_dtok(M, D, fam, seed=0):
    return integer_fam(M, D) if fam == "integer" else graded_fam(M, D, 700 + seed)


def check_bwd_packed(impl, g, D, fam, acc, form, k=0, rec=None):
    """pa_patch_bwd_varlen (form "varlen") / pa_patch_bwd_rows (form "rows": Patchout + per-clip toff, with p - toff[b] both negative
    and >= Tg for some time position p)"""
    if form == "varlen":
        lay = packed_layout(g, varlen_teff(g, k), seed=k)
        toff, Tpe = None, lay["Tg"] + 1
    else:
        lay = rows_layout(g, k)
        toff = torch.tensor([(0, 3, 1)[(b + k) % 3] for b in range(g.B)], dtype=I32)
        Tpe = lay["Tg"] + 3 + (1 if k % 2 else 0)
    Fpe = g.Fg
    dtok = packed_dtok(lay["M"], D, fam, seed=k)
    start = grad_start(D, Tpe, Fpe, fam, seed=k)
    call = (lambda: impl.bwd_varlen(dtok, lay, g.B, Tpe, Fpe, start, acc)) if form == "varlen" else \
        (lambda: impl.bwd_rows(dtok, lay, toff, g.B, Tpe, Fpe, start, acc))
    rc, o = call()
    what = f"bwd_{form} {g.name} D{D} {fam} acc{acc} k{k}"
    ok(rc, what)
    prefix, tri = packed_triples(lay, toff)
    ref = ref_param_grads(dtok, prefix, tri, D, Tpe, Fpe)
    check_grads(o, ref, start, acc, fam, what, rec, f"patch_bwd_{form}")
    if fam == "graded":
        _, o2 = call()
        for key in GRAD_KEYS:
            assert torch.equal(o[key], o2[key]), (what, key, "not deterministic")
    return lay, dtok, start, o


# ---- checkers: cross-entry equalities ----------------------------------------------------------------------------------------
def check_packed_equals_fixed(impl, g, dt, D=16):
    """equal lengths and the full patch list: gather, table, fold bit for bit; the parameter gradients on the integer family (their
    summation orders differ: batch sum first against clip after clip)"""
    assert g.pattern == "full"
    lay = packed_layout(g, (g.Tg,) * g.B)
    pf, pt = lay["row_f"][2:2 + g.Fg * g.Tg], lay["row_t"][2:2 + g.Fg * g.Tg]
    Np = pf.numel()
    patch = lay["row_f"] >= 0
    x = code_f32(g.B, g.F, g.T) if dt == PA_F32 else code_bf16(g.B * g.F, g.T).view(g.B, g.F, g.T)
    _, cf = impl.gather(x, pf, pt, g.P, g.fs, g.ts, dt)
    _, cv = impl.gather_varlen(x, lay, g.P, g.fs, g.ts, dt)
    equal(cv[patch], cf, "packed gather == fixed gather")
    w = table_weights(D, g.Tg, g.Fg)
    _, tf, _ = impl.pos_table(w, pf, pt, 0, g.B, Np + 2)
    _, tv = impl.pos_table_varlen(w, lay["row_f"], lay["row_t"])
    equal(tv[patch], tf.repeat(g.B, 1), "packed table == fixed table")
    dcols = fold_dcols(lay["M"], g.P * g.P, dt, "order")
    _, dxf = impl.fold(dcols[patch].contiguous(), g, pf, pt)
    _, dxv = impl.fold_varlen(nan_prefix(dcols, lay), g, lay)
    _, dxr = impl.fold_rows(nan_prefix(dcols, lay), g, lay["slot"])
    equal(dxv, dxf, "packed fold == fixed fold")
    equal(dxr, dxv, "rows fold with a full table == packed fold")
    start = grad_start(D, g.Tg, g.Fg, "integer")
    graded = packed_dtok(lay["M"], D, "graded")
    _, gv = impl.bwd_varlen(graded, lay, g.B, g.Tg, g.Fg, start, 1)
    _, gr = impl.bwd_rows(graded, lay, torch.zeros(g.B, dtype=I32), g.B, g.Tg, g.Fg, start, 1)
    for k in GRAD_KEYS:
        equal(gr[k], gv[k], f"rows gradients with a full table == packed gradients, {k}")
    dtok = packed_dtok(lay["M"], D, "integer")
    c = PG(Np, D, g.B, 0, g.Tg, 0, 1, PA_F32, "integer", Fpe=g.Fg)
    _, of = impl.patch_bwd(dtok.view(g.B, Np + 2, D), pf, pt, c, start)
    _, ov = impl.bwd_varlen(dtok, lay, g.B, g.Tg, g.Fg, start, 1)
    for k in GRAD_KEYS:
        equal(ov[k], of[k], f"packed gradients == fixed gradients (integer family), {k}")


def check_clip_alone(impl, g, dt, k=0):
    """every clip of a packed batch == that clip run alone: gather rows, table rows, fold planes"""
    assert g.B > 1
    teff = varlen_teff(g, k)
    lay = packed_layout(g, teff, seed=k)
    x = code_f32(g.B, g.F, g.T) if dt == PA_F32 else code_bf16(g.B * g.F, g.T).view(g.B, g.F, g.T)
    dcols = nan_prefix(fold_dcols(lay["M"], g.P * g.P, dt, "order", seed=k), lay)
    _, cols = impl.gather_varlen(x, lay, g.P, g.fs, g.ts, dt)
    _, dx = impl.fold_varlen(dcols, g, lay)
    cu = lay["cu_tok"].tolist()
    g1 = Geo(g.P, g.fs, g.ts, g.F, g.T, 1, g.pattern)
    for b, te in enumerate(teff):
        one = packed_layout(g1, (te,), seed=k)
        _, c1 = impl.gather_varlen(x[b:b + 1].contiguous(), one, g.P, g.fs, g.ts, dt)
        equal(cols[cu[b]:cu[b + 1]], c1, f"clip {b} alone, gather")
        _, d1 = impl.fold_varlen(dcols[cu[b]:cu[b + 1]].contiguous(), g1, one)
        equal(dx[b:b + 1], d1, f"clip {b} alone, fold")


# ---- checkers: movers and casts ------------------------------------------------------------------------------------------------
def mover_rows(n, row_bytes):
    """[n][row_bytes / 4] int32 words, every one distinct"""
    w = row_bytes // 4
    return (torch.arange(n * w, dtype=I32) + 1).view(n, w)


def check_gather_scatter(impl, row_bytes):
    n = 23
    src = mover_rows(n, row_bytes)
    gen = torch.Generator().manual_seed(row_bytes)
    perm = torch.randperm(n, generator=gen).to(I32)
    repeats = torch.tensor([0, n - 1, 5, 5, n - 1, 0, 7], dtype=I32)
    # offset: `in` and `out` one 4-byte word off 16-byte alignment -- the entries then move 4-byte words whatever row_bytes is
    for off, idx in enumerate((perm, repeats, torch.tensor([n - 1], dtype=I32))):
        rc, out = impl.gather_rows(src, idx, offset=off % 2)
        ok(rc, f"gather_rows {row_bytes}")
        equal(out, src[idx.long()], f"gather_rows {row_bytes}")
    for off, idx in enumerate((perm, perm[:9], torch.tensor([0, n - 1], dtype=I32))):
        inp = mover_rows(idx.numel(), row_bytes)
        rc, out = impl.scatter_rows(inp, idx, n, offset=off % 2)
        ok(rc, f"scatter_rows {row_bytes}")
        want = torch.full((n, row_bytes // 4), SENTINEL).view(I32).clone()
        want[idx.long()] = inp
        equal(out.view(I32), want, f"scatter_rows {row_bytes}: named rows hold the input, every other row is untouched")


def tail_cases():
    out = []
    j = 0
    for M in (7, 10):
        for D in (4, 260):
            for n_idx in (0, 1, M):
                for lp in (None, PA_F32, PA_BF16):
                    out.append((M, D, n_idx, lp, ((1, 1), (1, 0), (0, 1), (0, 0))[j % 4], ("integer", "tie")[j % 2]))
                    j += 1
    return out


def check_tail_inject(impl, M, D, n_idx, lp, adds, fam):
    idx = torch.arange(M, dtype=I32) if n_idx == M else torch.tensor([M - 2][:n_idx], dtype=I32)
    if fam == "integer":
        rows, a0, a1 = integer_fam(max(n_idx, 1), D)[:n_idx], integer_fam(M, D) * 3, integer_fam(M, D).flip(0)
    else:                                            # one tie value per element, everything else 0: dx is the value, dx_lp its rounding
        rows, a0, a1 = torch.zeros(n_idx, D), tie_tensor(M, D), torch.zeros(M, D)
        adds = (1, adds[1])
    add0, add1 = (a0 if adds[0] else None), (a1 if adds[1] else None)
    rc, dx, dx_lp = impl.tail_inject(rows, idx, add0, add1, M, D, lp)
    what = f"tail_inject M{M} D{D} n{n_idx} lp{lp} adds{adds} {fam}"
    ok(rc, what)
    want = torch.zeros(M, D)
    for a in (add0, add1):
        if a is not None:
            want = want + a
    if n_idx:
        want[idx.long()] += rows
    check_cast(dx, want, PA_F32, what)
    named = torch.zeros(M, dtype=torch.bool)
    named[idx.long()] = True
    if add0 is None and add1 is None:
        assert bool((dx[~named] == 0).all()), what + ": an untouched row is not exactly 0"
    if lp is None:
        assert dx_lp is None
    else:
        check_cast(dx_lp, want, lp, what + " dx_lp")


def transpose_cases():
    out = []
    j = 0
    for R in TRANSPOSE_RC:
        for C in TRANSPOSE_RC:
            ldo = (R, R + 3, cdiv(R, 64) * 64 + 5)[j % 3]          # the last opens a further 64-tile of pure zero fill
            out.append((R, C, C + (0, 5)[j % 2], ldo, DT_PAIRS[j % 4], "code"))
            j += 1
    out += [(65, 130, 133, 133, (PA_F32, PA_BF16), "tie"), (130, 63, 63, 130, (PA_F32, PA_BF16), "tie")]
    return out


def check_transpose(impl, R, C, ldi, ldo, pair, fam):
    in_dt, out_dt = pair
    if fam == "tie":
        src = tie_tensor(R, C)
    elif PA_BF16 in pair:
        src = code_bf16(R, C)
    else:
        src = code_f32(R, C)
    inp = torch.full((R, ldi), float("nan"), dtype=TD[in_dt])
    inp[:, :C] = src.to(TD[in_dt])
    rc, out = impl.transpose(inp, R, C, out_dt, ldo)
    what = f"transpose {R}x{C} ldi{ldi} ldo{ldo} {pair} {fam}"
    ok(rc, what)
    check_cast(out[:, :R], src.to(TD[in_dt]).float().t().contiguous(), out_dt, what)
    assert bool((out[:, R:].float() == 0).all()), what + ": columns [R, ldo) are not zero-filled"


def stage_cases():
    """(shapes, which, dtype): both kernel paths (rows | cols % 4 == 0 or not), dst only / dst_t only / both, tile counts that are no
    multiple of the tile grid, more than 64 descriptors"""
    small = ((8, 12), (5, 7), (64, 64), (65, 130), (130, 4), (3, 64), (68, 72), (1, 1))
    which = ("dt", "d", "t")
    a = ([s for s in small], [which[j % 3] for j in range(len(small))])
    many = ([small[j % 4] if j % 5 else (66, 6) for j in range(70)], [which[(j // 2) % 3] for j in range(70)])
    return [(a[0], a[1], PA_BF16, "code"), (a[0], a[1], PA_F32, "code"), (many[0], many[1], PA_BF16, "code"),
            (a[0], a[1], PA_BF16, "tie")]


def stage_paths(shapes):
    return {"fast" if (r | c) % 4 == 0 else "scalar" for r, c in shapes}


def check_stage(impl, shapes, which, dt, fam):
    srcs = []
    for j, (r, c) in enumerate(shapes):
        if fam == "tie":
            srcs.append(tie_tensor(r, c))
        else:
            srcs.append(code_bf16(r, c).roll(j, 0) if dt == PA_BF16 else code_f32(r, c, base=1 + 1000 * j))
    rc, outs = impl.stage(srcs, dt, which)
    ok(rc, "stage_weights")
    for j, (s, w, (d, t)) in enumerate(zip(srcs, which, outs)):
        what = f"stage entry {j} {tuple(s.shape)} {w} dt{dt} {fam}"
        assert (d is not None) == ("d" in w) and (t is not None) == ("t" in w), what
        if d is not None:
            check_cast(d, s, dt, what + " dst")
        if t is not None:
            check_cast(t, s.t().contiguous(), dt, what + " dst_t")


ZERO2D_CASES = (("kernel", 9, 48, 80, 0), ("memset", 9, 48, 48, 0), ("memset", 5, 20, 20, 4), ("memset2d", 9, 44, 80, 0),
                ("memset2d", 9, 48, 80, 4), ("kernel", 1, 16, 32, 0))          # (route, rows, width, pitch, offset of ptr in bytes)


def zero2d_route(width, pitch, offset):
    if pitch != width and (offset | pitch | width) % 16 == 0:
        return "kernel"
    return "memset" if pitch == width else "memset2d"


def check_zero2d(impl, rows, width, pitch, offset):
    rc, buf = impl.zero2d(rows, width, pitch, offset)
    what = f"zero2d {rows}x{width} pitch{pitch} off{offset}"
    ok(rc, what)
    assert buf.shape == (rows, pitch) and buf.dtype == torch.uint8
    assert bool((buf[:, :width] == 0).all()), what + ": not zero"
    assert bool((buf[:, width:] == torch.full((rows, pitch // 4), SENTINEL).view(torch.uint8)[:, width:]).all()), what + ": the pitch gap lost its sentinel"


def check_converts(impl, n, in_offset=0):
    """pa_convert_f32 (both dtypes), pa_convert_to_f32 (both dtypes), code and tie families"""
    for dt in DTS:
        for fam in ("code", "tie"):
            x = tie_tensor(n) if fam == "tie" else (code_bf16(1, min(n, 513)).flatten().repeat(cdiv(n, 513))[:n] if dt == PA_BF16 else code_f32(n))
            rc, out = impl.convert(x, dt, in_offset)
            ok(rc, f"convert_f32 n{n}")
            check_cast(out, x, dt, f"convert_f32 n{n} dt{dt} {fam} offset{in_offset}")
        src = (tie_tensor(n) if dt == PA_F32 else rne_bf16(tie_tensor(n)))
        src = torch.where(torch.isnan(src.float()), torch.ones_like(src), src)
        rc, out = impl.convert_to_f32(src, in_offset)
        ok(rc, f"convert_to_f32 n{n}")
        equal(out, src.float(), f"convert_to_f32 n{n} dt{dt} offset{in_offset}")


def check_convert_rowscale(impl, M, D):
    rs = torch.tensor([1.0, 2.0, 0.5, 0.0, -1.0])[torch.arange(M) % 5]
    for dt in DTS:
        for fam in ("integer", "tie"):
            x = integer_fam(M, D) if fam == "integer" else tie_tensor(M, D)
            if fam == "tie":                         # 0 * inf and 0 * NaN stay NaN on both sides; keep the factor exact
                rs_ = torch.where(rs == 0, torch.ones_like(rs), rs)
            else:
                rs_ = rs
            rc, out = impl.convert_rowscale(x, rs_, dt)
            ok(rc, f"convert_rowscale {M}x{D}")
            check_cast(out, x * rs_[:, None], dt, f"convert_rowscale {M}x{D} dt{dt} {fam}")


# ---- second trips of the capped grids -------------------------------------------------------------------------------------------
def check_second_trip(impl, entry, a):
    if entry.startswith("patch_rows"):
        B, Np, D = a["B"], a["Np"], a["D"]
        assert B * Np * D > TRIP[entry] and (D % 8 == 0) == (entry == "patch_rows_vec")
        c = PG(Np, D, B, 0, 1, 0, 0, PA_BF16 if entry == "patch_rows_vec" else PA_F32, "integer", rows_only=True)
        dtok = integer_fam(B * c.Ntok, D).view(B, c.Ntok, D)
        z = torch.zeros(Np, dtype=I32)
        rc, o = impl.patch_bwd(dtok, z, z, c, None)
        ok(rc, entry)
        check_cast(o["dpatch"], dtok[:, 2:].reshape(B * Np, D), c.dt, entry)
    elif entry == "convert_f32":
        assert a["n"] > TRIP[entry]
        x = integer_fam(1, a["n"]).flatten()
        for dt in DTS:
            rc, out = impl.convert(x, dt, 0)
            ok(rc, entry)
            check_cast(out, x, dt, entry)
    elif entry == "convert_to_f32":
        assert a["n"] > TRIP[entry]
        x = integer_fam(1, a["n"], BF16).flatten()
        for off in (0, 1):                           # a misaligned `in`: the kernel tests the pointers and takes its scalar path
            rc, out = impl.convert_to_f32(x, off)
            ok(rc, entry)
            equal(out, x.float(), f"{entry} offset {off}")
    elif entry == "convert_rowscale":
        M, D = a["M"], a["D"]
        assert M * D > TRIP[entry]
        x, rs = integer_fam(M, D), torch.tensor([1.0, 2.0, 0.5])[torch.arange(M) % 3]
        rc, out = impl.convert_rowscale(x, rs, PA_BF16)
        ok(rc, entry)
        check_cast(out, x * rs[:, None], PA_BF16, entry)
    else:
        assert a["rows"] * a["width"] > TRIP[entry] and zero2d_route(a["width"], a["pitch"], 0) == "kernel"
        check_zero2d(impl, a["rows"], a["width"], a["pitch"], 0)


# ---- refusals: launch nothing ----------------------------------------------------------------------------------------------------
def refusal_table(q, q4, q2):
    """(what, entry name, arguments, expected code).  q: a 16-byte aligned host address, q4 = q + 4, q2 = q + 2 -- every call must be
    refused before anything is launched, so the table runs without a device.  Order of the checks of the patch entries: NULL
    pointers and scalars, dtype, alignment (all PA_EINVAL), then size limits (PA_EUNSUPPORTED)."""
    E, U = PA_EINVAL, PA_EUNSUPPORTED
    N = None
    bwd = lambda **kw: _args(dict(dtok=q, B=2, Ntok=6, D=8, pf=q, pt=q, Np=4, toff=0, Tpe=3, Fpe=3, gsum=q, d_cls=q, d_dist=q, d_npe=q, d_bias=q,       # noqa: E731
                                  d_tpos=q, d_fpos=q, acc=0, dpatch=q, dtype=PA_BF16, st=N), kw)
    gat = lambda **kw: _args(dict(x=q, B=1, F=8, T=8, pf=q, pt=q, Np=1, P=4, fs=2, ts=2, cols=q, dtype=PA_F32, st=N), kw)       # noqa: E731
    tab = lambda **kw: _args(dict(bias=q, tpos=q, Tpe=3, fpos=q, Fpe=3, pf=q, pt=q, Np=4, toff=0, D=8, table=q, cls=q, dist=q, npe=q, tok=q, B=1,       # noqa: E731
                                  Ntok=6, st=N), kw)
    fold = lambda **kw: _args(dict(dcols=q, dtype=PA_BF16, B=1, Np=1, pf=q, pt=q, P=4, fs=2, ts=2, F=8, T=8, ws=q, dx=q, st=N), kw)       # noqa: E731
    foldv = lambda **kw: _args(dict(dcols=q, dtype=PA_BF16, cu=q, B=1, P=4, fs=2, ts=2, F=8, T=8, dx=q, st=N), kw)       # noqa: E731
    foldr = lambda **kw: _args(dict(dcols=q, dtype=PA_BF16, M=4, slot=q, B=1, Tg=3, P=4, fs=2, ts=2, F=8, T=8, dx=q, st=N), kw)       # noqa: E731
    tail = lambda **kw: _args(dict(rows=q, idx=q, n=1, add0=q, add1=q, dx=q, dx_lp=q, dtype=PA_BF16, M=4, D=8, st=N), kw)       # noqa: E731
    rowsc = lambda **kw: _args(dict(inp=q, rs=q, out=q, M=4, D=8, dtype=PA_BF16, st=N), kw)       # noqa: E731
    gr = lambda **kw: _args(dict(inp=q, idx=q, n=1, rb=16, out=q, st=N), kw)       # noqa: E731
    rows = [("bwd: unknown dtype with non-NULL gradients", "pa_patch_bwd", bwd(dtype=7), E),
            ("bwd: unknown dtype, rows only", "pa_patch_bwd", bwd(dtype=7, gsum=N, d_cls=N, d_dist=N, d_npe=N, d_bias=N, d_tpos=N, d_fpos=N), E),
            ("bwd: Tpe = 0", "pa_patch_bwd", bwd(Tpe=0), E), ("bwd: Fpe = 0", "pa_patch_bwd", bwd(Fpe=-1), E),
            ("bwd: Ntok < Np + 2", "pa_patch_bwd", bwd(Ntok=5), E), ("bwd: some gradients NULL", "pa_patch_bwd", bwd(d_bias=N), E),
            ("bwd: dtok off 16 bytes", "pa_patch_bwd", bwd(dtok=q4), E), ("bwd: gsum off 16 bytes", "pa_patch_bwd", bwd(gsum=q4), E),
            ("bwd: dpatch off 16 bytes", "pa_patch_bwd", bwd(dpatch=q2), E), ("bwd: dtok NULL", "pa_patch_bwd", bwd(dtok=N), E),
            ("gather: F < P", "pa_patch_gather", gat(F=3), E), ("gather: T < P", "pa_patch_gather", gat(T=3), E),
            ("gather: fstride 0", "pa_patch_gather", gat(fs=0), E), ("gather: tstride < 0", "pa_patch_gather", gat(ts=-1), E),
            ("gather: unknown dtype", "pa_patch_gather", gat(dtype=7), E), ("gather: P P > 1024", "pa_patch_gather", gat(P=33, F=40, T=40), U),
            ("table: Np = 0", "pa_patch_pos_table", tab(Np=0), E), ("table: B = 0", "pa_patch_pos_table", tab(B=0), E),
            ("table: Np = B = 0", "pa_patch_pos_table", tab(Np=0, B=0), E), ("table: D = 0", "pa_patch_pos_table", tab(D=0), E),
            ("table: Tpe = 0", "pa_patch_pos_table", tab(Tpe=0), E), ("table: Fpe = 0", "pa_patch_pos_table", tab(Fpe=0), E),
            ("table: Ntok < 2", "pa_patch_pos_table", tab(Ntok=1), E),
            ("fold: dx off 16 bytes", "pa_patch_input_bwd", fold(dx=q4), E), ("fold: bf16 dcols off 4 bytes", "pa_patch_input_bwd", fold(dcols=q2), E),
            ("fold: unknown dtype", "pa_patch_input_bwd", fold(dtype=7), E), ("fold: Np above the grid", "pa_patch_input_bwd", fold(Np=10), U),
            ("fold_varlen: dx off 16 bytes", "pa_patch_input_bwd_varlen", foldv(dx=q4), E),
            ("fold_varlen: dcols off 4 bytes", "pa_patch_input_bwd_varlen", foldv(dcols=q2), E),
            ("fold_rows: dx off 16 bytes", "pa_patch_input_bwd_rows", foldr(dx=q4), E),
            ("fold_rows: dcols off 4 bytes", "pa_patch_input_bwd_rows", foldr(dcols=q2), E),
            ("tail_inject: rows off 16 bytes", "pa_tail_inject", tail(rows=q4), E), ("tail_inject: add0", "pa_tail_inject", tail(add0=q4), E),
            ("tail_inject: add1", "pa_tail_inject", tail(add1=q4), E), ("tail_inject: dx", "pa_tail_inject", tail(dx=q4), E),
            ("tail_inject: dx_lp", "pa_tail_inject", tail(dx_lp=q4), E), ("tail_inject: D % 4", "pa_tail_inject", tail(D=6), U),
            ("rowscale: in off 16 bytes", "pa_convert_f32_rowscale", rowsc(inp=q4), E),
            ("rowscale: out off 16 bytes", "pa_convert_f32_rowscale", rowsc(out=q4), E),
            ("rowscale: unknown dtype", "pa_convert_f32_rowscale", rowsc(dtype=7), E),
            ("gather_rows: in off 4 bytes", "pa_gather_rows", gr(inp=q2), E), ("gather_rows: out off 4 bytes", "pa_gather_rows", gr(out=q2), E),
            ("scatter_rows: in off 4 bytes", "pa_scatter_rows", gr(inp=q2), E), ("scatter_rows: row_bytes % 4", "pa_scatter_rows", gr(rb=6), E)]
    return rows


def _args(base, over):
    assert set(over) <= set(base), over
    base.update(over)
    return list(base.values())


# ---- the suite: what both test files run -----------------------------------------------------------------------------------------
FORMS = ("fixed", "varlen", "rows")
FOLD_FAMS = ("order", "integer")


def fold_extra_cases(P, fs, ts):
    """fixed fold: Np equal to the grid size (pattern full has it) and a pair outside the grid; rows fold: table entries -2, M, M + 7"""
    g = geo_cases(P, fs, ts)[1]
    return dict(fixed=[Geo(g.P, g.fs, g.ts, g.F, g.T, g.B, "outside")], rows=[Geo(g.P, g.fs, g.ts, g.F, g.T, 3, "odd")], varlen=[])


def run_folds(impl, geom, form):
    cases = geo_cases(*geom) + fold_extra_cases(*geom)[form]
    for k, g in enumerate(cases):
        for dt in DTS:
            for fam in FOLD_FAMS:
                if form == "fixed":
                    check_fold_fixed(impl, g, dt, fam)
                elif form == "varlen":
                    check_fold_varlen(impl, g, dt, fam, k)
                else:
                    check_fold_rows(impl, g, dt, fam, k)


def run_gathers(impl, geom):
    for k, g in enumerate(geo_cases(*geom)):
        for dt in DTS:
            check_gather_fixed(impl, g, dt)
            check_gather_varlen(impl, g, dt, k=k, outside=k % 2 == 1)
        check_gather_fixed(impl, g, PA_BF16, "tie")
        check_gather_varlen(impl, g, PA_BF16, "tie", k=k)


def run_tables(impl, geom):
    for k, g in enumerate(geo_cases(*geom)):
        D = PG_D[k % 4]
        check_pos_table(impl, g, D, (0, 3)[k % 2], (0, 5)[(k // 2) % 2])
        check_pos_table_varlen(impl, g, D, k)
        check_pos_table_varlen(impl, g, D, k, toffs=[(0, 3, 1)[b % 3] for b in range(g.B)])


def run_packed_grads(impl, geom, form, rec=None):
    for k, g in enumerate(geo_cases(*geom) + fold_extra_cases(*geom)["rows" if form == "rows" else "varlen"]):
        for j, fam in enumerate(("integer", "graded")):
            check_bwd_packed(impl, g, PACKED_D[(k + j) % 4], fam, (k + j) % 2, form, k, rec)


def run_noop(impl):
    """all six NULL: nothing is launched, outputs keep the sentinel (the impl returns None for 'no output was touched')"""
    g = geo_cases(4, 3, 3)[1]
    lay = packed_layout(g, varlen_teff(g, 0))
    dtok = packed_dtok(lay["M"], 16, "integer")
    rc, o = impl.bwd_varlen(dtok, lay, g.B, lay["Tg"], g.Fg, None, 0, none=True)
    assert rc == PA_OK and o is None
    rc, o = impl.bwd_rows(dtok, lay, torch.zeros(g.B, dtype=I32), g.B, lay["Tg"], g.Fg, None, 0, none=True)
    assert rc == PA_OK and o is None


def run_cross_entry(impl):
    for geom in GEOMS:
        F, T = (36, 50) if geom == MODEL_GEOM else (geom[0] + 2 * geom[1] + 3, geom[0] + 3 * geom[2] + 2)
        for dt in DTS:
            check_packed_equals_fixed(impl, Geo(*geom, F, T, 3, "full"), dt)
            check_clip_alone(impl, Geo(*geom, F, T, 3, "full"), dt, k=(0, 1)[dt])


def run_tie_dpatch(impl):
    """dpatch: the 8-element vector store (D % 8 == 0) and the scalar path, on the tie family"""
    for D in (16, 5):
        c = PG(17, D, 2, 0, 1, 1, 0, PA_BF16, "tie", rows_only=True)
        dtok = tie_tensor(c.B, c.Ntok, D)
        z = torch.zeros(c.Np, dtype=I32)
        rc, o = impl.patch_bwd(dtok, z, z, c, None)
        ok(rc, c.name)
        check_cast(o["dpatch"], dtok[:, 2:2 + c.Np].reshape(-1, D), PA_BF16, c.name)


def run_movers(impl, which):
    if which == "gather_scatter":
        for rb in ROW_BYTES:
            check_gather_scatter(impl, rb)
    elif which == "tail_inject":
        for a in tail_cases():
            check_tail_inject(impl, *a)
    elif which == "transpose":
        for a in transpose_cases():
            check_transpose(impl, *a)
    elif which == "stage":
        for a in stage_cases():
            check_stage(impl, *a)
    elif which == "zero2d":
        for route, rows, width, pitch, off in ZERO2D_CASES:
            assert zero2d_route(width, pitch, off) == route
            check_zero2d(impl, rows, width, pitch, off)
    else:
        for n, off in ((1, 0), (3, 0), (4, 0), (1029, 0), (1029, 1), (2051, 3)):      # pa_convert_f32 / _to_f32 take their scalar path off 16 bytes
            check_converts(impl, n, off)
        for M, D in ((1, 4), (7, 260), (33, 8)):
            check_convert_rowscale(impl, M, D)


MOVERS = ("gather_scatter", "tail_inject", "transpose", "stage", "zero2d", "converts")

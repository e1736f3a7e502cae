"""The exact parity suite of the patch stage and the data movers checks itself (no GPU): every checker of tests/patch_cases.py passes
against TorchPatch, plain f32 torch, at every case the GPU suite runs, so every torch.equal and the one derived bound are ones an
honest implementation meets; the lists reach every code path they were derived for; thirteen small wrong variants of the torch
implementation are each rejected by at least one checker; and every refusal of the patch and mover entries is asserted through the
built library, which launches nothing and therefore needs no device."""
import ctypes

import pytest
import torch

from tests import patch_cases as P
from tests.patch_cases import PA_BF16, PA_F32, Geo, TorchPatch

IMPL = TorchPatch()


# ---- every case of the GPU suite -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("geom", P.GEOMS, ids=str)
def test_folds(geom, form):
    P.run_folds(IMPL, geom, form)


@pytest.mark.parametrize("geom", P.GEOMS, ids=str)
def test_gathers_and_tables(geom):
    P.run_gathers(IMPL, geom)
    P.run_tables(IMPL, geom)


@pytest.mark.parametrize("c", P.pg_cases(), ids=lambda c: c.name)
def test_patch_bwd(c):
    P.check_patch_bwd(IMPL, c)


@pytest.mark.parametrize("form", ("varlen", "rows"))
@pytest.mark.parametrize("geom", P.GEOMS, ids=str)
def test_packed_gradients(geom, form):
    P.run_packed_grads(IMPL, geom, form)


def test_cross_entry_equalities_noop_and_tie_dpatch():
    P.run_cross_entry(IMPL)
    P.run_noop(IMPL)
    P.run_tie_dpatch(IMPL)


@pytest.mark.parametrize("which", P.MOVERS)
def test_movers(which):
    P.run_movers(IMPL, which)


@pytest.mark.parametrize("entry,args", P.SECOND_TRIP, ids=[e for e, _ in P.SECOND_TRIP])
def test_second_trips(entry, args):
    P.check_second_trip(IMPL, entry, args)


# ---- the lists hold what they are meant to hold ----------------------------------------------------------------------------------
def test_operand_families_are_what_they_claim():
    v = P.tie_values()
    bits = v.view(torch.int32) & 0xFFFF
    lo, hi = P.TIE_CLASSES["tie"]
    assert bool((bits[lo:lo + 2] == 0x8000).all()), "exact ties"
    assert {int(b) for b in bits[2:6]} == {0x7FFF, 0x8001}, "one ulp on either side"
    assert ((int(v.view(torch.int32)[0]) >> 16) & 1) == 0 and ((int(v.view(torch.int32)[1]) >> 16) & 1) == 1, "even and odd kept mantissa"
    assert float(v[10]) == torch.finfo(torch.float32).max and bool(torch.isinf(P.rne_bf16(v[10:11])).all()), "the largest finite f32 rounds to inf"
    assert float(v[13]) == torch.finfo(torch.float32).tiny
    lo, hi = P.TIE_CLASSES["subnormal"]
    assert bool((v[lo:hi].abs() < torch.finfo(torch.float32).tiny).all()) and bool((v[lo:hi] != 0).all())
    assert bool((v[21:42] == -v[0:21]).all()) and bool(torch.isnan(v[42:]).all())
    # truncation differs from round-to-nearest-even on the family, so the tie checks can tell them apart
    trunc = (v.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    assert int((trunc.view(torch.int16) != P.rne_bf16(v).view(torch.int16)).sum()) >= 10
    c = P.code_bf16(40, 513)
    assert all(len(set(r.tolist())) == 513 for r in c) and float(c.abs().max()) <= 256
    i = P.integer_fam(300, 300)
    assert float(i.abs().max()) <= 127 and torch.equal(i, i.round()) and torch.equal(i.to(torch.bfloat16).float(), i)


@pytest.mark.parametrize("geom", P.GEOMS, ids=str)
def test_fold_lists_reach_every_path(geom):
    cases = P.geo_cases(*geom)
    Pp, fs, ts = geom
    if geom == P.MODEL_GEOM:
        assert {(g.F, g.T) for g in cases} == {(36, 50)}
    else:
        assert {g.T % 4 for g in cases} == {0, 1, 2, 3}
        assert any((g.B * g.F * g.T) % 4 for g in cases), "the tail at the end of dx"
        # (the strip is (F - P) mod fstride pixels: stride 2 leaves room for one)
        assert all(g.F - ((g.Fg - 1) * fs + Pp) >= P.strip_min(fs) for g in cases), "the zero strip behind the last patch row"
        wide = [g for g in cases if g.T - ((g.Tg - 1) * ts + Pp) >= P.strip_min(ts)]
        # (tstride 2 and 4: the strip is a function of T % 4, so only some residues have one)
        assert len(wide) >= (2 if ts in (2, 4) else len(cases)), "the zero strip behind the last patch column"
    assert any(g.B * g.F * g.T > 1024 for g in cases), "more than one workgroup"
    assert {g.pattern for g in cases} >= {"full", "random", "one", "empty_row", "empty_col"} and {g.B for g in cases} == {1, 3}
    paths = {dt: set().union(*(P.fold_paths(g, dt) for g in cases)) for dt in P.DTS}
    want = {"inside", "multi"} | ({"straddle", "tail", "strip"} if geom != P.MODEL_GEOM else set())
    assert paths[PA_F32] >= want and paths[PA_BF16] >= want, (paths, want)
    if Pp % 2:
        assert "pair" not in paths[PA_BF16] and "nopair" in paths[PA_BF16], "odd P: the bf16 pair read must not be taken"
    else:
        assert "pair" in paths[PA_BF16]
    if ts % 2:
        assert "nopair" in paths[PA_BF16], "odd tstride: odd offsets into the patch row"
    # the packed forms: clip lengths that give T_eff in {0, 1, 2, Tg}, cu_tok difference 2 for a clip without a patch column
    for g in cases:
        seen = set()
        for k in range(3):
            te = P.varlen_teff(g, k)
            seen |= set(te)
            lay = P.packed_layout(g, te)
            d = (lay["cu_tok"][1:] - lay["cu_tok"][:-1]).tolist()
            assert all((x == 2) == (t == 0) for x, t in zip(d, te))
        assert seen >= ({1, 2, g.Tg} if g.B == 1 else {0, 1, 2, g.Tg})
    ex = P.fold_extra_cases(*geom)
    pf, pt = P.kept_patches(ex["fixed"][0])
    assert ex["fixed"][0].pattern == "outside" and ex["rows"][0].pattern == "odd"
    lay = P.rows_layout(ex["rows"][0])
    odd = set(lay["slot"].flatten().tolist())
    assert {-1, -2, lay["M"]} <= odd, "table entries -1, -2 and M"
    full = [g for g in cases if g.pattern == "full"][0]
    assert P.kept_patches(full)[0].numel() == full.Fg * full.Tg, "Np equal to the grid size"


def test_geometry_families():
    assert set(P.GEOMS) == {(4, 3, 3), (4, 4, 4), (4, 6, 5), (3, 2, 2), (16, 10, 10)}
    seen = set()
    for geom in P.GEOMS:
        for g in P.geo_cases(*geom):
            seen |= P.fold_paths(g, PA_BF16)
    assert seen >= {"inside", "straddle", "tail", "multi", "pair", "nopair", "strip", "gaps", "overlap"}


def test_parameter_gradient_lists_reach_every_path():
    cases = [c for c in P.pg_cases() if not c.rows_only]
    assert {c.Np for c in cases} == set(P.PG_NP) == {1, 15, 16, 17, 31, 32, 33, 49}
    assert {c.D for c in cases} == {5, 16, 24, 100} and {c.B for c in cases} == {1, 3, 4, 5, 9}
    assert {c.toff for c in cases} == {0, 3} and {c.acc for c in cases} == {0, 1} and {c.dt for c in cases} == {PA_F32, PA_BF16}
    assert {c.extra for c in cases} == {0, 5} and {c.fam for c in cases} == {"integer", "graded"}
    paths = set().union(*(P.pg_paths(c) for c in cases))
    assert paths >= {"sum_vec", "sum_scalar", "pairs", "no_pairs", "remainder", "no_remainder", "rows_vec", "rows_scalar", "d_mask", "d_full",
                     "toff_edge", "sum_rem0", "sum_rem1", "sum_only_rem1", "sum_only_rem3"}, paths
    for c in cases:
        pf, pt = P.pg_patches(c)
        assert pf.numel() == c.Np and len({(int(a), int(b)) for a, b in zip(pf, pt)}) == c.Np, "distinct pairs"
        assert int(pt.max()) == P.PG_GRID[1] - 1
    assert any(c.toff + P.PG_GRID[1] - 1 == c.Tpe - 1 for c in cases)
    assert sum(c.rows_only for c in P.pg_cases()) == 2
    # per-clip offsets of the rows form: p - toff[b] both negative and >= Tg for some time position p
    g = P.geo_cases(4, 3, 3)[1]
    lay = P.rows_layout(g, 1)
    Tpe, Tg = lay["Tg"] + 3, lay["Tg"]
    toffs = [(0, 3, 1)[(b + 1) % 3] for b in range(g.B)]
    diffs = {p - t for p in range(Tpe) for t in toffs}
    assert min(diffs) < 0 and max(diffs) >= Tg


def test_mover_and_trip_lists():
    for entry, a in P.SECOND_TRIP:
        n = {"patch_rows_vec": lambda: a["B"] * a["Np"] * a["D"], "patch_rows_scalar": lambda: a["B"] * a["Np"] * a["D"],
             "convert_f32": lambda: a["n"], "convert_to_f32": lambda: a["n"], "convert_rowscale": lambda: a["M"] * a["D"],
             "zero2d": lambda: a["rows"] * a["width"]}[entry]()
        assert P.TRIP[entry] < n < 1.01 * P.TRIP[entry] + 4096, (entry, n)
    assert {e for e, _ in P.SECOND_TRIP} == set(P.TRIP)
    assert P.ROW_BYTES == (4, 12, 16, 2044, 2048, 4112)
    tc = P.transpose_cases()
    assert {(r, c) for r, c, *_ in tc} >= {(r, c) for r in P.TRANSPOSE_RC for c in P.TRANSPOSE_RC}
    assert {p for *_, p, fam in tc} == set(P.DT_PAIRS)
    assert any(ldi > C for _, C, ldi, *_ in tc) and any(-(-ldo // 64) > -(-R // 64) for R, _, _, ldo, *_ in tc), "a further 64-tile of zero fill"
    sc = P.stage_cases()
    assert all(P.stage_paths(s) == {"fast", "scalar"} for s, *_ in sc)
    assert any(len(s) > 64 for s, *_ in sc) and {w for _, ws, *_ in sc for w in ws} == {"d", "t", "dt"}
    assert any((-(-r // 64)) * (-(-c // 64)) > 1 for s, *_ in sc for r, c in s)
    assert {r for r, *_ in P.ZERO2D_CASES} == {"kernel", "memset", "memset2d"}
    t = P.tail_cases()
    assert {a[0] % 4 for a in t} - {0} and {a[1] for a in t} == {4, 260} and {a[3] for a in t} == {None, PA_F32, PA_BF16}
    assert {a[4] for a in t} == {(1, 1), (1, 0), (0, 1), (0, 0)} and {a[2] for a in t if a[0] == 7} == {0, 1, 7}


# ---- fault models ------------------------------------------------------------------------------------------------------------------
class DroppedKept(TorchPatch):
    def kept(self, r, rows):
        return -rows <= r < rows                    # -1 reads the last row instead of being skipped


class LastColumnLost(TorchPatch):
    def fold_finish(self, dx):
        if dx.shape[2] % 4:
            dx[:, :, -1] = P.SENTINEL               # the straddling vector never stored
        return dx


class CoverLoOffByOne(TorchPatch):
    def cover_lo(self, c, Pp, stride):
        return (c - Pp) // stride + 2 if c >= Pp else 0


class FoldColumnMajor(TorchPatch):
    def fold_order(self, cells):
        return sorted(cells, key=lambda c: (c[1], c[0]))


class StridesSwapped(TorchPatch):
    def gather_strides(self, fs, ts):
        return ts, fs


class TableIgnoresToff(TorchPatch):
    def table_toff(self, toff):
        return 0


class RowsIgnoreToff(TorchPatch):
    def rows_toff(self, toff):
        return 0


class LastPatchDropped(TorchPatch):
    def grad_patches(self, Np):
        return Np - 1 if Np % 16 == 1 and Np > 1 else Np


class AccumulateIgnored(TorchPatch):
    def start_of(self, start, acc):
        return None


class DpatchFromRow0(TorchPatch):
    def dpatch_first(self):
        return 0


class PrefixRowsNonZero(TorchPatch):
    def prefix_cols(self, v):
        return torch.ones_like(v)


class TransposeNoFill(TorchPatch):
    def transpose_fill(self, out, R):
        pass


class Truncating(TorchPatch):
    def cast(self, v, dt):
        if dt == PA_F32:
            return v
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


G433, G465 = P.geo_cases(4, 3, 3), P.geo_cases(4, 6, 5)
PG17 = [c for c in P.pg_cases() if c.Np == 17 and not c.rows_only]
PG_ACC = [c for c in P.pg_cases() if c.acc and not c.rows_only]
# (fault, the checker runs of which at least one must fail)
FAULTS = (
    ("a fold that treats a dropped patch as kept", DroppedKept, [lambda i: P.check_fold_fixed(i, G433[1], PA_F32, "integer"),
                                                                  lambda i: P.check_fold_rows(i, G433[1], PA_F32, "integer", 1)]),
    ("a fold that drops the last column when T % 4 != 0", LastColumnLost, [lambda i: P.check_fold_fixed(i, G433[1], PA_F32, "integer")]),
    ("cover_range low bound off by one", CoverLoOffByOne, [lambda i: P.check_fold_fixed(i, G433[0], PA_F32, "integer")]),
    ("strides swapped in the gather", StridesSwapped, [lambda i: P.check_gather_fixed(i, G465[0], PA_F32)]),
    ("toff ignored in the table", TableIgnoresToff, [lambda i: P.check_pos_table(i, G433[1], 16, 3, 0)]),
    ("toff[b] ignored in the rows gradients", RowsIgnoreToff, [lambda i: P.check_bwd_packed(i, G433[1], 16, "integer", 0, "rows", 1)]),
    ("the last patch dropped when Np % 16 == 1", LastPatchDropped, [lambda i, c=c: P.check_patch_bwd(i, c) for c in PG17]),
    ("accumulate ignored", AccumulateIgnored, [lambda i, c=c: P.check_patch_bwd(i, c) for c in PG_ACC[:2]]),
    ("dpatch starting at row 0 instead of 2", DpatchFromRow0, [lambda i: P.check_patch_bwd(i, PG17[0])]),
    ("non-zero prefix rows in the packed gather", PrefixRowsNonZero, [lambda i: P.check_gather_varlen(i, G433[0], PA_F32)]),
    ("a transpose without zero fill", TransposeNoFill, [lambda i: P.check_transpose(i, 63, 65, 65, 69, (PA_F32, PA_F32), "code")]),
    ("bf16 by truncation instead of round-to-nearest-even", Truncating,
     [lambda i: P.check_gather_fixed(i, G433[0], PA_BF16, "tie"), lambda i: P.check_transpose(i, 65, 130, 133, 133, (PA_F32, PA_BF16), "tie"),
      lambda i: P.check_converts(i, 1029), lambda i: P.run_tie_dpatch(i), lambda i: P.check_convert_rowscale(i, 7, 260),
      lambda i: P.check_stage(i, *P.stage_cases()[3]), lambda i: P.check_tail_inject(i, 7, 260, 0, PA_BF16, (1, 0), "tie")]),
)


@pytest.mark.parametrize("what,cls,runs", FAULTS, ids=[f[0] for f in FAULTS])
def test_fault_model_is_rejected(what, cls, runs):
    for run in runs:
        run(IMPL)                                    # the honest implementation passes the very same run
    caught = 0
    for run in runs:
        try:
            run(cls())
        except AssertionError:
            caught += 1
    need = len(runs) if cls is Truncating else 1     # every one of the seven conversion sites is pinned
    assert caught >= need, f"{what}: rejected by {caught} of {len(runs)} checker runs"


def test_fold_order_is_seen_by_the_order_family_only():
    """a fold that adds in (gt, gf) order: the integer family cannot see it (exact in any order), the order family must"""
    g = Geo(4, 2, 2, 12, 14, 3, "full")              # two-pixel overlaps: four terms at a quarter of the pixels
    bad = FoldColumnMajor()
    for dt in P.DTS:
        P.check_fold_fixed(bad, g, dt, "integer")
        P.check_fold_fixed(IMPL, g, dt, "order")
    with pytest.raises(AssertionError):
        P.check_fold_fixed(bad, g, PA_F32, "order")
    # bf16 dcols: four 8-bit significands within 2^6 of each other add exactly in f32, in any order -- nothing to see, and nothing
    # to get wrong
    P.check_fold_fixed(bad, g, PA_BF16, "order")


# ---- refusals through the built library: nothing is launched -----------------------------------------------------------------------
def test_refusals_launch_nothing():
    from passt_amd import _lib
    lib = _lib.load()
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 15) & ~15
    rows = P.refusal_table(base, base + 4, base + 2)
    assert len(rows) >= 40
    for what, entry, args, want in rows:
        got = getattr(lib, entry)(*args)
        assert got == want, (what, entry, got, want)

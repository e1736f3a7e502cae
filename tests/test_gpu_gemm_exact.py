"""Exact-integer and guarded-buffer parity of the GEMM family -- pa_gemm_nt with every tile variant, epilogue and flag, its row-factor
and split-K forms, pa_gemm_tn and its batched forms, pa_reduce_partials behind them -- through the C ABI (tests/gemm_cases.py holds
the shapes, operand families, conditions, bounds and checkers; the same checkers pass against plain torch in
tests/test_gemm_cases_cpu.py).  The worst got / bound per group of the two non-exact epilogues goes to
gemm_exact_parity_metrics.json in $PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root, as in
tests/test_gpu_row_kernels.py); profiles/gemm_exact_parity.txt keeps them."""
import ctypes
import json
import os
from dataclasses import replace

import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from tests import gemm_cases as G  # noqa: E402
from tests.gemm_cases import DGELU, GELU, PA_BF16, PA_F32, PA_OK, PARTIAL, RESID, STORE, TD, GuardedOut  # noqa: E402

DEV = "cuda"
F32 = torch.float32
_METRICS = {}


def record(group, ratio):
    _METRICS[group] = max(_METRICS.get(group, 0.0), float(ratio))
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_metrics")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "gemm_exact_parity_metrics.json"), "w") as f:
        json.dump({k: {"worst_got_over_bound": v} for k, v in _METRICS.items()}, f, indent=1, sort_keys=True)


def guards_only(g, what):
    """a workspace or an opaque buffer: only its guards are checked"""
    buf = g.buf.cpu()
    assert bool((buf[:g.lo] == G.SENTINEL).all()) and bool((buf[g.lo + g.n:] == G.SENTINEL).all()), f"{what}: a write outside the buffer"


class Hip:
    """The C entries of libpasst_amd.so behind the calling conventions of gemm_cases.TorchGemm: a case and its CPU tensors in, guarded
    device buffers out.  Every operand is a view into a larger allocation with NaN on both sides (and in the gap columns of a padded
    leading dimension), every output a GuardedOut."""
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self.st = torch.cuda.current_stream().cuda_stream
        assert self.lib.pa_gemm_tn_step_rows() == G.TN_STEP_ROWS

    @staticmethod
    def gin(t, pad=0, offset=0):
        if t is None:
            return None
        return G.guarded_in(G.padded(t, t.shape[1] + pad) if pad else t, DEV, offset)

    # ---- pa_gemm_nt and its forms
    def nt(self, c, i, override=None):
        lib, td, pad = self.lib, TD[c.dt], c.pad
        a = _lib.GemmArgs()
        keep = [self.gin(i["A"], pad), self.gin(i["B"], pad), self.gin(i["bias"]), self.gin(i["rowscale"], offset=1)]
        a.dtype, a.epilogue, a.M, a.N, a.K, a.lda, a.ldb = c.dt, c.epi, c.M, c.N, c.K, c.K + pad, c.K + pad
        a.A, a.B, a.bias = keep[0].data_ptr(), keep[1].data_ptr(), (keep[2].data_ptr() if keep[2] is not None else None)
        a.split_k, a.tune, a.reserved, a.colscale_n, a.colscale = c.split_k, c.tune, c.flags, c.colscale_n, c.colscale
        outs, ld = {}, c.N + pad
        if c.epi in (STORE, GELU, DGELU):
            outs["out_lp"] = G.new_out(c.M, c.N, pad, td, DEV)
            a.out_lp, a.ldolp = outs["out_lp"].ptr(), ld
        if c.epi == GELU:
            outs["out_lp2"] = G.new_out(c.M, c.N, pad, td, DEV)
            a.out_lp2, a.ldolp2 = outs["out_lp2"].ptr(), ld
        if c.epi == RESID:
            if c.inplace:
                outs["out_f32"] = G.new_out(c.M, c.N, pad, F32, DEV, init=i["resid"])
                a.resid, a.ldr = outs["out_f32"].ptr(), ld
            else:
                outs["out_f32"] = G.new_out(c.out_rows, c.N, pad, F32, DEV)
                keep.append(self.gin(i["resid"], pad))
                a.resid, a.ldr = keep[-1].data_ptr(), ld
            a.out_f32, a.ldo32 = outs["out_f32"].ptr(), ld
            if c.row_mod:
                a.row_mod, a.out_batch_rows, a.out_row_off = c.row_mod, c.row_mod + G.REMAP_OFF, G.REMAP_OFF
        if c.epi == PARTIAL:
            outs["out_f32"] = G.new_out(c.split_k * c.M, c.N, pad, F32, DEV)
            a.out_f32, a.ldo32 = outs["out_f32"].ptr(), ld
        cws = None
        if c.epi == DGELU:
            keep.append(self.gin(i["aux"], pad))
            a.aux, a.ldaux = keep[-1].data_ptr(), ld
            if c.colsum:
                outs["colsum"] = GuardedOut(c.N, F32, DEV, init=i["start"] if c.colsum == "acc" else None)
                cws = GuardedOut(lib.pa_gemm_colsum_ws_floats(c.M, c.N), F32, DEV)
                a.colsum_out, a.colsum_ws, a.colsum_accumulate = outs["colsum"].ptr(), cws.ptr(), int(c.colsum == "acc")
                if c.colsum == "defer":
                    a.reserved |= G.COLSUM_DEFER
        for k, v in (override or {}).items():
            setattr(a, k, v)
        rs = keep[3].data_ptr() if keep[3] is not None else None
        ws = None
        if c.entry in ("splitk", "splitk_rowscale"):
            n = lib.pa_gemm_nt_splitk_ws_floats(c.M, c.N, c.K, c.epi, c.dt)
            n = n - 1 if c.ws == "small" else n
            ws = GuardedOut(max(n, 1), F32, DEV) if c.ws != "null" else None
            wp, wn = (ws.ptr(), n) if ws is not None else (None, 0)
        if c.entry == "nt":
            rc = lib.pa_gemm_nt(ctypes.byref(a), self.st)
        elif c.entry == "rowscale":
            rc = lib.pa_gemm_nt_rowscale(ctypes.byref(a), rs, self.st)
        elif c.entry == "splitk":
            rc = lib.pa_gemm_nt_splitk(ctypes.byref(a), wp, wn, self.st)
        else:
            rc = lib.pa_gemm_nt_splitk_rowscale(ctypes.byref(a), rs, wp, wn, self.st)
        if rc == PA_OK and c.colsum == "defer" and not override:
            rows = lib.pa_gemm_last_colsum_rows()
            assert 1 <= rows and rows * c.N <= cws.n, (rows, c.N, cws.n)
            assert bool((outs["colsum"].buf == G.SENTINEL).all()), "PA_GEMM_COLSUM_DEFER: colsum_out is not written"
            d = (_lib.ReduceDesc * 1)(_lib.ReduceDesc(cws.ptr(), outs["colsum"].ptr(), c.N, rows, 0, c.N, _lib.REDUCE_ROWS, 0))
            assert lib.pa_reduce_partials_batched(d, 1, self.st) == PA_OK
        torch.cuda.synchronize()
        for g, what in ((cws, "colsum_ws"), (ws, "split-K workspace")):
            if g is not None:
                guards_only(g, what)
        return rc, outs

    def mlp_blocked(self, c, i, i2):
        lib, td = self.lib, TD[c.dt]
        assert lib.pa_gemm_blocked_pre_ok(c.M, c.N, c.K) == 1
        keep = [self.gin(i["A"]), self.gin(i["B"]), self.gin(i["bias"]), self.gin(i2["A"]), self.gin(i2["B"])]
        pre = GuardedOut(lib.pa_gemm_blocked_pre_elems(c.M, c.N), td, DEV)
        act, dpre, cs = G.new_out(c.M, c.N, 0, td, DEV), G.new_out(c.M, c.N, 0, td, DEV), GuardedOut(c.N, F32, DEV)
        cws = GuardedOut(lib.pa_gemm_colsum_ws_floats(c.M, c.N), F32, DEV)
        a = _lib.GemmArgs()
        a.dtype, a.epilogue, a.M, a.N, a.K, a.lda, a.ldb, a.split_k = c.dt, GELU, c.M, c.N, c.K, c.K, c.K, 1
        a.A, a.B, a.bias, a.reserved = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), G.BLOCKED_PRE
        a.out_lp, a.ldolp, a.out_lp2, a.ldolp2 = pre.ptr(), c.N, act.ptr(), c.N
        rc = lib.pa_gemm_nt(ctypes.byref(a), self.st)
        if rc == PA_OK:
            b = _lib.GemmArgs()
            b.dtype, b.epilogue, b.M, b.N, b.K, b.lda, b.ldb, b.split_k = c.dt, DGELU, c.M, c.N, c.K, c.K, c.K, 1
            b.A, b.B, b.aux, b.ldaux, b.reserved = keep[3].data_ptr(), keep[4].data_ptr(), pre.ptr(), c.N, G.BLOCKED_PRE
            b.out_lp, b.ldolp, b.colsum_out, b.colsum_ws = dpre.ptr(), c.N, cs.ptr(), cws.ptr()
            rc = lib.pa_gemm_nt(ctypes.byref(b), self.st)
        torch.cuda.synchronize()
        guards_only(pre, "blocked pre-activation")
        guards_only(cws, "colsum_ws")
        return rc, dict(act=act, d_pre=dpre, colsum=cs)

    # ---- pa_gemm_tn and its forms
    def _tn_args(self, c, i, S, keep, override=None):
        a = _lib.GemmArgs()
        dY, X = self.gin(i["dY"], c.pad), self.gin(i["X"], c.pad)
        keep += [dY, X]
        a.dtype, a.epilogue, a.M, a.N, a.K, a.lda, a.ldb = c.dt, PARTIAL, c.M, c.N, c.T, c.M + c.pad, c.N + c.pad
        a.A, a.B, a.split_k, a.tune = dY.data_ptr(), X.data_ptr(), S, c.tune
        o = dict(out_f32=G.new_out(S * c.M, c.N, c.pad, F32, DEV), colsum_ws=GuardedOut((S, c.M), F32, DEV) if c.colsum else None)
        a.out_f32, a.ldo32 = o["out_f32"].ptr(), c.N + c.pad
        if c.colsum:
            a.colsum_ws = o["colsum_ws"].ptr()
        for k, v in (override or {}).items():
            setattr(a, k, v)
        return a, o

    def tn(self, c, i, override=None):
        keep = []
        a, o = self._tn_args(c, i, c.split_k, keep, override)
        rc = self.lib.pa_gemm_tn(ctypes.byref(a), self.st)
        torch.cuda.synchronize()
        return rc, o

    def tn_batched(self, cs, ins, plan=None, problem_major=False, override=None):
        keep, outs = [], []
        arr = (_lib.GemmArgs * len(cs))()
        for p, (c, i) in enumerate(zip(cs, ins)):
            arr[p], o = self._tn_args(c, i, plan[0] + 1 if plan else c.split_k, keep, (override or {}).get(p))
            outs.append(o)
        if problem_major:
            arr[0].tune = 2
        if plan:
            rc = self.lib.pa_gemm_tn_batched_plan(arr, len(cs), plan[0], plan[1], self.st)
        else:
            rc = self.lib.pa_gemm_tn_batched(arr, len(cs), self.st)
        torch.cuda.synchronize()
        return rc, outs

    def reduce(self, partial, accumulate, start, offset=0):
        S, n = partial.shape
        p = G.guarded_in(partial.contiguous(), DEV, offset)
        g = GuardedOut(n, F32, DEV, init=start if accumulate else None, offset=offset)
        assert self.lib.pa_reduce_partials(p.data_ptr(), S, n, g.ptr(), int(accumulate), self.st) == PA_OK
        torch.cuda.synchronize()
        return g


@pytest.fixture(scope="module")
def hip():
    return Hip()


def run(hip, cases):
    for c in cases:
        G.check_nt(hip, c, record)


# ---- pa_gemm_nt ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tune", G.TUNES)
def test_nt_tile_variants_bf16(hip, tune):
    """every epilogue of every tile variant at the edge shapes of its own tile, exact"""
    run(hip, G.nt_variant_cases(tune, PA_BF16))


def test_nt_f32(hip):
    run(hip, G.nt_variant_cases(0, PA_F32))


@pytest.mark.parametrize("tune", G.ROLE_SPLIT)
def test_nt_flags(hip, tune):
    """PA_GEMM_EPILOGUE_V3 and PA_GEMM_NO_PERSIST against the exact reference, not against each other"""
    run(hip, G.nt_flag_cases(tune))


@pytest.mark.parametrize("tune,dt", [(t, PA_BF16) for t in G.ROWSCALE_TUNES] + [(0, PA_F32)])
def test_rowscale(hip, tune, dt):
    """resid + f * (acc + bias) with f from {0, 1, 2, 0.5}: epilogues v2 and v3, no-persist, in place, exact"""
    run(hip, G.rowscale_cases(tune, dt))


@pytest.mark.parametrize("M,N,steps", G.SPLITK_SHAPES)
def test_splitk(hip, M, N, steps):
    K = G.kelems(PA_BF16, steps)
    for epi in (STORE, RESID):
        assert hip.lib.pa_gemm_nt_splitk_plan(M, N, K, epi, PA_BF16) >= 2, "the shape is meant to be split"
    for c in G.splitk_cases(M, N, steps):
        o = G.check_nt(hip, c, record)
        if c.ws != "ok":            # ws NULL or one float too small: this IS pa_gemm_nt, bit for bit
            k = "out_lp" if c.epi == STORE else "out_f32"
            o2 = G.check_nt(hip, replace(c, entry="nt", ws="ok"))
            assert torch.equal(G.grab(o[k], c.name, N), G.grab(o2[k], c.name, N))


@pytest.mark.parametrize("M,N,steps", G.SPLITK_UNSPLIT)
def test_splitk_entry_at_k_1024_is_the_plain_gemm(hip, M, N, steps):
    """16 K steps: the plan is one slice (see gemm_cases.SPLITK_UNSPLIT) and the entry is pa_gemm_nt"""
    K = G.kelems(PA_BF16, steps)
    assert hip.lib.pa_gemm_nt_splitk_plan(M, N, K, STORE, PA_BF16) == 1 and hip.lib.pa_gemm_nt_splitk_ws_floats(M, N, K, RESID, PA_BF16) == 0
    run(hip, G.splitk_cases(M, N, steps))


def smallest_blocked_m(lib, N, K):
    return next((M for M in range(1, 20000) if lib.pa_gemm_blocked_pre_ok(M, N, K) == 1), None)


@pytest.mark.parametrize("N,K,want", [(3072, 768, 2689), (1024, 768, 8193), (3072, 1088, 1), (1024, 1088, 1)])
def test_mlp_blocked_smallest_shape(hip, N, K, want):
    """the smallest M for which the library has the blocked form: at K <= 1024 the first M whose 128 x 128 tiles need a second
    round (neither a multiple of 32 nor of the 192-row tile that then runs), at K > 1024 a single row"""
    M = smallest_blocked_m(hip.lib, N, K)
    assert M == want
    G.check_mlp_blocked(hip, M, N, K, record)


@pytest.mark.parametrize("M,N,K", [(33, 3072, 1088), (129, 1024, 1088)])
def test_mlp_blocked_edge_rows(hip, M, N, K):
    assert hip.lib.pa_gemm_blocked_pre_ok(M, N, K) == 1
    G.check_mlp_blocked(hip, M, N, K, record)


# ---- pa_gemm_tn ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,tune", G.TN_KERNELS)
@pytest.mark.parametrize("T", G.TN_TOKENS)
def test_tn(hip, dt, tune, T):
    """every partial slab, the fused column sums of dY and both reductions, exact; NaN behind the last token"""
    for c in G.tn_cases(dt, tune, T):
        G.check_tn(hip, c)


def test_tn_batched(hip):
    G.check_tn_batched(hip, G.batch_cases(341, G.TN_BATCH_1))
    G.check_tn_batched(hip, G.batch_cases(97, G.TN_BATCH_4))
    G.check_tn_batched(hip, G.batch_cases(97, G.TN_BATCH_4), problem_major=True)
    G.check_tn_batched(hip, G.batch_cases((341, 97, 48, 1), G.TN_BATCH_MIXED_SPLITS))


@pytest.mark.parametrize("T,n_long,long_steps", G.TN_PLANS)
def test_tn_batched_plan(hip, T, n_long, long_steps):
    probs = [(M, N, n_long + 1, db) for M, N, _, db in G.TN_BATCH_4]
    G.check_tn_batched(hip, G.batch_cases(T, probs, fam_shift=n_long), plan=(n_long, long_steps))
    G.check_tn_batched(hip, G.batch_cases(T, probs[:1]), plan=(n_long, long_steps))


# ---- argument checks -------------------------------------------------------------------------------------------------------
def refused(outs):
    for o in (outs if isinstance(outs, list) else [outs]):
        for k, g in o.items():
            if g is not None:
                G.untouched(g, k)


def test_argument_checks(hip):
    """every PA_EINVAL / PA_EUNSUPPORTED the header documents for these entries, with the outputs left at the sentinel"""
    for name, entry, c, override, want in G.NT_ARG_CASES:
        rc, outs = hip.nt(c, G.nt_inputs(c), override=override)
        assert rc == want, (name, rc, want)
        refused(outs)
    for name, c, override, want in G.TN_ARG_CASES:
        rc, outs = hip.tn(c, G.tn_inputs(c), override=override)
        assert rc == want, (name, rc, want)
        refused(outs)
    cs = G.batch_cases(97, G.TN_BATCH_4)
    ins = [G.tn_inputs(c) for c in cs]
    for name, kw, want in (("different token counts", dict(plan=(1, 1), override={2: dict(K=96)}), G.PA_EUNSUPPORTED),
                           ("an empty short slice", dict(plan=(1, 3)), G.PA_EINVAL),
                           ("n_long = 0", dict(plan=(0, 1)), G.PA_EINVAL),
                           ("long_steps = 0", dict(plan=(1, 0)), G.PA_EINVAL),
                           ("split_k other than n_long + 1", dict(plan=(1, 1), override={1: dict(split_k=3)}), G.PA_EINVAL),
                           ("f32", dict(override={0: dict(dtype=PA_F32)}), G.PA_EUNSUPPORTED),
                           ("M % 8", dict(override={3: dict(M=244)}), G.PA_EUNSUPPORTED)):
        rc, outs = hip.tn_batched(cs, ins, **kw)
        assert rc == want, (name, rc, want)
        refused(outs)
    arr = (_lib.GemmArgs * 5)()
    assert hip.lib.pa_gemm_tn_batched(arr, 5, hip.st) == G.PA_EINVAL and hip.lib.pa_gemm_tn_batched(arr, 0, hip.st) == G.PA_EINVAL
    assert hip.lib.pa_gemm_nt(None, hip.st) == G.PA_EINVAL and hip.lib.pa_gemm_tn(None, hip.st) == G.PA_EINVAL

"""Shapes, operands, references, conditions and checkers of the exact GEMM parity suite (pa_gemm_nt and its split-K / row-factor
forms, pa_gemm_tn and its batched forms, pa_reduce_partials behind them).

Used by tests/test_gpu_gemm_exact.py (the HIP kernels, through the C ABI) and tests/test_gemm_cases_cpu.py (the same checkers run
against `TorchGemm`, plain torch: the f64 product of the operands, the header's epilogue formula in f32, ONE round-to-nearest-even
where the output is bf16 -- every torch.equal and every bound below is one an honest implementation meets).  A checker takes an
`impl` object, hands it a case and its CPU tensors and gets guarded output buffers back (tests/row_kernel_cases.py: guarded_in,
GuardedOut, SENTINEL, GUARD); it neither knows nor cares where the arithmetic ran.

Operand families, all exact (the conditions are asserted by the checkers themselves, on the CPU and on the GPU):

  ternary   entries from {-1, 0, 1} times a power of two `scale` (2^-3 for the GELU cases); bias n mod 17 - 8, residual and
            accumulate-start values small integers, times the same scale.  Every f32 partial sum is an integer far below 2^24 in
            any summation order: f32 outputs are compared with torch.equal against the f64 product.  bf16 outputs need
            max|ref| <= 256 * scale: every reference is then a bf16 number, an error of one unit cannot hide in the rounding.
  full      integers in [-90, 90] (all mantissa bits of bf16 in use), reduction length <= 2048, so K * 8100 <= 2^24 and every f32
            sum is still exact.  f32 outputs: torch.equal.  bf16 outputs: torch.equal against the exact integer rounded ONCE --
            a second rounding or a truncating conversion shows.  This family notices an operand bit lost on the way through LDS.
  tag       ternary with row m of A scaled by 2^(m mod 3) and row n of B by 2^(n mod 3) (the weight gradients: column m of dY
            and column n of X): with the bias n mod 17 - 8 a misattributed row or column lands on a different integer.

The two non-exact epilogues (GELU's activation, GELU' with a non-zero pre-activation) have exact `pre` / `acc`, so what remains is
the documented approximation error and one output rounding: per-element bounds, derived below (ACT_POLY ...), never tuned.

Alignment: the header promises nothing about operands off 16-byte alignment (the LDS-DMA and 16-byte vector loads need it), so
only `rowscale` -- read one float per row -- and the operands of pa_reduce_partials are taken off it.
"""
import functools
import math
from dataclasses import dataclass, replace

import torch

from tests.row_kernel_cases import (EXACT_LIMIT, GUARD, PA_BF16, PA_F32, SENTINEL, TD, GuardedOut, guarded_in, padded,  # noqa: F401
                                    rel_err)

PA_OK, PA_EINVAL, PA_EUNSUPPORTED = 0, -1, -2
STORE, GELU, RESID, DGELU, PARTIAL = range(5)
BLOCKED_PRE, NO_PERSIST, EPILOGUE_V3, COLSUM_DEFER = 0x100, 0x400, 0x1000, 0x2000
EPI_NAME = {STORE: "store", GELU: "gelu", RESID: "resid", DGELU: "dgelu", PARTIAL: "partial"}
F32 = torch.float32

# workgroup tile (rows x columns) of every pa_gemm_args.tune the header lists; 0 is the heuristic, which runs shapes this small on
# variant 1.  The f32 path has one variant (128 x 128) whatever tune says.
TILE = {0: (128, 128), 1: (128, 128), 2: (256, 256), 3: (192, 128), 6: (256, 256), 7: (192, 256), 8: (128, 256), 9: (128, 256),
        13: (192, 128), 17: (192, 256), 18: (128, 256), 19: (128, 256)}
TUNES = tuple(TILE)
ROLE_SPLIT = (6, 7, 8, 17, 18)
ROWSCALE_TUNES = (0, 1, 6, 7, 8, 17, 18)
NO_PARTIAL = (13, 19)                 # epilogue v2 only: PA_EPI_PARTIAL is PA_EINVAL (include/passt_amd.h, pa_gemm_args.tune)
TN_STEP_ROWS = 48                     # PA_TN_STEP_ROWS; the GPU suite asserts pa_gemm_tn_step_rows() agrees
QK_COLSCALE = 64 ** -0.5 * math.log2(math.e)      # the model's q prescale: head_dim^-0.5 * log2(e)

# ---- per-element bounds of the two non-exact epilogues --------------------------------------------------------------------
# |act - gelu64(pre)| <= OUT_ROUND |ref| + ACT_POLY |pre|,   |d_pre - acc gelu'64(aux)| <= OUT_ROUND |ref| + DACT_POLY |acc|.
# The bounds as specified are  2^-9 |ref| + 1.3e-5 |pre|  and  2^-9 |ref| + 1.5e-4 |acc|  in bf16 (2^-24 and 1.5e-7 in f32) -- one
# output rounding plus the documented polynomial error (pa_common.h / tools/gelu_fit.py: |Phi err| <= 1.3e-5, |gelu' err| <= 1.5e-4
# for the bf16 epilogues; Abramowitz-Stegun 7.1.26, |err| <= 1.5e-7, for the f32 ones) -- and EACH BOUND GETS A FACTOR 2 for the
# f32 evaluation order: the figures are those of exact arithmetic on the exact argument, while the kernel's Horner chain, x * Phi(x)
# and the product with acc round a few more times before the one rounding of the output.  In bf16 the factor covers both terms:
# 2 * 2^-9 = 2^-8 |ref| is also exactly the unit roundoff of bf16's 8 significant bits (half an ulp at the binade's lower end), which
# a single correct rounding reaches -- TorchGemm uses up to 83 % of the doubled bound, i.e. 1.65 x the undoubled one.  In f32 only
# the polynomial term is doubled (2^-24 is the unit roundoff already): stricter than specified, and met.
OUT_ROUND = {PA_BF16: 2 * 2.0 ** -9, PA_F32: 2.0 ** -24}
ACT_POLY = {PA_BF16: 2 * 1.3e-5, PA_F32: 2 * 1.5e-7}
DACT_POLY = {PA_BF16: 2 * 1.5e-4, PA_F32: 2 * 1.5e-7}
# the rel_err bounds of the random-operand tests (tests/test_gpu_kernels.py): what the mutation tests show to be blind
OLD_BOUND_LP, OLD_BOUND_F32_OF_BF16 = 1.2e-2, 3e-3


def kelems(dt, steps):
    """K of `steps` 128-byte steps"""
    return steps * (64 if dt == PA_BF16 else 32)


def cdiv(a, b):
    return -(-a // b)


# ---- cases ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class NT:
    """one pa_gemm_nt* call.  entry: nt | rowscale | splitk | splitk_rowscale.  pad: extra elements in every leading dimension
    (operands: NaN, outputs: the sentinel).  colsum: "" | set | acc | defer.  aux: zero | eighths.  ws: ok | null | small."""
    dt: int
    epi: int
    M: int
    N: int
    K: int
    fam: str = "ternary"
    scale: float = 1.0
    tune: int = 0
    flags: int = 0
    bias: bool = True
    entry: str = "nt"
    split_k: int = 1
    colscale_n: int = 0
    colscale: float = 1.0
    row_mod: int = 0
    inplace: bool = False
    pad: int = 0
    factors: bool = False
    ws: str = "ok"
    colsum: str = ""
    aux: str = "zero"
    seed: int = 0
    small_bias: bool = False          # bias from {-1, 0, 1} (mutation demonstrations)
    resid_mul: int = 1                # residual = small integers x this (mutation demonstrations)

    @property
    def name(self):
        bits = [EPI_NAME[self.epi], f"dt{self.dt}", f"t{self.tune}", f"{self.M}x{self.N}x{self.K}", self.fam]
        for k, d in (("flags", 0), ("entry", "nt"), ("split_k", 1), ("colscale_n", 0), ("row_mod", 0), ("pad", 0), ("ws", "ok"),
                     ("colsum", ""), ("aux", "zero")):
            if getattr(self, k) != d:
                bits.append(f"{k}={getattr(self, k)}")
        for k in ("inplace", "factors"):
            if getattr(self, k):
                bits.append(k)
        if not self.bias:
            bits.append("nobias")
        return ",".join(bits)

    @property
    def tile(self):
        return TILE[self.tune] if self.dt == PA_BF16 else (128, 128)

    @property
    def out_rows(self):
        return (self.M // self.row_mod) * (self.row_mod + REMAP_OFF) if self.row_mod else self.M


REMAP_OFF = 2                         # out_row_off; out_batch_rows = row_mod + REMAP_OFF


@dataclass(frozen=True)
class TN:
    """one weight-gradient problem: dY [T][M], X [T][N] -> out[split_k][M][N] (+ colsum_ws[split_k][M])"""
    dt: int
    T: int
    M: int
    N: int
    tune: int = 0
    split_k: int = 1
    fam: str = "ternary"
    colsum: bool = False
    pad: int = 0
    seed: int = 0

    @property
    def name(self):
        return f"tn,dt{self.dt},t{self.tune},{self.T}x{self.M}x{self.N},s{self.split_k},{self.fam}" + (",db" if self.colsum else "") + \
            (f",pad{self.pad}" if self.pad else "")

    @property
    def step(self):
        """tokens per pipeline step: PA_TN_STEP_ROWS for the bf16 role-split kernel, 64 (bf16, tune 1) / 32 (f32) for the generic"""
        return 32 if self.dt == PA_F32 else (64 if self.tune == 1 else TN_STEP_ROWS)


def nt_slices(c):
    """K ranges of the PA_EPI_PARTIAL slabs: ceil(steps / split_k) steps each, the last ones shorter or EMPTY (a slab of zeros);
    a step is 128 bytes of K, 64 bytes for tune 9 (include/passt_amd.h)"""
    es = 2 if c.dt == PA_BF16 else 4
    step = (64 if (c.dt == PA_BF16 and c.tune in (9, 19)) else 128) // es
    steps = c.K // step
    per = cdiv(steps, c.split_k)
    return [(min(z * per, steps) * step, min((z + 1) * per, steps) * step) for z in range(c.split_k)]


def tn_slices(c):
    steps = cdiv(c.T, c.step)
    per = cdiv(steps, c.split_k)
    return [(min(z * per * c.step, c.T), min((z + 1) * per * c.step, c.T)) for z in range(c.split_k)]


def plan_slices(T, n_long, long_steps, step=TN_STEP_ROWS):
    """pa_gemm_tn_batched_plan: n_long slices of long_steps steps and one short slice of what is left"""
    cuts = [min(z * long_steps * step, T) for z in range(n_long + 1)] + [T]
    return list(zip(cuts[:-1], cuts[1:]))


def ragged_split(T, step):
    """a split_k >= 2 that leaves the last slice a single ragged step, or None"""
    steps = cdiv(T, step)
    if T % step == 0:
        return None
    for s in range(2, steps + 1):
        per = cdiv(steps, s)
        if steps - (s - 1) * per == 1:
            return s
    return None


# ---- shape lists ---------------------------------------------------------------------------------------------------------
def nt_shapes(tune, dt):
    """six (M, N, K) that hold every value of M in {1, TM-1, TM, TM+1, 2 TM+33}, N in {8, TN-8, TN, TN+8} and K steps in
    {1, 2, 3, 7, 17}; the last is the all-edges corner"""
    tm, tn = TILE[tune] if dt == PA_BF16 else (128, 128)
    Ms, Ns, Ks = (1, tm - 1, tm, tm + 1, 2 * tm + 33), (8, tn - 8, tn, tn + 8), (1, 2, 3, 7, 17)
    s = [(Ms[j], Ns[(j + 1) % 4], kelems(dt, Ks[(j + 2) % 5])) for j in range(5)]
    return s + [(Ms[4], Ns[3], kelems(dt, 17))]




def nt_variant_cases(tune, dt):
    """every epilogue of one tile variant at all six shapes, then the q-prescale columns at the corner and the row remap"""
    out = []
    shapes = nt_shapes(tune, dt)
    for j, (M, N, K) in enumerate(shapes):
        base = dict(dt=dt, M=M, N=N, K=K, tune=tune, seed=j)
        out.append(NT(epi=STORE, fam=("ternary", "full", "tag")[j % 3] if K <= kelems(dt, 3) else ("ternary", "full")[j % 2], bias=j % 2 == 0,
                      **base))
        out.append(NT(epi=STORE, fam="full", bias=True, **base))
        out.append(NT(epi=GELU, scale=0.125, **base))
        out.append(NT(epi=RESID, fam="tag" if K <= kelems(dt, 7) else "full", **base))
        out.append(NT(epi=RESID, inplace=True, pad=8 if j == 5 else 0, **base))
        out.append(NT(epi=DGELU, colsum=("set", "acc", "defer")[j % 3], **base))
        out.append(NT(epi=DGELU, aux="eighths", colsum="set" if j == 5 else "", **base))
        if dt == PA_BF16 and tune in NO_PARTIAL:
            continue
        for s in (1, 2, 3):
            out.append(NT(epi=PARTIAL, split_k=s, fam=("tag", "full", "ternary")[s - 1], bias=False, pad=8 if (s == 2 and j == 5) else 0, **base))
    M, N, K = shapes[5]
    base = dict(dt=dt, epi=STORE, M=M, N=N, K=K, tune=tune)
    out.append(NT(colscale_n=64, colscale=0.5, pad=8, **base))
    if N >= 128:
        out.append(NT(colscale_n=N // 64 * 64, colscale=2.0, fam="full", **base))
    out.append(NT(colscale_n=N // 64 * 64, colscale=QK_COLSCALE, **base))
    out.append(NT(dt=dt, epi=RESID, M=3 * 37, N=N, K=kelems(dt, 2), tune=tune, row_mod=37, fam="tag"))
    return out


def nt_flag_cases(tune):
    """PA_GEMM_EPILOGUE_V3 and PA_GEMM_NO_PERSIST on a role-split variant, against the exact reference"""
    out = []
    shapes = nt_shapes(tune, PA_BF16)
    for flags in (EPILOGUE_V3, NO_PERSIST, EPILOGUE_V3 | NO_PERSIST):
        for j in (3, 5):
            M, N, K = shapes[j]
            base = dict(dt=PA_BF16, M=M, N=N, K=K, tune=tune, flags=flags, seed=j)
            out += [NT(epi=STORE, fam="full", **base), NT(epi=GELU, scale=0.125, **base), NT(epi=RESID, fam="full", **base),
                    NT(epi=DGELU, **base), NT(epi=DGELU, aux="eighths", **base), NT(epi=STORE, colscale_n=64, colscale=2.0, **base)]
    return out


def rowscale_cases(tune, dt):
    tm, tn = TILE[tune] if dt == PA_BF16 else (128, 128)
    out = []
    for M in (1, 33, 257, 2 * tm + 33):
        for flags in ((0, EPILOGUE_V3, NO_PERSIST) if (dt == PA_BF16 and tune in ROLE_SPLIT) else (0,)):
            for inplace in (False, True):
                out.append(NT(dt=dt, epi=RESID, M=M, N=tn + 8, K=kelems(dt, 3), tune=tune, flags=flags, inplace=inplace, factors=True,
                              entry="rowscale", fam="tag" if inplace else "full", seed=M))
    return out


# (M, N, K steps) of the split-K entry.  16 steps is K = 1024, where the heuristic keeps the generic kernel and the plan is ONE
# slice for every M (pick_nt_variant: the role-split kernels only win above K = 1024 or when the 128 x 128 tiles need a second
# round, and then there are more than 128 tiles): those cases assert the plan is 1 and that the entry IS pa_gemm_nt.
SPLITK_SHAPES = ((1, 264, 17), (24, 768, 17), (129, 264, 48), (129, 768, 17), (24, 264, 48))
SPLITK_UNSPLIT = ((24, 264, 16), (129, 768, 16))


def splitk_cases(M, N, steps):
    base = dict(dt=PA_BF16, M=M, N=N, K=kelems(PA_BF16, steps), entry="splitk")
    return [NT(epi=STORE, colscale_n=64, colscale=0.5, **base), NT(epi=STORE, fam="full" if steps <= 32 else "ternary", bias=False, **base),
            NT(epi=RESID, fam="tag" if steps <= 17 else "ternary", **base), NT(epi=RESID, inplace=True, **base),
            NT(epi=RESID, pad=8, **base), NT(epi=STORE, pad=8, **base),
            NT(epi=RESID, ws="null", **base), NT(epi=STORE, ws="small", **base),
            NT(epi=RESID, factors=True, entry="splitk_rowscale", **{k: v for k, v in base.items() if k != "entry"}),
            NT(epi=RESID, factors=True, inplace=True, entry="splitk_rowscale", **{k: v for k, v in base.items() if k != "entry"})]


TN_TOKENS = (1, 15, 16, 17, 47, 48, 49, 96, 97, 341)
TN_SHAPES = ((8, 8), (248, 264), (256, 256), (264, 776))
TN_KERNELS = ((PA_BF16, 0), (PA_BF16, 1), (PA_F32, 0))


def tn_cases(dt, tune, T):
    out = []
    step = TN(dt, T, 8, 8, tune).step
    splits = [1, 2] + ([ragged_split(T, step)] if ragged_split(T, step) not in (None, 2) else [])
    for j, (M, N) in enumerate(TN_SHAPES):
        for s in splits:
            fam = ("ternary", "full", "tag")[(j + s) % 3]
            out.append(TN(dt, T, M, N, tune, s, fam, colsum=(dt == PA_BF16 and tune != 1), pad=8 if (j == 1 and s == 2) else 0, seed=j))
    return out


# batched entries: (token count, problems' (M, N, split_k, db)) -- 1 and 4 problems, different widths, db on some
TN_BATCH_1 = ((264, 776, 3, True),)
TN_BATCH_4 = ((256, 256, 2, False), (776, 264, 2, True), (8, 8, 2, True), (248, 264, 2, False))
TN_BATCH_MIXED_SPLITS = ((256, 256, 1, True), (776, 264, 3, False), (8, 8, 2, True), (248, 264, 4, False))
TN_PLANS = ((96, 1, 1), (341, 2, 3), (341, 1, 5))          # (tokens, n_long, long_steps)


# ---- operands ------------------------------------------------------------------------------------------------------------
def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pow2_tags(n):
    return 2.0 ** (torch.arange(n) % 3).float()


def row_factors(M):
    """factors from {0, 1, 2, 0.5} that change every 5 rows (inside every 32-row pass) and at EVERY multiple of 32 (every wave-tile
    boundary, the first row of the last partial tile)"""
    m = torch.arange(M)
    return torch.tensor([0.0, 1.0, 2.0, 0.5])[(m // 5 + m // 32) % 4]


@functools.lru_cache(maxsize=8)
def _operands(fam, M, N, K, scale, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    if fam == "full":
        A, B = _ints(g, -90, 90, M, K), _ints(g, -90, 90, N, K)
    else:
        A, B = _ints(g, -1, 1, M, K), _ints(g, -1, 1, N, K)
        if fam == "tag":
            A, B = A * _pow2_tags(M)[:, None], B * _pow2_tags(N)[:, None]
    A = A * scale
    return A, B, A.double() @ B.double().t()


def nt_inputs(c):
    """CPU tensors of a case: A [M][K], B [N][K] (dtype), the exact product P (f64) and what the epilogue takes"""
    A, B, P = _operands(c.fam, c.M, c.N, c.K, c.scale, c.seed)
    g = torch.Generator().manual_seed(2000 + c.seed)
    i = dict(A=A.to(TD[c.dt]), B=B.to(TD[c.dt]), P=P, bias=None, resid=None, aux=None, rowscale=None, start=None)
    assert torch.equal(i["A"].float(), A) and torch.equal(i["B"].float(), B), "operands must be exact in the dtype"
    if c.bias and c.epi in (STORE, GELU, RESID):
        b = _ints(g, -1, 1, c.N) if c.small_bias else ((torch.arange(c.N) % 17).float() - 8)
        i["bias"] = b * c.scale
    if c.epi == RESID:
        i["resid"] = _ints(g, -8, 8, c.row_mod or c.M, c.N) * (c.scale * c.resid_mul)
    if c.epi == DGELU:
        i["aux"] = (torch.zeros(c.M, c.N) if c.aux == "zero" else _ints(g, -48, 48, c.M, c.N) / 8).to(TD[c.dt])
        if c.colsum:
            i["start"] = _ints(g, -50, 50, c.N) * c.scale
    if c.factors:
        i["rowscale"] = row_factors(c.M)
    return i


@functools.lru_cache(maxsize=8)
def tn_inputs(c):
    g = torch.Generator().manual_seed(3000 + c.seed + c.T)
    lo, hi = (-90, 90) if c.fam == "full" else (-1, 1)
    dY, X = _ints(g, lo, hi, c.T, c.M), _ints(g, lo, hi, c.T, c.N)
    if c.fam == "tag":
        dY, X = dY * _pow2_tags(c.M), X * _pow2_tags(c.N)
    start = _ints(g, -50, 50, c.M, c.N)
    return dict(dY=dY.to(TD[c.dt]), X=X.to(TD[c.dt]), start=start, start_db=_ints(g, -50, 50, c.M))


# ---- f64 references ------------------------------------------------------------------------------------------------------
def gelu64(x):
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2)))


def dgelu64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)


def f32_exact(t):
    """`t` (f64) is a tensor of f32 numbers"""
    return torch.equal(t.float().double(), t)


def lp_exact(t, dt):
    return torch.equal(t.to(F32).to(TD[dt]).double(), t)


def nt_conditions(c, i):
    """the conditions of the operand families, per case (never clipped)"""
    P = i["P"]
    if c.fam == "full":
        assert c.K <= 2048 and c.K * 8100 <= EXACT_LIMIT and float(i["A"].abs().max()) <= 90 and float(i["B"].abs().max()) <= 90
    # every partial sum in any order: sum_k |a b| (+ |bias| + |resid|) stays below 2^24 units of `scale`
    mag = i["A"].double().abs() @ i["B"].double().abs().t()
    extra = sum(float(i[k].abs().max()) for k in ("bias", "resid", "start") if i[k] is not None)
    assert (float(mag.max()) * (2 if c.factors else 1) + extra) / c.scale < EXACT_LIMIT / 2       # (/ 2: the halves of acc / 2, f = 0.5)
    assert f32_exact(P) and torch.equal(P / c.scale, (P / c.scale).round()), "the f64 product is an exact integer"
    lp_out = c.epi in (STORE, GELU) or (c.epi == DGELU and c.aux == "zero" and c.dt == PA_BF16)
    if lp_out and c.dt == PA_BF16 and c.fam != "full":
        ref = P + (i["bias"].double() if i["bias"] is not None else 0.0)
        assert float(ref.abs().max()) <= 256 * c.scale, (c.name, float(ref.abs().max()))
        assert lp_exact(ref, c.dt)


# ---- buffers -------------------------------------------------------------------------------------------------------------
def new_out(rows, N, pad, dtype, device, init=None):
    """a guarded [rows][N + pad] output whose gap columns hold the sentinel; init: [rows][N] start values"""
    full = None
    if init is not None:
        full = torch.full((rows, N + pad), SENTINEL, dtype=dtype)
        full[:, :N] = init
    return GuardedOut((rows, N + pad), dtype, device, init=full)


def grab(g, what, N, row_mask=None):
    """the [rows][N] result on the CPU after the checks of the buffer: both guards and the gap columns untouched, no promised
    element still the sentinel, every row outside row_mask (the row remap) untouched"""
    buf = g.buf.cpu()
    assert bool((buf[:g.lo] == SENTINEL).all()), f"{what}: a write in front of the output"
    assert bool((buf[g.lo + g.n:] == SENTINEL).all()), f"{what}: a write behind the output"
    full = buf[g.lo:g.lo + g.n].view(g.view.shape)
    dense = full[:, :N]
    assert bool((full[:, N:] == SENTINEL).all()), f"{what}: a write into the gap columns"
    if row_mask is not None:
        assert bool((dense[~row_mask] == SENTINEL).all()), f"{what}: a write into a row the remap does not name"
        dense = dense[row_mask]
    assert not bool((dense == SENTINEL).any()), f"{what}: elements the kernel never wrote"
    return dense.clone()


def untouched(g, what):
    buf = g.buf.cpu()
    assert bool((buf == SENTINEL).all()), f"{what}: a refused call wrote"


def remap_rows(c):
    """output row of every product row, and the mask of rows the remap names"""
    m = torch.arange(c.M)
    orow = (m // c.row_mod) * (c.row_mod + REMAP_OFF) + REMAP_OFF + m % c.row_mod
    mask = torch.zeros(c.out_rows, dtype=torch.bool)
    mask[orow] = True
    return orow, mask


# ---- the plain torch implementation --------------------------------------------------------------------------------------
class TorchGemm:
    """pa_gemm_nt* / pa_gemm_tn* / pa_reduce_partials in plain torch on the CPU with the kernels' calling conventions: the f64
    product of the operands, the header's epilogue formula in f32, one round-to-nearest-even where the output is bf16 (GELU: torch's
    erf form in f32).  The small methods are the places a tile kernel goes wrong; the mutation tests override them one at a time."""
    name = "torch"
    dev = "cpu"

    # -- hooks
    def product(self, A, B, c, z=None):
        """f32 of the exact product of a K slice (z: slab index, None = the whole K)"""
        return (A.double() @ B.double().t()).float()

    def bias_of(self, c, bias):
        return bias[None, :].expand(c.M, c.N)

    def factors_of(self, c, f):
        return f

    def round_out(self, v, dtype):
        return v.to(dtype)

    def write(self, g, v, rows=None, N=None):
        N = v.shape[1] if N is None else N
        if rows is None:
            g.view[:, :N] = v
        else:
            g.view[rows, :N] = v

    def tn_product(self, dY, X, c, t0, t1, last):
        return (dY[t0:t1].double().t() @ X[t0:t1].double()).float()

    # -- entries
    def nt(self, c, i):
        td, A, B = TD[c.dt], i["A"], i["B"]
        outs = {}
        if c.epi == PARTIAL:
            g = new_out(c.split_k * c.M, c.N, c.pad, F32, self.dev)
            for z, (k0, k1) in enumerate(nt_slices(c)):
                self.write(g, self.product(A[:, k0:k1], B[:, k0:k1], c, z), rows=slice(z * c.M, (z + 1) * c.M))
            return PA_OK, dict(out_f32=g)
        v = self.product(A, B, c)
        if i["bias"] is not None:
            v = v + self.bias_of(c, i["bias"])
        if c.epi == STORE:
            if c.colscale_n:
                v = torch.cat([v[:, :c.colscale_n] * torch.tensor(c.colscale, dtype=F32), v[:, c.colscale_n:]], 1)
            outs["out_lp"] = new_out(c.M, c.N, c.pad, td, self.dev)
            self.write(outs["out_lp"], self.round_out(v, td))
        elif c.epi == GELU:
            outs["out_lp"], outs["out_lp2"] = new_out(c.M, c.N, c.pad, td, self.dev), new_out(c.M, c.N, c.pad, td, self.dev)
            self.write(outs["out_lp"], self.round_out(v, td))
            self.write(outs["out_lp2"], self.round_out(torch.nn.functional.gelu(v), td))
        elif c.epi == RESID:
            if c.row_mod:
                orow, _ = remap_rows(c)
                g = new_out(c.out_rows, c.N, c.pad, F32, self.dev)
                self.write(g, v + i["resid"][torch.arange(c.M) % c.row_mod], rows=orow)
            else:
                g = new_out(c.M, c.N, c.pad, F32, self.dev, init=i["resid"] if c.inplace else None)
                if c.factors:
                    v = self.factors_of(c, i["rowscale"])[:, None] * v
                self.write(g, i["resid"] + v)
            outs["out_f32"] = g
        else:
            x = i["aux"].float()
            d = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)
            v = v * d
            outs["out_lp"] = new_out(c.M, c.N, c.pad, td, self.dev)
            self.write(outs["out_lp"], self.round_out(v, td))
            if c.colsum:
                s = v.sum(0)
                outs["colsum"] = GuardedOut(c.N, F32, self.dev)
                outs["colsum"].view.copy_(i["start"] + s if c.colsum == "acc" else s)
        return PA_OK, outs

    def mlp_blocked(self, c, i, i2):
        """fc1 + GELU with the blocked pre-activation, then GELU' of the second product reading it back: act, d_pre, column sums"""
        pre = (self.product(i["A"], i["B"], c) + i["bias"]).to(TD[c.dt])
        act, dpre, cs = new_out(c.M, c.N, 0, TD[c.dt], self.dev), new_out(c.M, c.N, 0, TD[c.dt], self.dev), GuardedOut(c.N, F32, self.dev)
        self.write(act, torch.nn.functional.gelu(pre.float()).to(TD[c.dt]))
        x = pre.float()
        v = self.product(i2["A"], i2["B"], c) * (0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi))
        self.write(dpre, v.to(TD[c.dt]))
        cs.view.copy_(v.sum(0))
        return PA_OK, dict(act=act, d_pre=dpre, colsum=cs)

    def tn(self, c, i, slices=None):
        slices = slices or tn_slices(c)
        S = len(slices)
        g = new_out(S * c.M, c.N, c.pad, F32, self.dev)
        cs = GuardedOut((S, c.M), F32, self.dev) if c.colsum else None
        for z, (t0, t1) in enumerate(slices):
            self.write(g, self.tn_product(i["dY"], i["X"], c, t0, t1, z == S - 1), rows=slice(z * c.M, (z + 1) * c.M))
            if cs is not None:
                cs.view[z] = i["dY"][t0:t1].float().sum(0)
        return PA_OK, dict(out_f32=g, colsum_ws=cs)

    def tn_batched(self, cs, ins, plan=None, problem_major=False):
        sl = [plan_slices(c.T, plan[0], plan[1]) if plan else None for c in cs]
        return PA_OK, [self.tn(c, i, s)[1] for c, i, s in zip(cs, ins, sl)]

    def reduce(self, partial, accumulate, start, offset=0):
        g = GuardedOut(partial.shape[1], F32, self.dev, init=start if accumulate else None, offset=offset)
        s = partial.sum(0)
        g.view.copy_(start + s if accumulate else s)
        return g


# ---- checkers ------------------------------------------------------------------------------------------------------------
def _rec(rec, group, ratio):
    if rec is not None:
        rec(group, ratio)


def within(got, ref, bound, what):
    """|got - ref| <= bound per element; returns the worst got / bound (over the elements whose bound is not 0)"""
    err = (got.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bad = err > bound
    assert not bool(bad.any()), (what, "elements over the bound:", int(bad.sum()), "worst error / bound:",
                                 float((err / bound.clamp_min(1e-300))[bad].max()))
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


def equal(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ, first at {idx}: "
                             f"got {float(got[tuple(idx)])}, want {float(want[tuple(idx)])}")


def nt_reference(c, i):
    """f64 results of the header's formulas on the exact product"""
    P = i["P"]
    v = P + (i["bias"].double() if i["bias"] is not None else 0.0)
    if c.epi == STORE:
        if c.colscale_n:
            v = torch.cat([v[:, :c.colscale_n] * float(torch.tensor(c.colscale, dtype=F32)), v[:, c.colscale_n:]], 1)
        return dict(out_lp=v)
    if c.epi == GELU:
        return dict(out_lp=v, out_lp2=gelu64(v))
    if c.epi == RESID:
        if c.row_mod:
            return dict(out_f32=v + i["resid"].double()[torch.arange(c.M) % c.row_mod])
        if c.factors:
            v = i["rowscale"].double()[:, None] * v
        return dict(out_f32=i["resid"].double() + v)
    if c.epi == DGELU:
        return dict(out_lp=P * dgelu64(i["aux"].double()), acc=P)
    return dict(slabs=[i["A"][:, k0:k1].double() @ i["B"][:, k0:k1].double().t() for k0, k1 in nt_slices(c)])


def check_nt(impl, c, rec=None):
    """one positive case: PA_OK, every buffer check of grab(), the exact comparison (or the derived bound) of its epilogue"""
    i = nt_inputs(c)
    nt_conditions(c, i)
    r = nt_reference(c, i)
    rc, o = impl.nt(c, i)
    assert rc == PA_OK, f"{c.name}: code {rc} for a case of the positive list"
    td, N = TD[c.dt], c.N
    pow2 = c.colscale_n == 0 or math.log2(c.colscale).is_integer()
    if c.epi == STORE:
        got = grab(o["out_lp"], c.name, N)
        if pow2:
            assert f32_exact(r["out_lp"])
            equal(got, r["out_lp"].float().to(td), c.name)
        else:
            # (acc + bias) * colscale: f32 roundings of bias * colscale and of the multiply-add (2^-24 each, of at most |acc cs| +
            # |bias cs|), then ONE rounding of the output
            ref = r["out_lp"]
            cs = float(torch.tensor(c.colscale, dtype=F32))
            mag = (i["P"].abs() + (i["bias"].double().abs() if i["bias"] is not None else 0.0)) * cs
            mag = torch.cat([mag[:, :c.colscale_n], torch.zeros_like(mag[:, c.colscale_n:])], 1)
            bound = (OUT_ROUND[c.dt] if c.dt == PA_BF16 else 0.0) * (ref.abs() + 2.0 ** -22 * mag) + 2.0 ** -22 * mag
            _rec(rec, f"colscale[dt{c.dt}]", within(got, ref, bound, c.name))
    elif c.epi == GELU:
        pre, act = grab(o["out_lp"], c.name + " pre", N), grab(o["out_lp2"], c.name + " act", N)
        equal(pre, r["out_lp"].float().to(td), c.name + " pre")
        bound = OUT_ROUND[c.dt] * r["out_lp2"].abs() + ACT_POLY[c.dt] * r["out_lp"].abs()
        _rec(rec, f"act[dt{c.dt}]", within(act, r["out_lp2"], bound, c.name + " act"))
    elif c.epi == RESID:
        mask = remap_rows(c)[1] if c.row_mod else None
        got = grab(o["out_f32"], c.name, N, row_mask=mask)
        assert f32_exact(r["out_f32"])
        equal(got, r["out_f32"].float(), c.name)
    elif c.epi == DGELU:
        got = grab(o["out_lp"], c.name, N)
        elem = OUT_ROUND[c.dt] * r["out_lp"].abs() + DACT_POLY[c.dt] * r["acc"].abs()
        exact = c.aux == "zero" and c.dt == PA_BF16       # gelu_grad_fast1(0) = fmaf(0, q, 0.5) = 0.5: d_pre = acc / 2
        if exact:
            equal(got, (r["acc"] / 2).float().to(td), c.name)
        else:
            _rec(rec, f"d_pre[dt{c.dt}]", within(got, r["out_lp"], elem, c.name))
        if c.colsum:
            cs = o["colsum"].take(c.name + " colsum")
            start = i["start"].double() if c.colsum == "acc" else 0.0
            if exact:
                equal(cs, (start + (r["acc"] / 2).sum(0)).float(), c.name + " colsum")
            else:
                # the sum of the column's per-element bounds (without their output rounding: the sum is of the f32 values), plus
                # the roundings of M f32 additions of terms of at most max|term|
                col = DACT_POLY[c.dt] * r["acc"].abs().sum(0) + 2.0 ** -24 * c.M * r["out_lp"].abs().sum(0)
                _rec(rec, f"d_pre_colsum[dt{c.dt}]", within(cs, start + r["out_lp"].sum(0), col, c.name + " colsum"))
    else:
        got = grab(o["out_f32"], c.name, N)
        for z, ref in enumerate(r["slabs"]):
            equal(got[z * c.M:(z + 1) * c.M], ref.float(), f"{c.name} slab {z}")
        equal(got.view(c.split_k, c.M, N).sum(0), i["P"].float(), c.name + " sum of the slabs")
    return o


def blocked_inputs(M, N, K):
    c = NT(dt=PA_BF16, epi=GELU, M=M, N=N, K=K, scale=0.125, flags=BLOCKED_PRE, seed=7)
    c2 = replace(c, epi=DGELU, scale=1.0, seed=8)
    return c, nt_inputs(c), c2, nt_inputs(c2)


def check_mlp_blocked(impl, M, N, K, rec=None):
    """GELU -> GELU' through the opaque blocked buffer: act and d_pre per element, the fused column sums within the sum of the
    per-element bounds (aux = 0 is impossible here: the pre-activation is the first GEMM's)"""
    c, i, c2, i2 = blocked_inputs(M, N, K)
    nt_conditions(c, i)
    nt_conditions(replace(c2, aux="eighths"), i2)
    pre = i["P"] + i["bias"].double()
    rc, o = impl.mlp_blocked(c, i, i2)
    assert rc == PA_OK, f"blocked {M}x{N}x{K}: code {rc}"
    act, dpre, cs = grab(o["act"], "act", N), grab(o["d_pre"], "d_pre", N), o["colsum"].take("colsum")
    ref_act, ref_d = gelu64(pre), i2["P"] * dgelu64(pre)
    _rec(rec, "blocked_act", within(act, ref_act, OUT_ROUND[PA_BF16] * ref_act.abs() + ACT_POLY[PA_BF16] * pre.abs(), "blocked act"))
    _rec(rec, "blocked_d_pre", within(dpre, ref_d, OUT_ROUND[PA_BF16] * ref_d.abs() + DACT_POLY[PA_BF16] * i2["P"].abs(), "blocked d_pre"))
    col = DACT_POLY[PA_BF16] * i2["P"].abs().sum(0) + 2.0 ** -24 * M * ref_d.abs().sum(0)
    _rec(rec, "blocked_colsum", within(cs, ref_d.sum(0), col, "blocked colsum"))


def tn_conditions(c, i):
    if c.fam == "full":
        assert c.T <= 2048 and c.T * 8100 <= EXACT_LIMIT
    mag = i["dY"].double().abs().t() @ i["X"].double().abs()
    assert float(mag.max()) + 50 < EXACT_LIMIT and float(i["dY"].double().abs().sum(0).max()) + 50 < EXACT_LIMIT


def check_tn_outputs(impl, c, i, o, slices, what):
    """every partial slab on its own, the fused column sums of dY, then pa_reduce_partials of both with accumulate off and on"""
    dY, X, S = i["dY"].double(), i["X"].double(), len(slices)
    got = grab(o["out_f32"], what, c.N)
    for z, (t0, t1) in enumerate(slices):
        equal(got[z * c.M:(z + 1) * c.M], (dY[t0:t1].t() @ X[t0:t1]).float(), f"{what} slab {z}")
    full = (dY.t() @ X).float()
    for acc in (0, 1):
        red = impl.reduce(got.reshape(S, c.M * c.N), acc, i["start"].reshape(-1), offset=acc).take(what + " reduced")
        equal(red.view(c.M, c.N), full + (i["start"] if acc else 0), f"{what} reduced, accumulate {acc}")
    if c.colsum:
        cs = o["colsum_ws"].take(what + " colsum_ws")
        for z, (t0, t1) in enumerate(slices):
            equal(cs[z], dY[t0:t1].sum(0).float(), f"{what} colsum slab {z}")
        for acc in (0, 1):
            red = impl.reduce(cs, acc, i["start_db"], offset=1 - acc).take(what + " db")
            equal(red, dY.sum(0).float() + (i["start_db"] if acc else 0), f"{what} db, accumulate {acc}")
    else:
        assert o["colsum_ws"] is None


def check_tn(impl, c):
    i = tn_inputs(c)
    tn_conditions(c, i)
    rc, o = impl.tn(c, i)
    assert rc == PA_OK, f"{c.name}: code {rc} for a case of the positive list"
    check_tn_outputs(impl, c, i, o, tn_slices(c), c.name)


def batch_cases(T, probs, fam_shift=0):
    return [TN(PA_BF16, T if isinstance(T, int) else T[j], M, N, 0, s, ("tag", "full", "ternary")[(j + fam_shift) % 3], colsum=db, seed=10 + j)
            for j, (M, N, s, db) in enumerate(probs)]


def check_tn_batched(impl, cs, plan=None, problem_major=False):
    ins = [tn_inputs(c) for c in cs]
    for c, i in zip(cs, ins):
        tn_conditions(c, i)
    rc, outs = impl.tn_batched(cs, ins, plan=plan, problem_major=problem_major)
    assert rc == PA_OK, f"batched {[c.name for c in cs]} plan {plan}: code {rc}"
    for c, i, o in zip(cs, ins, outs):
        check_tn_outputs(impl, c, i, o, plan_slices(c.T, plan[0], plan[1]) if plan else tn_slices(c), f"{c.name} plan {plan}")


# ---- argument checks -----------------------------------------------------------------------------------------------------
# (name, entry, base case, fields of pa_gemm_args to override (None = a NULL pointer), expected code); every base case is so small
# that even a call wrongly let through would stay inside the guards
_S = NT(dt=PA_BF16, epi=STORE, M=16, N=64, K=64)
_R = replace(_S, epi=RESID)
_G = replace(_S, epi=GELU, scale=0.125)
_D = replace(_S, epi=DGELU, colsum="set")
_P = replace(_S, epi=PARTIAL, bias=False, split_k=2, K=128)
NT_ARG_CASES = (
    ("K bytes not a multiple of 128", "nt", _S, dict(K=56), PA_EUNSUPPORTED),
    ("K bytes not a multiple of 128, f32", "nt", replace(_S, dt=PA_F32), dict(K=48), PA_EUNSUPPORTED),
    ("N % 8", "nt", _S, dict(N=60), PA_EUNSUPPORTED),
    ("lda off 16 bytes", "nt", _S, dict(lda=68), PA_EUNSUPPORTED),
    ("ldb off 16 bytes", "nt", _S, dict(ldb=68), PA_EUNSUPPORTED),
    ("ldolp % 8", "nt", _S, dict(ldolp=68), PA_EUNSUPPORTED),
    ("ldolp2 % 8", "nt", _G, dict(ldolp2=68), PA_EUNSUPPORTED),
    ("ldo32 % 4", "nt", _R, dict(ldo32=66), PA_EUNSUPPORTED),
    ("ldr % 4", "nt", _R, dict(ldr=66), PA_EUNSUPPORTED),
    ("ldaux % 8", "nt", _D, dict(ldaux=68), PA_EUNSUPPORTED),
    ("split_k > 1 outside PARTIAL", "nt", _S, dict(split_k=2), PA_EINVAL),
    ("colscale_n not a multiple of 64", "nt", _S, dict(colscale_n=32, colscale=0.5), PA_EINVAL),
    ("colscale_n outside STORE", "nt", _G, dict(colscale_n=64, colscale=0.5), PA_EINVAL),
    ("colsum_out without colsum_ws", "nt", _D, dict(colsum_ws=None), PA_EINVAL),
    ("A NULL", "nt", _S, dict(A=None), PA_EINVAL),
    ("B NULL", "nt", _S, dict(B=None), PA_EINVAL),
    ("M = 0", "nt", _S, dict(M=0), PA_EINVAL),
    ("STORE without out_lp", "nt", _S, dict(out_lp=None), PA_EINVAL),
    ("GELU without out_lp2", "nt", _G, dict(out_lp2=None), PA_EINVAL),
    ("RESID without resid", "nt", _R, dict(resid=None), PA_EINVAL),
    ("DGELU without aux", "nt", replace(_D, colsum=""), dict(aux=None), PA_EINVAL),
    ("PARTIAL on tune 13", "nt", replace(_P, tune=13), dict(), PA_EINVAL),
    ("PARTIAL on tune 19", "nt", replace(_P, tune=19), dict(), PA_EINVAL),
    ("an unknown tune", "nt", replace(_S, tune=5), dict(), PA_EINVAL),
    ("BLOCKED_PRE on a shape pa_gemm_blocked_pre_ok refuses", "nt", replace(_G, flags=BLOCKED_PRE), dict(), PA_EUNSUPPORTED),
    ("a row factor outside RESID", "rowscale", replace(_S, factors=True, entry="rowscale"), dict(), PA_EINVAL),
    ("a row factor with the row remap", "rowscale", replace(_R, factors=True, entry="rowscale"), dict(row_mod=8, out_batch_rows=10, out_row_off=2), PA_EINVAL),
    ("a row factor with the row remap, split-K", "splitk_rowscale", replace(_R, factors=True, entry="splitk_rowscale"),
     dict(row_mod=8, out_batch_rows=10, out_row_off=2), PA_EINVAL),
)
_T = TN(PA_BF16, 16, 16, 16)
TN_ARG_CASES = (
    ("an epilogue other than PARTIAL", _T, dict(epilogue=STORE), PA_EUNSUPPORTED),
    ("M below one 16-byte vector", _T, dict(M=4), PA_EUNSUPPORTED),
    ("N % 8", _T, dict(N=12), PA_EUNSUPPORTED),
    ("ldo32 % 4", _T, dict(ldo32=18), PA_EUNSUPPORTED),
    ("lda off 16 bytes", _T, dict(lda=20), PA_EUNSUPPORTED),
    ("split_k = 0", _T, dict(split_k=0), PA_EINVAL),
    ("out_f32 NULL", _T, dict(out_f32=None), PA_EINVAL),
    ("colsum_ws with tune 1", replace(_T, tune=1, colsum=True), dict(), PA_EUNSUPPORTED),
    ("colsum_ws in f32", replace(_T, dt=PA_F32, colsum=True), dict(), PA_EUNSUPPORTED),
)


# ---- the rel_err metric of the random-operand tests ------------------------------------------------------------------------
def old_metric_passes(c, o):
    """would max|got - ref| / max|ref| of the case's main output pass the bound tests/test_gpu_kernels.py applies to it?"""
    i = nt_inputs(c)
    r = nt_reference(c, i)
    if c.epi == STORE:
        got, ref, bound = o["out_lp"].view[:, :c.N], r["out_lp"], OLD_BOUND_LP if c.dt == PA_BF16 else 2e-5
    else:
        got, ref, bound = o["out_f32"].view[:, :c.N], r["out_f32"], OLD_BOUND_F32_OF_BF16
    return rel_err(got, ref) < bound

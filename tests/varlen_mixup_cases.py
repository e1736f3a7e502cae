"""Cases, references and checkers of the ragged spectrogram mixup (pa_mixup_varlen / ops.mixup_varlen).

Used by tests/test_gpu_varlen_step.py (the HIP kernel through ops.mixup_varlen) and tests/test_varlen_mixup_cases_cpu.py (the same
checkers against `TorchMixup`, a plain-torch restatement, and against fault models that must be rejected).  A checker builds the
operands on the CPU inside guarded buffers, hands an `impl` the flat buffers and gets the flat buffers back; it neither knows nor
cares where the arithmetic ran.

The definition (clip i has n_i valid frames, j = perm[i]):

    t <  n_i :  out[i, f, t] = x[i, f, t] * lam_i + (x[j, f, t] if t < n_j else pad) * (1 - lam_i)
    t >= n_i :  out[i, f, t] = 0.0 exactly

Buffers: x and out are views into larger allocations with GUARD (at least one row of) NaN on either side; x holds NaN behind every
clip's length as well, and the out view starts as NaN, so an element that was never written, a value taken from behind a length and a
tail that was multiplied by zero instead of chosen all show as a non-finite output.

Shapes: B = 4 clips of 3 rows, row pitch 40 (16-byte groups) and 37 (4-byte accesses), pitch 40 one element off 16-byte
alignment (4-byte accesses by the pointers), and 4 rows of pitch 37 (16-byte groups that run over the rows' ends).  Lengths
(1, ldt, 18, 5): 18 and 5 fall inside a 16-byte group (16..19, 4..7), 1 leaves a group's first lane only.  The permutations between them hold a clip with itself, a longer partner, a shorter partner, and the
full-length clip as partner of the 1-frame clip.

Families:
  exact    x small integers (distinct between clips, rows and columns), lam in {0.5, 0.75, 1.0}, pad = -3.0: every product is a
           multiple of 1/4 below 2^8 and every sum is exact whatever the compiler contracts; torch.equal against the definition
           computed in float64 and cast.
  graded   x uniform in +-1.5, lam from the beta draw of the training step (max(l, 1 - l), so 1 - lam is exact in f32: Sterbenz),
           pad the step's default: per element |got - want64| <= 2^-23 (|a l| + |c (1 - l)|), two roundings -- the product
           c (1 - l) and the sum -- which covers the fused (product, then one fma) and the unfused (two products, one sum: three
           roundings of which the two products' add up to 2^-24 (|a l| + |c (1 - l)|)) evaluation alike.
Always: out exactly 0.0 behind n_i, finite everywhere, guards intact, x untouched, two runs bit-identical.
Full lengths at pitch 40: torch.equal with the fixed-shape mixup of the same impl (ops.mixup on the GPU).
"""
import math
from dataclasses import dataclass

import numpy as np
import torch

GUARD = 256
B, ROWS = 4, 3
LDTS = (40, 37)
DEFAULT_PAD = float(np.float32((math.log(1e-5) + 4.5) / 5.0))      # passt_amd.train.MIXUP_PAD
EXACT_PAD = -3.0
EXACT_LAM = (0.75, 0.5, 1.0, 0.75)
# i -> perm[i] over lengths (1, ldt, 18, 5)
PERMS = {
    "swap": (1, 0, 3, 2),      # 1-frame clip with the full-length one and back; 18 with the shorter 5, 5 with the longer 18
    "self": (0, 2, 1, 3),      # clips 0 and 3 with themselves; full with the shorter 18, 18 with the longer full
    "cycle": (3, 2, 0, 1),     # 1 with the longer 5; full with 18; 18 with the 1-frame clip (cut inside group 0); 5 with the full one
}


def lengths(ldt):
    return (1, ldt, 18, 5)


@dataclass(frozen=True)
class Case:
    ldt: int
    perm: str
    family: str                 # "exact" / "graded"
    offset: int = 0             # elements x and out are moved off 16-byte alignment
    full: bool = False          # every length = ldt
    rows: int = ROWS

    @property
    def id(self):
        return (f"ldt{self.ldt}-{self.perm}-{self.family}" + (f"-off{self.offset}" if self.offset else "") + ("-full" if self.full else "")
                + (f"-rows{self.rows}" if self.rows != ROWS else ""))


CASES = tuple(Case(ldt, perm, fam) for ldt in LDTS for perm in PERMS for fam in ("exact", "graded")) + (
    Case(40, "cycle", "exact", offset=1), Case(40, "swap", "graded", offset=1),
    # four rows of 37: a clip is a whole number of 16-byte groups although a row is not, and groups run over the rows' ends
    Case(37, "swap", "exact", rows=4), Case(37, "cycle", "exact", rows=4), Case(37, "self", "graded", rows=4))
FULL_CASES = (Case(40, "swap", "graded", full=True), Case(40, "cycle", "exact", full=True))


# ---- operands ----------------------------------------------------------------------------------------------------------------
def guarded(t, offset=0, fill=float("nan")):
    """(flat buffer, index of the view's first element): `t` inside an allocation with GUARD (at least one row of) `fill` on both sides"""
    n, guard = t.numel(), max(GUARD, t.shape[-1])
    buf = torch.full((guard + offset + n + guard,), fill, dtype=t.dtype)
    buf[guard + offset:guard + offset + n] = t.reshape(-1)
    return buf, guard + offset


def operands(case):
    """x (B, ROWS, ldt) f32 with NaN behind every clip's length, lens / perm (int32), lam (f32), pad"""
    ldt = case.ldt
    lens = (ldt,) * B if case.full else lengths(ldt)
    if case.family == "exact":
        b, r, t = torch.arange(B)[:, None, None], torch.arange(case.rows)[None, :, None], torch.arange(ldt)[None, None, :]
        x = (((b * 131 + r * 17 + t * 7) % 255) - 127).float()
        lam, pad = torch.tensor(EXACT_LAM, dtype=torch.float32), EXACT_PAD
    else:
        g = torch.Generator().manual_seed(11 + ldt)
        x = (torch.rand(B, case.rows, ldt, generator=g) * 2 - 1) * 1.5
        l = np.random.RandomState(5 + ldt).beta(0.3, 0.3, B).astype(np.float32)
        lam, pad = torch.from_numpy(np.maximum(l, 1.0 - l)), DEFAULT_PAD
        assert bool(((lam >= 0.5) & (lam <= 1.0)).all())
    for i, n in enumerate(lens):
        x[i, :, n:] = float("nan")
    return x, torch.tensor(lens, dtype=torch.int32), torch.tensor(PERMS[case.perm], dtype=torch.int32), lam, pad


def definition(x, lens, perm, lam, pad):
    """The definition in float64: (want (B, ROWS, ldt) f64, |a l| + |c (1 - l)| per element -- 0 behind n_i)"""
    Bn, rows, ldt = x.shape
    t = torch.arange(ldt)[None, None, :]
    ni, nj = lens.long()[:, None, None], lens.long()[perm.long()][:, None, None]
    l = lam.double()[:, None, None]
    a = torch.where(t < ni, x.double(), torch.zeros((), dtype=torch.float64))
    c = torch.where(t < nj, x.double()[perm.long()], torch.full((), float(np.float32(pad)), dtype=torch.float64))
    al, cl = a * l, c * (1.0 - l)
    inside = (t < ni).expand(Bn, rows, ldt)
    zero = torch.zeros((), dtype=torch.float64)
    return torch.where(inside, al + cl, zero), torch.where(inside, al.abs() + cl.abs(), zero)


# ---- the plain-torch restatement -------------------------------------------------------------------------------------------------
class TorchMixup:
    """f32 torch on the CPU.  mixup_varlen takes the flat guarded buffers and returns them (x's as it is afterwards, out's written)."""

    def views(self, xbuf, x_lo, obuf, o_lo, shape):
        n = math.prod(shape)
        return xbuf[x_lo:x_lo + n].view(shape), obuf[o_lo:o_lo + n].view(shape)

    # the pieces a fault model overrides
    def partner(self, x, perm, t, nj, pad):
        return torch.where(t < nj, x[perm.long()], torch.full((), pad, dtype=torch.float32))

    def mix(self, a, c, l):
        return a * l + c * (1.0 - l)

    def tail(self, mix, t, ni, out):
        return torch.where(t < ni, mix, torch.zeros((), dtype=torch.float32))

    def mixup_varlen(self, xbuf, x_lo, obuf, o_lo, shape, lens, perm, lam, pad):
        xbuf, obuf = xbuf.clone(), obuf.clone()
        x, out = self.views(xbuf, x_lo, obuf, o_lo, shape)
        t = torch.arange(shape[-1])[None, None, :]
        ni, nj = lens.long()[:, None, None], lens.long()[perm.long()][:, None, None]
        c = self.partner(x, perm, t, nj, float(np.float32(pad)))
        out.copy_(self.tail(self.mix(x, c, lam[:, None, None]), t, ni, out))
        return xbuf, obuf

    def mixup(self, x, perm, lam):
        """the fixed-shape mixup of the same arithmetic"""
        return self.mix(x, x[perm.long()], lam[:, None, None])


# ---- the host draws of a ragged step ---------------------------------------------------------------------------------------------
def host_draws(mel, net, lengths, alpha, use_mixup=True):
    """The documented host sequence of TrainStep.step(..., lengths=), with the library's own draw functions: all front-end draws of the
    batch clip after clip (``mel`` given: ``lengths`` are samples; a front end in eval mode draws its two randint per call), then
    randperm and beta, then the Patchout draws clip after clip.  Returns dict(frames, front, perm, lam, geometry)."""
    from passt_amd.passt import varlen_geometry_train
    from passt_amd.preprocess import varlen_clip_draws
    front, frames = None, [int(n) for n in lengths]
    if mel is not None:
        if mel.training:
            front = varlen_clip_draws(mel, lengths)
            frames = front["frames"]
        else:
            torch.randint(mel.fmin_aug_range, (1,))
            torch.randint(mel.fmax_aug_range, (1,))
            frames = [1 + (n - 1) // mel.hopsize for n in frames]
    perm = lam = None
    if use_mixup:
        perm = torch.randperm(len(frames))
        lam = np.random.beta(alpha, alpha, len(frames)).astype(np.float32)
        lam = np.maximum(lam, 1.0 - lam)
    return dict(frames=frames, front=front, perm=perm, lam=lam, geometry=varlen_geometry_train(net, frames))


# ---- checkers ------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def run(impl, case):
    """One call through `impl` on guarded buffers; checks what holds always and returns (out (B, ROWS, ldt) f32, the operands)."""
    x, lens, perm, lam, pad = operands(case)
    shape, n = tuple(x.shape), x.numel()
    xbuf, x_lo = guarded(x, case.offset)
    obuf, o_lo = guarded(torch.full(shape, float("nan")), case.offset)
    xb1, ob1 = impl.mixup_varlen(xbuf, x_lo, obuf, o_lo, shape, lens, perm, lam, pad)
    xb2, ob2 = impl.mixup_varlen(xbuf, x_lo, obuf, o_lo, shape, lens, perm, lam, pad)
    what = case.id
    assert torch.equal(_bits(xb1), _bits(xbuf)) and torch.equal(_bits(xb2), _bits(xbuf)), f"{what}: x or its guards were written"
    assert bool(torch.isnan(ob1[:o_lo]).all()) and bool(torch.isnan(ob1[o_lo + n:]).all()), f"{what}: a write outside out"
    assert torch.equal(_bits(ob1), _bits(ob2)), f"{what}: two runs differ in their bits"
    out = ob1[o_lo:o_lo + n].view(shape).clone()
    bad = ~torch.isfinite(out)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} outputs are not finite (never written, taken from behind a length, or a "
                                 f"tail multiplied instead of chosen), first at {bad.nonzero()[0].tolist()}")
    for i, ni in enumerate(lens.tolist()):
        tail = out[i, :, ni:]
        assert bool((_bits(tail) == 0).all()) if tail.numel() else True, f"{what}: clip {i} is not exactly +0.0 behind its {ni} frames"
    return out, (x, lens, perm, lam, pad)


def check_case(impl, case):
    """The family's check of one case: returns the worst ratio |error| / bound (graded) or 0.0 (exact)."""
    out, (x, lens, perm, lam, pad) = run(impl, case)
    want, mag = definition(x, lens, perm, lam, pad)
    if case.family == "exact":
        w32 = want.float()
        assert torch.equal(w32.double(), want), f"{case.id}: the exact family is not exact"
        if not torch.equal(out, w32):
            bad = out != w32
            idx = tuple(bad.nonzero()[0].tolist())
            raise AssertionError(f"{case.id}: {int(bad.sum())} of {out.numel()} elements differ, first at {idx}: got {float(out[idx])}, "
                                 f"want {float(w32[idx])}")
        return 0.0
    err, bound = (out.double() - want).abs(), 2.0 ** -23 * mag
    over = err > bound
    if bool(over.any()):
        idx = tuple(over.nonzero()[0].tolist())
        raise AssertionError(f"{case.id}: {int(over.sum())} elements beyond 2^-23 (|a l| + |c (1 - l)|), first at {idx}: error "
                             f"{float(err[idx]):.3e}, bound {float(bound[idx]):.3e}")
    inside = mag > 0
    return float((err[inside] / bound[inside]).max())


def check_full(impl, case):
    """Every length = ldt, ldt % 4 == 0: bit for bit the fixed-shape mixup of the same impl, and the family's own check."""
    assert case.full and case.ldt % 4 == 0 and case.offset == 0
    out, (x, lens, perm, lam, pad) = run(impl, case)
    assert not bool(torch.isnan(x).any())
    fixed = impl.mixup(x, perm, lam)
    assert torch.equal(_bits(out), _bits(fixed)), f"{case.id}: {int((out != fixed).sum())} elements differ from the fixed-shape mixup"
    return check_case(impl, case)

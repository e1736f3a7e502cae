"""Cases, float64 truth and checkers of the ragged waveform augmentation (pa_wave_augment_varlen / ops.wave_augment_varlen /
WaveAugment(..., ragged=True)).  No device needed: tests/test_gpu_wave_varlen.py runs the checkers on the HIP kernel through the C
ABI, tests/test_wave_varlen_cases_cpu.py on `NumpyWave`, a plain float32 numpy restatement, and on fault models that must be rejected.
A checker builds the operands on the CPU inside guarded buffers, hands an `impl` the flat buffers and gets the flat buffers back.

The definition (row b has n_b = olen[b] samples; "clip c as row b sees it" is gain, pad_or_truncate(n_b), roll(shift[c])):

    m            = min(len[c], n_b)
    s(t)         = (t - shift[c]) mod n_b                      true modulo
    item(c|b)[t] = x[c][s(t)] * amp[c] if s(t) < m else 0      0 <= t < n_b
    mean(c|b)    = (amp[c] / n_b) * sum_{s < m} x[c][s]
    unmixed:       out[b][t] = item(b|b)[t]
    mixed with p:  l = max(lam[b], 1 - lam[b]);  out[b][t] = (item(b|b)[t] - mean(b|b)) l + (item(p|b)[t] - mean(p|b)) (1 - l)
    n_b <= t < L:  out[b][t] = +0.0

Buffers: x [B][ldx] and out [B][ldo], ldo > L, are views into larger allocations with GUARD NaNs on either side; x holds NaN behind
every len[c], the whole out allocation starts as NaN.  A sample that was never written, a value read from behind a length, a tail
multiplied by zero instead of chosen and a write into the pitch gap or the guards all show.

Cases (the smallest shapes at which the kernel can go wrong):
  ragged   B = 6, len (1, 3, 64, 1027, 4099, 2050), ldx = 4100, clip_samples = 3000 cuts clip 4: n = (1, 3, 64, 1027, 3000, 2050),
           L = 3000 (three workgroups' worth of 16-byte groups per row and a 4-byte remainder: ldo = 3008 keeps rows aligned).  Partners:
           row 0 a longer clip that is itself mixed, row 1 itself, row 2 unmixed, row 3 a shorter, unmixed clip, row 4 a shorter clip that
           is itself mixed, row 5 a longer clip cut to it.  lam (0.3, 0.5, -, 0, 1, 0.3).
  equal    B = 4, every len = n = L = 4096 (ldx = 4100 so that NaNs stand behind): equal lengths, one partner itself, one row unmixed; the
           case that is also run through pa_wave_augment.
  skew     the ragged shapes with ldo = L + 3 and x and out one element off 16-byte alignment: every row starts at another alignment.
Shifts are taken per clip from {0, 1, -1, n - 1, n, n + 7, -(2 n + 3), 50} (n the clip's own length), so that a clip mixed into a
shorter row is also rolled by more than that row's length.  Gains -7 .. 6 dB.  Inputs 0.3 randn + 0.01 i, the scale of the fixed entry's
oracle test (tests/test_gpu_kernels.py), whose cap of 5e-7 against oracle.wave_oracle is the cap of `check_oracle` here.

Bounds.  Unmixed rows: equal, bit for bit, to the float32 product x * amp, rolled (one f32 multiplication, the one the oracle does).
Mixed rows: per element against the float64 truth, derived below in `bound` from the arithmetic -- never from an implementation's output.
"""
import copy
from dataclasses import dataclass, field

import numpy as np

GUARD = 256
U = 2.0 ** -24                       # unit roundoff of float32
ORACLE_CAP = 5e-7                    # tests/test_gpu_kernels.py::test_wave_augment_matches_reference_pipeline, same input scale
PA_OK, PA_EINVAL = 0, -1
NAN = float("nan")


@dataclass(frozen=True)
class Case:
    name: str
    lens: tuple                      # valid samples per row of x
    ldx: int
    clip_samples: int                # WaveAugment's cap: n_b = min(len_b, clip_samples)
    ldo: int
    gain_db: tuple
    shift: tuple
    partner: tuple
    lam: tuple
    x_off: int = 0                   # elements x / out are moved off 16-byte alignment
    o_off: int = 0
    seed: int = 0
    B: int = field(init=False)
    olen: tuple = field(init=False)
    L: int = field(init=False)

    def __post_init__(self):
        object.__setattr__(self, "B", len(self.lens))
        object.__setattr__(self, "olen", tuple(min(n, self.clip_samples) for n in self.lens))
        object.__setattr__(self, "L", max(self.olen))
        assert self.ldo > self.L and self.ldx >= max(self.lens)
        assert all(len(v) == self.B for v in (self.gain_db, self.shift, self.partner, self.lam))

    def with_lens(self, lens):
        """the same rows (olen, L) over clips of other valid lengths: what an impulse response's tail makes of a batch"""
        other = copy.copy(self)
        object.__setattr__(other, "lens", tuple(int(v) for v in lens))
        assert other.ldx >= max(other.lens)
        return other

    @property
    def amp(self):                   # what WaveAugment hands the kernel: 10^(dB/20) evaluated in float64, rounded once
        return (10.0 ** (np.asarray(self.gain_db, np.float64) / 20.0)).astype(np.float32)


_RAGGED = dict(lens=(1, 3, 64, 1027, 4099, 2050), ldx=4100, clip_samples=3000, partner=(4, 1, -1, 2, 0, 4),
               lam=(0.3, 0.5, 1.0, 0.0, 1.0, 0.3))
RAGGED = Case("ragged", ldo=3008, gain_db=(-7, 6, 0, -3, 2, 5),
              # n + 7, -(2 n + 3), 50, -1, n - 1 (n = 3000), 1: clip 4 rolled by 2999 is rolled by 2999 mod 1 and mod 2050 where it is a partner
              shift=(8, -9, 50, -1, 2999, 1), seed=1, **_RAGGED)
EQUAL = Case("equal", lens=(4096,) * 4, ldx=4100, clip_samples=4096, ldo=4100, gain_db=(6, -7, 1, -2),
             shift=(4095, -(2 * 4096 + 3), 0, 4096 + 7), partner=(1, 1, -1, 0), lam=(0.3, 0.5, 1.0, 0.0), seed=2)
SKEW = Case("skew", ldo=3003, gain_db=(3, -6, 4, -1, -5, 0),
            # 0, n, -(2 n + 3), n + 7, 50, n
            shift=(0, 3, -131, 1034, 50, 2050), x_off=1, o_off=1, seed=3, **_RAGGED)
CASES = (RAGGED, EQUAL, SKEW)


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def make_x(case):
    """x (B, ldx) f32: 0.3 randn + 0.01 i, NaN behind every len"""
    rng = np.random.default_rng(100 + case.seed)
    x = (0.3 * rng.standard_normal((case.B, case.ldx)) + 0.01 * np.arange(case.B)[:, None]).astype(np.float32)
    for c, n in enumerate(case.lens):
        x[c, n:] = NAN
    return x


def guarded(a, offset, pitch=None):
    """(flat f32 buffer, index of a's first element): the rows of `a` at `pitch` inside an allocation of NaN with GUARD on both sides"""
    rows, cols = a.shape
    pitch = cols if pitch is None else pitch
    buf = np.full(GUARD + offset + rows * pitch + GUARD, NAN, np.float32)
    view = buf[GUARD + offset:GUARD + offset + rows * pitch].reshape(rows, pitch)
    view[:, :cols] = a
    return buf, GUARD + offset


def rows_of(buf, lo, rows, pitch):
    return buf[lo:lo + rows * pitch].reshape(rows, pitch)


# ---- the definition in float64 ------------------------------------------------------------------------------------------------------------
def _src(t, shift, n):
    return (t - int(shift)) % n                              # numpy's % on int64 is the true modulo


def item64(x, case, c, n):
    """(item(c|b) for a row of n samples, its mean), float64, from the float32 operands"""
    m = min(case.lens[c], n)
    amp = float(case.amp[c])
    s = _src(np.arange(n, dtype=np.int64), case.shift[c], n)
    it = np.zeros(n, np.float64)
    inside = s < m
    it[inside] = x[c, s[inside]].astype(np.float64) * amp
    return it, amp / n * float(np.sum(x[c, :m].astype(np.float64)))


def mean_error(x, case, c, n):
    """Bound on |f32 mean - mean(c|b)| for the reduction the kernel documents (include/passt_amd.h): 1024 threads, thread i adds its
    k = ceil(m / 1024) samples in order (k - 1 roundings), a 64-lane butterfly (6), a butterfly over the 16 wave sums (at most 6 more;
    an addition of 0 is exact), then sum * amp and / n, one rounding each: gamma(k + 13) times (amp / n) sum |x|.  It is a
    worst case for that shape and is not widened for any other: `NumpyWave` sums pairwise (numpy), whose longest path has a few
    roundings more and whose actual error, like the kernel's, is a small fraction of this."""
    m = min(case.lens[c], n)
    j = -(-m // 1024) + 13
    return (j * U / (1.0 - j * U)) * float(case.amp[c]) / n * float(np.sum(np.abs(x[c, :m].astype(np.float64))))


def definition(x, case):
    """(want (B, L) f64, bound (B, L) f64 -- 0 on unmixed rows and behind n_b --, exact (B, L) f32: what an unmixed row must equal)

    The bound of a mixed element, with u = 2^-24, I = |item|, A = item(b|b) - mean(b|b), C = item(p|b) - mean(p|b), E = mean_error:
      the items        x * amp is rounded once:                      u I_b, u I_p
      the means        E_b, E_p
      the subtractions one rounding each:                            u |A|, u |C|          -> |dA| <= u I_b + E_b + u |A|, same for C
      l = fl(1 - lam)  where lam < 1/2 (exact otherwise: Sterbenz) is off by at most u l, and 1 - l, exact in f32, carries that error
                       into the other weight:                        u l (|A| + |C|)
      the products     A l and C (1 - l), one rounding each (a fused multiply-add drops the first):   u (l |A| + (1 - l) |C|)
      the sum          one rounding:                                 u |out|  <=  u (l |A| + (1 - l) |C|)
    Together  l |dA| + (1 - l) |dC| + u l (|A| + |C|) + 2 u (l |A| + (1 - l) |C|),  times 1 + 2^-10 for the products of two such terms."""
    B, L = case.B, case.L
    want, bnd, exact = np.zeros((B, L)), np.zeros((B, L)), np.zeros((B, L), np.float32)
    for b in range(B):
        n, p = case.olen[b], case.partner[b]
        ib, mb = item64(x, case, b, n)
        m = min(case.lens[b], n)
        s = _src(np.arange(n, dtype=np.int64), case.shift[b], n)
        row = np.zeros(n, np.float32)
        row[s < m] = x[b, s[s < m]] * case.amp[b]             # one float32 multiplication
        exact[b, :n] = row
        if p < 0:
            want[b, :n] = ib
            continue
        lam = float(np.float32(case.lam[b]))
        l = max(lam, 1.0 - lam)
        ip, mp = item64(x, case, p, n)
        A, C = ib - mb, ip - mp
        want[b, :n] = A * l + C * (1.0 - l)
        dA = U * np.abs(ib) + mean_error(x, case, b, n) + U * np.abs(A)
        dC = U * np.abs(ip) + mean_error(x, case, p, n) + U * np.abs(C)
        wsum = l * np.abs(A) + (1.0 - l) * np.abs(C)
        bnd[b, :n] = (l * dA + (1.0 - l) * dC + U * l * (np.abs(A) + np.abs(C)) + 2.0 * U * wsum) * (1.0 + 2.0 ** -10)
    return want, bnd, exact


def oracle_rows(x, case):
    """oracle.wave_oracle applied clip by clip at L = n_b: one float32 array of n_b samples per row"""
    from oracle import wave_oracle as W
    rows = []
    for b in range(case.B):
        n, p = case.olen[b], case.partner[b]
        own = W.item(x[b, :case.lens[b]], case.gain_db[b], case.shift[b], n)[0]
        if p < 0:
            rows.append(own)
        else:
            rows.append(W.wav_mixup(own, W.item(x[p, :case.lens[p]], case.gain_db[p], case.shift[p], n)[0], float(np.float32(case.lam[b])))[0])
    return rows


# ---- the plain numpy restatement and its fault models ---------------------------------------------------------------------------------------
class NumpyWave:
    """float32 numpy on the CPU.  wave_augment_varlen takes the flat guarded buffers and returns them (x's as it is afterwards, out's
    written).  The small methods are the pieces a fault model overrides."""

    def wrap(self, case, b, c):               # the length the roll of clip c wraps at in row b
        return case.olen[b]

    def src(self, t, shift, n):
        return (t - int(shift)) % n

    def valid(self, case, b, c):              # samples of clip c that row b uses
        return min(case.lens[c], case.olen[b])

    def shift(self, case, b, c):
        return case.shift[c]

    def mean(self, x, case, b, c):
        m = self.valid(case, b, c)
        return np.float32(np.float32(np.sum(x[c, :m], dtype=np.float32) * case.amp[c]) / np.float32(case.olen[b]))

    def weight(self, lam):
        return max(lam, np.float32(1.0) - lam)

    def item(self, x, case, b, c):
        n, m = case.olen[b], self.valid(case, b, c)
        s = self.src(np.arange(n, dtype=np.int64), self.shift(case, b, c), self.wrap(case, b, c))
        it = np.zeros(n, np.float32)
        inside = (s >= 0) & (s < m)
        it[inside] = x[c, s[inside]] * case.amp[c]
        return it

    def finish(self, case, out):              # out: the (B, ldo) view, rows written in [0, L)
        pass

    def wave_augment_varlen(self, xbuf, x_lo, obuf, o_lo, case):
        xbuf, obuf = xbuf.copy(), obuf.copy()
        x, out = rows_of(xbuf, x_lo, case.B, case.ldx), rows_of(obuf, o_lo, case.B, case.ldo)
        for b in range(case.B):
            n, p = case.olen[b], case.partner[b]
            row = self.item(x, case, b, b)
            if p >= 0:
                l = self.weight(np.float32(case.lam[b]))
                row = (row - self.mean(x, case, b, b)) * l + (self.item(x, case, b, p) - self.mean(x, case, b, p)) * (np.float32(1.0) - l)
            out[b, :n] = row
            out[b, n:case.L] = 0.0
        self.finish(case, out)
        return xbuf, obuf

    def wave_augment(self, x, case):
        """the fixed-shape entry of the same arithmetic (every n_b = L): dense (B, L)"""
        xbuf, lo = guarded(x, 0)
        obuf, o_lo = guarded(np.full((case.B, case.L), NAN, np.float32), 0, case.ldo)
        _, ob = self.wave_augment_varlen(xbuf, lo, obuf, o_lo, case)
        return rows_of(ob, o_lo, case.B, case.ldo)[:, :case.L].copy()


class RollAtLongest(NumpyWave):               # roll modulo the batch's longest length instead of n_b
    def wrap(self, case, b, c):
        return case.L


class PartnerOwnMean(NumpyWave):              # the partner centred by its mean over its own length (one mean per clip)
    def mean(self, x, case, b, c):
        if c == b:
            return super().mean(x, case, b, c)
        m = case.olen[c]
        return np.float32(np.float32(np.sum(x[c, :min(case.lens[c], m)], dtype=np.float32) * case.amp[c]) / np.float32(m))


class PartnerNotCut(NumpyWave):               # the partner rolled at its own length, then cut to n_b
    def wrap(self, case, b, c):
        return case.olen[b] if c == b else max(case.olen[c], case.olen[b])

    def valid(self, case, b, c):
        return min(case.lens[c], case.olen[b]) if c == b else case.lens[c]


class PartnerShiftIgnored(NumpyWave):
    def shift(self, case, b, c):
        return case.shift[c] if c == b else 0


class RawLam(NumpyWave):                      # lam instead of max(lam, 1 - lam)
    def weight(self, lam):
        return lam


class SingleWrap(NumpyWave):                  # t - shift corrected by one +-n only: wrong for |shift| >= n
    def src(self, t, shift, n):
        s = t - int(shift)
        s = np.where(s < 0, s + n, s)
        return np.where(s >= n, s - n, s)


class ReadsBehindPartner(NumpyWave):          # the partner taken as n_b valid samples whatever its length
    def valid(self, case, b, c):
        return min(case.lens[c], case.olen[b]) if c == b else min(case.olen[b], case.ldx)


class TailNotZero(NumpyWave):
    def finish(self, case, out):
        for b, n in enumerate(case.olen):
            out[b, n:case.L] = 1e-3


class NegativeZeroTail(NumpyWave):            # a tail multiplied by zero: -0.0 where the product was negative
    def finish(self, case, out):
        for b, n in enumerate(case.olen):
            out[b, n:case.L] = -0.0


class WritesPitchGap(NumpyWave):
    def finish(self, case, out):
        out[:, case.L] = 0.0


FAULTS = (RollAtLongest, PartnerOwnMean, PartnerNotCut, PartnerShiftIgnored, RawLam, SingleWrap, ReadsBehindPartner, TailNotZero,
          NegativeZeroTail, WritesPitchGap)


# ---- checkers --------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


_TRUTH = {}


def truth(case):
    """(x, want, bound, exact) of a case, computed once and shared (read-only)"""
    if case.name not in _TRUTH:
        x = make_x(case)
        arrays = (x,) + definition(x, case)
        for a in arrays:
            a.setflags(write=False)
        _TRUTH[case.name] = arrays
    return _TRUTH[case.name]


def run(impl, case):
    """One call (and a second, which must give the same bits) through `impl` on guarded buffers; checks what holds always and returns
    out (B, L) f32."""
    x = truth(case)[0]
    B, L, ldo = case.B, case.L, case.ldo
    xbuf, x_lo = guarded(x, case.x_off)
    obuf, o_lo = guarded(np.full((B, L), NAN, np.float32), case.o_off, ldo)
    xb1, ob1 = impl.wave_augment_varlen(xbuf, x_lo, obuf, o_lo, case)
    xb2, ob2 = impl.wave_augment_varlen(xbuf, x_lo, obuf, o_lo, case)
    what = case.name
    assert np.array_equal(_bits(xb1), _bits(xbuf)) and np.array_equal(_bits(xb2), _bits(xbuf)), f"{what}: x or its guards were written"
    assert np.isnan(ob1[:o_lo]).all() and np.isnan(ob1[o_lo + B * ldo:]).all(), f"{what}: a write into out's guards"
    view = rows_of(ob1, o_lo, B, ldo)
    assert np.isnan(view[:, L:]).all(), f"{what}: a write into the pitch gap out[b][L:ldo)"
    assert np.array_equal(_bits(ob1), _bits(ob2)), f"{what}: two runs differ in their bits"
    out = view[:, :L].copy()
    bad = ~np.isfinite(out)
    assert not bad.any(), (f"{what}: {int(bad.sum())} outputs are not finite (never written, read from behind a length, or multiplied "
                           f"instead of chosen), first at {tuple(np.argwhere(bad)[0])}")
    for b, n in enumerate(case.olen):
        assert (_bits(out[b, n:]) == 0).all(), f"{what}: row {b} is not exactly +0.0 behind its {n} samples"
    return out


def check_case(impl, case):
    """Unmixed rows bit for bit, mixed rows within the derived bound.  Returns the worst |error| / bound over the mixed elements."""
    out = run(impl, case)
    _, want, bnd, exact = truth(case)
    worst = 0.0
    for b in range(case.B):
        n = case.olen[b]
        if case.partner[b] < 0:
            same = _bits(out[b, :n]) == _bits(exact[b, :n])
            assert same.all(), (f"{case.name}: unmixed row {b} differs from x * amp rolled in {int((~same).sum())} of {n} samples, first at "
                                f"{int(np.argmin(same))}: got {out[b, int(np.argmin(same))]!r}, want {exact[b, int(np.argmin(same))]!r}")
            continue
        err = np.abs(out[b, :n].astype(np.float64) - want[b, :n])
        over = err > bnd[b, :n]
        if over.any():
            t = int(np.argmax(over))
            raise AssertionError(f"{case.name}: row {b}: {int(over.sum())} of {n} samples beyond the bound, first at {t}: error {err[t]:.3e}, "
                                 f"bound {bnd[b, t]:.3e}")
        worst = max(worst, float((err / bnd[b, :n]).max()))
    return worst


def check_oracle(impl, case):
    """Every row against oracle.wave_oracle run on the pair (b, partner[b]) alone at L = n_b, under the fixed entry's cap.  Returns the
    largest |error|."""
    out = run(impl, case)
    worst = 0.0
    for b, ref in enumerate(oracle_rows(truth(case)[0], case)):
        e = float(np.abs(out[b, :case.olen[b]] - ref).max())
        assert e < ORACLE_CAP, f"{case.name}: row {b} is {e:.3e} from the oracle at L = {case.olen[b]} (cap {ORACLE_CAP})"
        worst = max(worst, e)
    return worst


def check_equal_lengths(impl, case=EQUAL):
    """Every n_b = L: against the fixed-shape entry of the same impl on the same operands.  Unmixed rows bit for bit, mixed rows within
    the derived bound of each other: both entries take a clip's sum from one reduction, so the means are the same numbers and only
    the roundings of the mix itself can differ, which the bound holds several times over.  Returns whether the mixed rows are
    bit-identical as well (reported, not required)."""
    assert all(n == case.L for n in case.olen)
    out = run(impl, case)
    x, _, bnd, _ = truth(case)
    fixed = impl.wave_augment(x, case)
    identical = True
    for b in range(case.B):
        if case.partner[b] < 0:
            assert np.array_equal(_bits(out[b]), _bits(fixed[b])), f"{case.name}: unmixed row {b} differs from the fixed entry's"
            continue
        err = np.abs(out[b].astype(np.float64) - fixed[b].astype(np.float64))
        assert (err <= bnd[b]).all(), f"{case.name}: row {b} is {float((err / bnd[b]).max()):.2f} bounds from the fixed entry's"
        identical = identical and np.array_equal(_bits(out[b]), _bits(fixed[b]))
    return identical


# ---- refusals: (what, args of pa_wave_augment_varlen, expected return) ----------------------------------------------------------------------------
def refusal_table(p):
    """`p`: any non-NULL address; none of the refused calls may launch, so it is never dereferenced"""
    good = dict(x=p, B=4, ldx=9000, len=p, olen=p, amp=p, shift=p, partner=p, lam=p, ws=p, out=p + 4096, ldo=8000, L=8000)
    rows = []
    for what, change in (("x NULL", dict(x=None)), ("out NULL", dict(out=None)), ("olen NULL", dict(olen=None)), ("B 0", dict(B=0)),
                         ("B -3", dict(B=-3)), ("ldx 0", dict(ldx=0)), ("ldx -1", dict(ldx=-1)), ("L 0", dict(L=0, ldo=0)),
                         ("L -1", dict(L=-1)), ("L 2^31", dict(L=1 << 31, ldo=1 << 31)), ("ldo < L", dict(ldo=7999)),
                         ("partner without lam", dict(lam=None)), ("partner without ws", dict(ws=None)), ("out == x", dict(out=p))):
        a = dict(good, **change)
        rows.append((what, (a["x"], a["B"], a["ldx"], a["len"], a["olen"], a["amp"], a["shift"], a["partner"], a["lam"], a["ws"], a["out"],
                            a["ldo"], a["L"], None), PA_EINVAL))
    return rows

"""Case builders, references and checkers for the device-impulse-response convolution (pa_ir_conv_plan, pa_ir_bank_prepare,
pa_wave_ir_convolve; passt_amd.augment.IRBank / WaveAugment(ir_augment=...)).  No device needed: tests/test_gpu_ir_conv.py runs the
checkers on the kernel's output, tests/test_ir_cases_cpu.py on a plain float32 numpy overlap-save and on wrong variants of it.

Truth is ``np.convolve`` in float64 of the float32 operands, cut or zero padded to L.  The error unit of clip b is
``u_b = 2**-24 * ||h_b||_2 * max|x_b|``.  The reference's own ``scipy.signal.convolve`` in float32 sits 13-14 u from that truth where
it picks its FFT method (10 s clips, 2000 and 8192 taps) and 3-5 u where it picks the direct method; a float32 overlap-save at 4096 /
16 384 points sits at 8-11 u.  The cap per element is therefore ``max(4 * the reference's own error on that clip, 48 u_b)``: the
reference's error is computed HERE with scipy and stored with the case (never taken from the code under test), the factor 4 covers
another tile size and butterfly order, the floor the clips where the reference runs the direct method, which an FFT cannot match."""
import ctypes

import numpy as np
import scipy.signal

PA_OK, PA_EINVAL = 0, -1
IR_MAX_TAPS = 8192
EPS = 2.0 ** -24
CAP_FACTOR, CAP_FLOOR = 4.0, 48.0
SENTINEL = 12345.0


# ---- geometry ------------------------------------------------------------------------------------------------------------------------
def plan(max_taps):
    """(fft_n, hop) of pa_ir_conv_plan, or None where it refuses"""
    from passt_amd import _lib
    n, hop = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = _lib.load().pa_ir_conv_plan(int(max_taps), ctypes.byref(n), ctypes.byref(hop))
    return (n.value, hop.value) if rc == PA_OK else None


def compiled_sizes():
    """{fft_n: largest max_taps that selects it}: one bank per compiled tile size, the one with the shortest hop"""
    sizes = {}
    for m in range(1, IR_MAX_TAPS + 1):
        sizes[plan(m)[0]] = m
    return sizes


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def graded_noise(rng, n):
    """white noise whose level climbs 40 dB over the clip and carries an offset: every tile has another scale"""
    return ((rng.standard_normal(n) * np.logspace(-2, 0, n) + 0.05) * 0.3).astype(np.float32)


def decaying_noise(rng, k):
    """noise under an exponential envelope (60 dB over the taps), a direct path of 1 in front: the shape of a room / device IR"""
    h = rng.standard_normal(k) * np.exp(-6.9 * np.arange(k) / max(k, 1))
    h[0] = 1.0
    return h.astype(np.float32)


def truth(x, h, L):
    """(float64 [L], len_out): np.convolve(x, h) in float64 cut or zero padded to L"""
    out = np.zeros(L, np.float64)
    if len(x) == 0:
        return out, 0
    full = np.convolve(x.astype(np.float64), h.astype(np.float64))
    m = min(len(full), L)
    out[:m] = full[:m]
    return out, m


def unit(x, h):
    return EPS * float(np.linalg.norm(h.astype(np.float64))) * float(np.abs(x).max() if len(x) else 0.0)


def reference_error(x, h, L, want):
    """max |scipy.signal.convolve(x, h, 'full') in float32, cut / padded to L, - truth|: the reference's own error on this clip"""
    full = scipy.signal.convolve(x, h, "full").astype(np.float32)
    got = np.zeros(L, np.float64)
    m = min(len(full), L)
    got[:m] = full[:m]
    return float(np.abs(got - want).max())


class Case:
    """B clips, each with its IR of one bank.  x [B][ldx] and irs [n_ir][max_taps] carry NaN behind the valid samples / taps."""

    def __init__(self, max_taps, taps, lens, ir_idx, L, seed, ldx_extra=13):
        rng = np.random.default_rng(seed)
        self.max_taps, self.L, self.B = int(max_taps), int(L), len(lens)
        self.fft_n, self.hop = plan(max_taps)
        self.taps = np.asarray(taps, np.int32)
        self.lens = np.asarray(lens, np.int32)
        self.ir_idx = np.asarray(ir_idx, np.int32)
        self.irs = np.full((len(taps), max_taps), np.nan, np.float32)
        for i, k in enumerate(taps):
            self.irs[i, :k] = decaying_noise(rng, k)
        self.ldx = int(max(lens)) + ldx_extra
        self.x = np.full((self.B, self.ldx), np.nan, np.float32)
        for b, n in enumerate(lens):
            self.x[b, :n] = graded_noise(rng, n)
        self.want = np.zeros((self.B, self.L), np.float64)
        self.len_out = np.zeros(self.B, np.int32)
        self.unit = np.zeros(self.B)
        self.ref_err = np.zeros(self.B)
        for b in range(self.B):
            xb = self.x[b, :self.lens[b]]
            if self.ir_idx[b] < 0:
                m = min(len(xb), self.L)
                self.want[b, :m], self.len_out[b] = xb[:m], m
                continue
            h = self.irs[self.ir_idx[b], :self.taps[self.ir_idx[b]]]
            self.want[b], self.len_out[b] = truth(xb, h, self.L)
            self.unit[b] = unit(xb, h)
            self.ref_err[b] = reference_error(xb, h, self.L, self.want[b])
        self.cap = np.maximum(CAP_FACTOR * self.ref_err, CAP_FLOOR * self.unit)


def operand_case(max_taps, seed=0):
    """six clips, six IRs of 1, 2, 3, an odd middle count, max_taps - 1 and max_taps taps; len_out = 1, hop - 1, hop, hop + 1,
    2 hop + 1 and one clip shorter than its IR"""
    _, hop = plan(max_taps)
    mid = (max_taps // 2) | 1
    taps = [1, 2, 3, mid, max_taps - 1, max_taps]
    len_out = [1, hop - 1, hop, hop + 1, 2 * hop + 1]
    lens = [lo - k + 1 for lo, k in zip(len_out, taps)] + [max(max_taps // 3, 1)]
    assert min(lens) >= 1 and lens[5] < taps[5]
    return Case(max_taps, taps, lens, range(6), L=2 * hop + 1 + 37, seed=seed)


def truncation_case(max_taps, seed=1):
    """L cuts inside the IR's tail (len + taps - 1 > L >= len) and inside the clip itself (len > L)"""
    _, hop = plan(max_taps)
    L = hop + 29
    taps = [max_taps, (max_taps // 2) | 1]
    lens = [L - 5, L + hop // 2 + 3]
    return Case(max_taps, taps, lens, [0, 1], L=L, seed=seed)


# ---- checkers: each returns the worst |error| / cap (values) or raises AssertionError ------------------------------------------------------
def check_values(out, case, rows=None):
    worst = 0.0
    for b in (range(case.B) if rows is None else rows):
        err = np.abs(out[b].astype(np.float64) - case.want[b])
        if case.ir_idx[b] < 0:
            assert err.max() == 0.0, f"clip {b}: a pass-through must be a bit-exact copy"
            continue
        k = int(err.argmax())
        assert err[k] <= case.cap[b], (f"clip {b} (taps {case.taps[case.ir_idx[b]]}, len {case.lens[b]}): |err| {err[k]:.3e} = "
                                       f"{err[k] / case.unit[b]:.1f} u at t = {k}, cap {case.cap[b] / case.unit[b]:.1f} u "
                                       f"(reference {case.ref_err[b] / case.unit[b]:.1f} u)")
        worst = max(worst, float(err[k] / case.cap[b]))
    return worst


def check_len_out(len_out, case):
    assert np.array_equal(np.asarray(len_out, np.int64), case.len_out.astype(np.int64)), (list(len_out), list(case.len_out))


def check_tail(out, case):
    """finite everywhere, exactly zero from len_out[b] to L"""
    assert np.isfinite(out).all(), "non-finite output: NaN padding of x or of the IR rows was read"
    for b in range(case.B):
        tail = out[b, case.len_out[b]:]
        assert not tail.any(), f"clip {b}: out[{case.len_out[b]}:{case.L}] must be zero, {np.count_nonzero(tail)} elements are not"


def check_all(out, len_out, case):
    check_len_out(len_out, case)
    check_tail(out, case)
    return check_values(out, case)


# ---- a plain float32 overlap-save, and wrong variants of it ------------------------------------------------------------------------------
FAULTS = ("hop_off_by_one", "tail_not_zeroed", "circular_wrap_kept", "neighbour_ir", "truncate_at_len")


def numpy_overlap_save(case, fault=None):
    """(out float32 [B][L], len_out): what the kernel computes, tile by tile, with numpy's float32 FFT (scipy.fft keeps float32)"""
    import scipy.fft
    n, hop = case.fft_n, case.hop
    out = np.zeros((case.B, case.L), np.float32)
    len_out = np.zeros(case.B, np.int32)
    for b in range(case.B):
        lb = int(case.lens[b])
        xb = case.x[b, :lb]
        ir = int(case.ir_idx[b])
        if ir < 0:
            m = min(lb, case.L)
            out[b, :m], len_out[b] = xb[:m], m
            continue
        if fault == "neighbour_ir":
            ir = int(case.ir_idx[(b + 1) % case.B])
        k = int(case.taps[ir])
        lo = min(lb + (0 if fault == "truncate_at_len" else k - 1), case.L)
        len_out[b] = min(lb + k - 1, case.L)
        hpad = np.zeros(n, np.float32)
        hpad[:k] = case.irs[ir, :k]
        H = scipy.fft.fft(hpad)
        assert H.dtype == np.complex64
        step = hop + 1 if fault == "hop_off_by_one" else hop
        for p in range(-(-case.L // hop)):
            o0 = p * step
            if o0 >= case.L:
                break
            w0 = o0 - (n - hop)
            win = np.zeros(n, np.float32)
            a, e = max(w0, 0), min(w0 + n, lb)
            if e > a:
                win[a - w0:e - w0] = xb[a:e]
            y = scipy.fft.ifft(scipy.fft.fft(win) * H).real.astype(np.float32)
            seg = y[n - hop:]
            if fault == "circular_wrap_kept":
                seg = y[n - hop - 1:n - 1]
            m = min(hop, case.L - o0)
            out[b, o0:o0 + m] = seg[:m]
        if fault == "tail_not_zeroed":
            out[b, lo:] += np.float32(1e-3)
        else:
            out[b, lo:] = 0
    return out, len_out


# ---- refusals: (what, entry, args, expected return) ------------------------------------------------------------------------------------------
def refusal_table(p):
    """`p`: any non-NULL 8-byte aligned address; none of these calls may launch, so it is never dereferenced"""
    rows = []
    for m in (0, -1, IR_MAX_TAPS + 1, 1 << 30):
        rows.append((f"plan max_taps {m}", "pa_ir_conv_plan", (m, None, None), PA_EINVAL))
    for m in (1, 1024, 1025, IR_MAX_TAPS):
        rows.append((f"plan max_taps {m}", "pa_ir_conv_plan", (m, None, None), PA_OK))
    # pa_ir_bank_prepare(irs, n_ir, ld_ir, ir_len, spectra, stream)
    good = dict(irs=p, n_ir=3, ld_ir=700, ir_len=p, spectra=p)
    for what, change in (("irs NULL", dict(irs=None)), ("spectra NULL", dict(spectra=None)), ("n_ir 0", dict(n_ir=0)),
                         ("n_ir -1", dict(n_ir=-1)), ("ld_ir 0", dict(ld_ir=0)), ("ld_ir 8193", dict(ld_ir=IR_MAX_TAPS + 1)),
                         ("spectra unaligned", dict(spectra=p + 4))):
        a = dict(good, **change)
        rows.append(("prepare " + what, "pa_ir_bank_prepare", (a["irs"], a["n_ir"], a["ld_ir"], a["ir_len"], a["spectra"], None), PA_EINVAL))
    # pa_wave_ir_convolve(x, B, ldx, len, ir_idx, spectra, ir_len, n_ir, max_taps, out, ldo, L, len_out, stream)
    good = dict(x=p, B=4, ldx=9000, len=p, ir_idx=p, spectra=p, ir_len=p, n_ir=3, max_taps=700, out=p, ldo=8000, L=8000, len_out=p)
    for what, change in (("x NULL", dict(x=None)), ("out NULL", dict(out=None)), ("spectra NULL", dict(spectra=None)),
                         ("B 0", dict(B=0)), ("B -2", dict(B=-2)), ("L 0", dict(L=0, ldo=0)), ("L -1", dict(L=-1)),
                         ("ldx 0", dict(ldx=0)), ("ldx -5", dict(ldx=-5)), ("n_ir 0", dict(n_ir=0)), ("n_ir -1", dict(n_ir=-1)),
                         ("ldo < L", dict(ldo=7999)), ("max_taps 0", dict(max_taps=0)), ("max_taps -1", dict(max_taps=-1)),
                         ("max_taps 8193", dict(max_taps=IR_MAX_TAPS + 1)), ("ir_idx without ir_len", dict(ir_len=None))):
        a = dict(good, **change)
        rows.append(("convolve " + what, "pa_wave_ir_convolve",
                     (a["x"], a["B"], a["ldx"], a["len"], a["ir_idx"], a["spectra"], a["ir_len"], a["n_ir"], a["max_taps"], a["out"], a["ldo"],
                      a["L"], a["len_out"], None), PA_EINVAL))
    return rows


# ---- the WaveAugment end-to-end case (tests/golden/make_golden_ir.py writes tests/golden/ir_augment.npz from it) ------------------------
IR_AUG_CASE = dict(seed=47, L=8000, lens=[8000, 3000, 9000, 5200], ir_taps=[5, 300, 700], ir_idx=[1, -1, 2, -1],
                   gain_db=[-3, 5, 0, -7], shift=[0, 17, -50, 33], partner=[-1, 2, -1, -1], lam=[0.5, 0.31, 0.5, 0.5])


def ir_aug_inputs(case=IR_AUG_CASE):
    """(raw clips, IRs): float32 arrays regenerated bit-exactly from the seed"""
    rng = np.random.default_rng(case["seed"])
    raws = [graded_noise(rng, n) for n in case["lens"]]
    irs = [decaying_noise(rng, k) for k in case["ir_taps"]]
    return raws, irs

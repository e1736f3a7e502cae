"""pa_wave_augment_varlen on the device: the cases and checkers of tests/wave_varlen_cases.py through the C ABI (the test owns the
guarded buffers), the equal-length case against pa_wave_augment, every refusal, row pitches past 2^31 elements, and
WaveAugment(..., ragged=True) end to end -- drawn parameters against oracle.wave_oracle clip by clip, and with an impulse-response bank
against float64 numpy.convolve plus the definition."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from passt_amd.augment import IRBank, WaveAugment  # noqa: E402
from tests import ir_cases as IC  # noqa: E402
from tests import wave_varlen_cases as WC  # noqa: E402

DEV = "cuda"


def dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype)).to(DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


class HipWave:
    """the HIP kernels behind the interface of WC.NumpyWave"""

    def operands(self, case):
        return (dev(case.lens, np.int32), dev(case.olen, np.int32), dev(case.amp, np.float32), dev(case.shift, np.int32),
                dev(case.partner, np.int32), dev(case.lam, np.float32))

    def wave_augment_varlen(self, xbuf, x_lo, obuf, o_lo, case):
        xd, od = dev(xbuf, np.float32), dev(obuf, np.float32)
        lens, olen, amp, shift, partner, lam = self.operands(case)
        ws = torch.full((2 * case.B,), float("nan"), device=DEV)
        rc = _lib.load().pa_wave_augment_varlen(xd.data_ptr() + 4 * x_lo, case.B, case.ldx, lens.data_ptr(), olen.data_ptr(), amp.data_ptr(),
                                                shift.data_ptr(), partner.data_ptr(), lam.data_ptr(), ws.data_ptr(),
                                                od.data_ptr() + 4 * o_lo, case.ldo, case.L, stream())
        assert rc == WC.PA_OK
        torch.cuda.synchronize()
        return xd.cpu().numpy(), od.cpu().numpy()

    def wave_augment(self, x, case):
        xd = dev(x, np.float32)
        lens, _, amp, shift, partner, lam = self.operands(case)
        out = torch.full((case.B, case.L), float("nan"), device=DEV)
        ws = torch.empty(case.B, device=DEV)
        rc = _lib.load().pa_wave_augment(xd.data_ptr(), case.B, case.ldx, lens.data_ptr(), amp.data_ptr(), shift.data_ptr(), partner.data_ptr(),
                                         lam.data_ptr(), ws.data_ptr(), out.data_ptr(), case.L, stream())
        assert rc == WC.PA_OK
        torch.cuda.synchronize()
        return out.cpu().numpy()


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.name)
def test_cases_against_the_definition(case):
    worst = WC.check_case(HipWave(), case)
    print(f"{case.name}: worst |error| / bound on the mixed rows {worst:.3f}")


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.name)
def test_cases_against_the_oracle_clip_by_clip(case):
    worst = WC.check_oracle(HipWave(), case)
    print(f"{case.name}: worst |error| against the oracle at L = n_b {worst:.3e} (cap {WC.ORACLE_CAP})")


def test_equal_lengths_against_the_fixed_entry():
    identical = WC.check_equal_lengths(HipWave())
    print(f"equal lengths: mixed rows bit-identical to pa_wave_augment: {identical}")


def test_null_arrays_copy_and_pad():
    """amp, shift, partner and len NULL: every row is its clip's first n_b samples, bit for bit, zeros behind"""
    case = WC.RAGGED
    x = np.nan_to_num(WC.truth(case)[0], nan=3.0)                    # len == NULL means ldx: the whole row is valid
    xd, olen = dev(x, np.float32), dev(case.olen, np.int32)
    out = torch.full((case.B, case.L), float("nan"), device=DEV)
    rc = _lib.load().pa_wave_augment_varlen(xd.data_ptr(), case.B, case.ldx, None, olen.data_ptr(), None, None, None, None, None,
                                            out.data_ptr(), case.L, case.L, stream())
    assert rc == WC.PA_OK
    got = out.cpu().numpy()
    for b, n in enumerate(case.olen):
        assert np.array_equal(got[b, :n], x[b, :n]) and not got[b, n:].any()


def test_refusals():
    buf = torch.zeros(16, device=DEV)
    lib = _lib.load()
    for what, args, want in WC.refusal_table(buf.data_ptr()):
        assert lib.pa_wave_augment_varlen(*args) == want, what
    torch.cuda.synchronize()


def test_row_pitches_past_2_31_elements():
    """ldx = ldo = 2^31 + 4: the second row starts past what 32 bits index; only the rows' first samples exist.  The result is the one
    the same operands give at a small pitch, bit for bit."""
    case = WC.EQUAL
    x = WC.truth(case)[0]
    B, L, pitch = 2, case.L, (1 << 31) + 4
    lens, olen, amp, shift = (dev(v[:B], t) for v, t in ((case.lens, np.int32), (case.olen, np.int32), (case.amp, np.float32),
                                                        (case.shift, np.int32)))
    partner, lam = dev([1, 0], np.int32), dev([0.3, 0.5], np.float32)
    lib = _lib.load()

    def call(xd, ldx, od, ldo):
        ws = torch.empty(2 * B, device=DEV)
        assert lib.pa_wave_augment_varlen(xd.data_ptr(), B, ldx, lens.data_ptr(), olen.data_ptr(), amp.data_ptr(), shift.data_ptr(),
                                          partner.data_ptr(), lam.data_ptr(), ws.data_ptr(), od.data_ptr(), ldo, L, stream()) == WC.PA_OK
        torch.cuda.synchronize()

    small_x, small_o = dev(x[:B], np.float32), torch.full((B, L), float("nan"), device=DEV)
    call(small_x, case.ldx, small_o, L)
    assert bool(torch.isfinite(small_o).all())
    big_x = torch.empty(pitch + case.ldx, device=DEV)
    big_o = torch.empty(pitch + L, device=DEV)
    for b in range(B):
        big_x[b * pitch:b * pitch + case.ldx] = small_x[b]
        big_o[b * pitch:b * pitch + L] = float("nan")
    call(big_x, pitch, big_o, pitch)
    for b in range(B):
        assert torch.equal(big_o[b * pitch:b * pitch + L], small_o[b])


def _rnd(n, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) * 2 - 1) * scale


def test_wave_augment_ragged_matches_the_oracle_clip_by_clip():
    """WaveAugment(ragged=True) with drawn parameters, four clips of 20 000 - 40 000 samples, a cap that cuts one: every row against the
    oracle run on the pair alone at L = n_b, under the fixed entry's cap; the generators end where the fixed call leaves them."""
    lens, cap = [31234, 20000, 40000, 27001], 36000
    raws = [(_rnd(n, 60 + i, 0.3) + 0.01 * i).numpy() for i, n in enumerate(lens)]
    x = np.full((4, 40000), np.nan, np.float32)
    for b, r in enumerate(raws):
        x[b, :len(r)] = r
    aug = WaveAugment(clip_samples=cap)
    torch.manual_seed(5)
    np.random.seed(5)
    fixed, tgt_f = aug(torch.from_numpy(np.nan_to_num(x)).to(DEV), torch.eye(4).to(DEV), torch.tensor(lens, dtype=torch.int32))
    after_fixed = (torch.get_rng_state().clone(), np.random.get_state())
    torch.manual_seed(5)
    np.random.seed(5)
    p = aug.draw(4)
    torch.manual_seed(5)
    np.random.seed(5)
    wave, tgt, n = aug(torch.from_numpy(x).to(DEV), torch.eye(4).to(DEV), lens, ragged=True)
    assert torch.equal(torch.get_rng_state(), after_fixed[0]) and all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), after_fixed[1]))
    assert n == [min(v, cap) for v in lens] and wave.shape == (4, 1, max(n)) and torch.equal(tgt, tgt_f)
    assert any(q >= 0 for q in p[2]) and any(q < 0 for q in p[2]), "the seed must draw mixed and unmixed rows"
    case = WC.Case("drawn", lens=tuple(lens), ldx=40000, clip_samples=cap, ldo=max(n) + 1, gain_db=tuple(int(v) for v in p[0]),
                   shift=tuple(int(v) for v in p[1]), partner=tuple(int(v) for v in p[2]), lam=tuple(float(v) for v in p[3]))
    got = wave[:, 0].cpu().numpy()
    assert np.isfinite(got).all()
    for b, ref in enumerate(WC.oracle_rows(x, case)):
        e = float(np.abs(got[b, :n[b]] - ref).max())
        print(f"row {b}: n {n[b]}, partner {case.partner[b]}, |error| against the oracle {e:.3e}")
        assert e < WC.ORACLE_CAP
        assert (got[b, n[b]:].view(np.int32) == 0).all()
    # the same arguments feed the next stage: lengths as a device tensor give the same batch
    torch.manual_seed(5)
    np.random.seed(5)
    again, _, n2 = aug(torch.from_numpy(x).to(DEV), None, torch.tensor(lens, dtype=torch.int32, device=DEV), ragged=True)
    assert n2 == n and torch.equal(again, wave)


def test_wave_augment_ragged_with_irs():
    """A bank of 3 and 300 taps, clips 0 and 2 hit, clip 1 not; row 0 mixed with the clip that was not hit, row 1 with a hit one.
    Truth: numpy.convolve in float64, cut at the batch's longest n_b as the module asks pa_wave_ir_convolve to, then the definition
    at each row's n_b.  Cap per row, as tests/test_gpu_ir_conv.py derives it for the fixed path: the convolution's cap
    (tests/ir_cases.py: max(CAP_FACTOR * the reference's own error, CAP_FLOOR * unit)) times the clip's gain; a mixed row carries w
    times its own and (1 - w) times its partner's, and twice that for the two mean-centrings; plus 4 * 2^-24 of the row's peak for
    pa_wave_augment_varlen's own roundings."""
    rng = np.random.default_rng(47)
    lens, cap = [5000, 3000, 4000], 4500
    raws = [IC.graded_noise(rng, k) for k in lens]
    irs = [IC.decaying_noise(rng, k) for k in (3, 300)]
    ir_idx, gain_db, shift, partner, lam = [1, -1, 0], [-3, 5, 2], [17, -4000, 33], [1, 2, -1], [0.31, 0.5, 1.0]
    x = np.full((3, 5003), np.nan, np.float32)
    for b, r in enumerate(raws):
        x[b, :len(r)] = r
    aug = WaveAugment(clip_samples=cap, ir_bank=IRBank(irs), ir_augment=0.5)
    params = (np.array(gain_db), np.array(shift), np.array(partner), np.array(lam, np.float32), np.array(ir_idx))
    wave, _, n = aug(torch.from_numpy(x).to(DEV), None, lens, params, ragged=True)
    L = max(n)
    assert n == [4500, 3000, 4000] and wave.shape == (3, 1, L)
    conv, conv_len, conv_cap = np.zeros((3, L)), [], np.zeros(3)
    for b in range(3):
        h = irs[ir_idx[b]] if ir_idx[b] >= 0 else np.ones(1, np.float32)
        conv[b], m = IC.truth(raws[b], h, L)
        conv_len.append(m)
        if ir_idx[b] >= 0:
            conv_cap[b] = max(IC.CAP_FACTOR * IC.reference_error(raws[b], h, L, conv[b]), IC.CAP_FLOOR * IC.unit(raws[b], h))
    case = WC.Case("irs", lens=tuple(lens), ldx=max(lens), clip_samples=cap, ldo=L + 1, gain_db=tuple(gain_db), shift=tuple(shift),
                   partner=tuple(partner), lam=tuple(lam)).with_lens(conv_len)           # len = len_out, olen = n
    assert case.olen == tuple(n) and case.lens == (4500, 3000, 4002)
    want = WC.definition(conv, case)[0]
    own = conv_cap * case.amp.astype(np.float64)
    got = wave[:, 0].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    for b in range(3):
        bound = own[b]
        if partner[b] >= 0:
            w = max(lam[b], 1.0 - lam[b])
            bound = 2.0 * (w * own[b] + (1.0 - w) * own[partner[b]])
        bound += 4 * IC.EPS * np.abs(want[b]).max()
        err = float(np.abs(got[b] - want[b]).max())
        print(f"row {b}: n {n[b]}, |error| {err:.3e}, cap {bound:.3e}")
        assert err <= bound, (b, err, bound)
        assert not got[b, n[b]:].any()

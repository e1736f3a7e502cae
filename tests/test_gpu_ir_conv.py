"""pa_ir_bank_prepare / pa_wave_ir_convolve on the device against float64 truth (tests/ir_cases.py holds the cases, the cap and the
checkers; the same checkers pass against a float32 numpy overlap-save in tests/test_ir_cases_cpu.py), through the C ABI where the test
must own the buffers (guards, bad device-side values) and through passt_amd.ops / passt_amd.augment otherwise.  Shapes come from
pa_ir_conv_plan, so they sit on the tile edges of whatever geometry is built.  The worst |error| / cap per group goes to
ir_conv_metrics.json in $PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib, ops  # noqa: E402
from tests import ir_cases as IC  # noqa: E402

DEV = "cuda"
I32 = torch.int32
_METRICS = {}


def record(group, ratio):
    _METRICS[group] = max(_METRICS.get(group, 0.0), float(ratio))
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_metrics")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "ir_conv_metrics.json"), "w") as f:
        json.dump({k: {"worst_err_over_cap": v} for k, v in _METRICS.items()}, f, indent=1, sort_keys=True)


SIZES = IC.compiled_sizes()                      # {fft_n: the largest max_taps that selects it}
_CASES = {}


def operand_case(n):
    if n not in _CASES:
        _CASES[n] = IC.operand_case(SIZES[n])
    return _CASES[n]


def dev_i32(a):
    return torch.as_tensor(np.asarray(a, np.int32)).to(DEV)


def prepare(case):
    return ops.ir_bank_prepare(torch.from_numpy(case.irs).to(DEV), dev_i32(case.taps))


def run(case, bank=None, L=None, rows=None, ir_idx=None):
    rows = list(range(case.B)) if rows is None else rows
    bank = prepare(case) if bank is None else bank
    x = torch.from_numpy(case.x[rows]).to(DEV)
    out, len_out = ops.wave_ir_convolve(x, case.L if L is None else L, dev_i32(case.lens[rows]),
                                        dev_i32(case.ir_idx[rows] if ir_idx is None else ir_idx), bank)
    torch.cuda.synchronize()
    return out.cpu().numpy(), len_out.cpu().numpy()


@pytest.mark.parametrize("n", sorted(SIZES))
def test_operands(n):
    """six clips with six IRs of 1 .. max_taps taps, len_out on every side of a tile edge: each element within the cap, len_out exact"""
    case = operand_case(n)
    out, len_out = run(case)
    worst = IC.check_all(out, len_out, case)
    print(f"fft_n {n} hop {case.hop}: worst |err| / cap {worst:.3f}; kernel error in u per clip "
          f"{[round(float(np.abs(out[b] - case.want[b]).max() / case.unit[b]), 1) for b in range(case.B)]}, reference "
          f"{[round(float(case.ref_err[b] / case.unit[b]), 1) for b in range(case.B)]}")
    record(f"operands_{n}", worst)


@pytest.mark.parametrize("n", sorted(SIZES))
def test_guards(n):
    """NaN behind every clip's samples and every IR's taps, out with ldo > L inside sentinel rows: finite output, zero tails, sentinels
    untouched"""
    case = operand_case(n)
    B, L, ldo = case.B, case.L, case.L + 19
    buf = torch.full((B + 2, ldo), IC.SENTINEL, device=DEV)
    bank = prepare(case)
    out, len_out = ops.wave_ir_convolve(torch.from_numpy(case.x).to(DEV), L, dev_i32(case.lens), dev_i32(case.ir_idx), bank,
                                        out=buf[1:B + 1, :L])
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    assert (full[0] == IC.SENTINEL).all() and (full[B + 1] == IC.SENTINEL).all() and (full[1:B + 1, L:] == IC.SENTINEL).all()
    record(f"guards_{n}", IC.check_all(full[1:B + 1, :L], len_out.cpu().numpy(), case))


@pytest.mark.parametrize("n", sorted(SIZES))
def test_truncation(n):
    """L inside the IR's tail and inside the clip: the first L samples of the un-truncated run, bit for bit"""
    case = IC.truncation_case(SIZES[n])
    bank = prepare(case)
    out, len_out = run(case, bank)
    record(f"truncation_{n}", IC.check_all(out, len_out, case))
    L_all = int(case.lens.max()) + case.max_taps + 5
    long, len_long = run(case, bank, L=L_all)
    assert list(len_long) == [int(l + k - 1) for l, k in zip(case.lens, case.taps)]
    assert np.array_equal(out, long[:, :case.L])


@pytest.mark.parametrize("n", sorted(SIZES))
def test_exact_facts(n):
    """what an FFT form still gives exactly: pass-through copies, zeros from zeros, a row independent of its slot and of the batch"""
    case = operand_case(n)
    bank = prepare(case)
    L = case.L
    # ir_idx = -1: the input, bit for bit, zeros behind
    out, len_out = run(case, bank, ir_idx=[-1] * case.B)
    for b in range(case.B):
        m = min(int(case.lens[b]), L)
        assert len_out[b] == m and np.array_equal(out[b, :m], case.x[b, :m]) and not out[b, m:].any()
    # an all-zero clip
    z, _ = ops.wave_ir_convolve(torch.zeros(2, L, device=DEV), L, None, dev_i32([5, 3]), bank)
    assert not z.any().item()
    # the same clip with the same IR in two slots of a batch, and alone
    rows, ir = [4, 1, 4, 0], [5, 1, 5, -1]
    both, _ = run(case, bank, rows=rows, ir_idx=ir)
    assert np.array_equal(both[0], both[2])
    alone, _ = run(case, bank, rows=[4], ir_idx=[5])
    assert np.array_equal(alone[0], both[0])


@pytest.mark.parametrize("n", sorted(SIZES))
def test_bad_device_side_values(n):
    """ir_idx >= n_ir and ir_len outside 1..max_taps in the DEVICE arrays: clamped, the row is a pass-through, nothing outside the
    buffers is touched.  `spectra` is allocated for twice the bank, so an index one bank too far would still read this allocation."""
    case = operand_case(n)
    lib = _lib.load()
    n_ir, m, B, L = len(case.taps), case.max_taps, case.B, case.L
    floats = lib.pa_ir_bank_floats(n_ir, m)
    spectra = torch.full((2 * floats,), float("nan"), device=DEV)
    irs = torch.from_numpy(case.irs).to(DEV)
    bad_len = case.taps.copy()
    bad_len[2], bad_len[4] = 0, m + 1                            # IRs 2 and 4 carry an impossible tap count
    ir_len = dev_i32(np.concatenate([bad_len, np.full(2 * n_ir, 7, np.int32)]))     # readable past n_ir as well
    st = torch.cuda.current_stream().cuda_stream
    assert lib.pa_ir_bank_prepare(irs.data_ptr(), n_ir, m, ir_len.data_ptr(), spectra.data_ptr(), st) == IC.PA_OK
    ir_idx = np.array([0, n_ir, 2, 2 * n_ir - 1, 4, n_ir + 1], np.int32)
    x = torch.from_numpy(case.x).to(DEV)
    ldo = L + 19
    buf = torch.full((B + 2, ldo), IC.SENTINEL, device=DEV)
    len_out = torch.full((B + 2,), -77, dtype=I32, device=DEV)
    lens_d, idx_d = dev_i32(case.lens), dev_i32(ir_idx)
    rc = lib.pa_wave_ir_convolve(x.data_ptr(), B, x.stride(0), lens_d.data_ptr(), idx_d.data_ptr(), spectra.data_ptr(),
                                 ir_len.data_ptr(), n_ir, m, buf[1].data_ptr(), ldo, L, len_out[1:].data_ptr(), st)
    assert rc == IC.PA_OK
    torch.cuda.synchronize()
    full, lo = buf.cpu().numpy(), len_out.cpu().numpy()
    assert (full[0] == IC.SENTINEL).all() and (full[B + 1] == IC.SENTINEL).all() and (full[1:B + 1, L:] == IC.SENTINEL).all()
    assert lo[0] == -77 and lo[B + 1] == -77
    for b in range(1, B):                                       # every clip but the first is a pass-through
        k = min(int(case.lens[b]), L)
        assert lo[1 + b] == k and np.array_equal(full[1 + b, :k], case.x[b, :k]) and not full[1 + b, k:L].any(), b
    assert lo[1] == case.len_out[0]
    IC.check_values(full[1:B + 1, :L], case, rows=[0])


def test_wave_augment_with_irs_matches_reference_pipeline():
    """WaveAugment(ir_bank, ir_augment) end to end against the outputs of the reference's own pydub_augment / pad_or_truncate / roll /
    MixupDataset bodies (tests/golden/ir_augment.npz, written by tests/golden/make_golden_ir.py).

    Cap per output row: |kernel - golden| <= |kernel - truth| + |golden - truth|.  The second term is the fixture's ref_err.  The first
    is the convolution's cap (tests/ir_cases.py) times the clip's gain; a mixed row carries w times its own and (1 - w) times its
    partner's, and twice that because each mean-centring subtracts a mean that is off by at most as much.  On top, pa_wave_augment's
    own rounding (gain, centring, mix: one rounding each): 4 * 2**-24 of the row's peak."""
    from passt_amd.augment import IRBank, WaveAugment
    c = IC.IR_AUG_CASE
    raws, irs = IC.ir_aug_inputs(c)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ir_augment.npz"))
    B, L, ldx = len(raws), c["L"], max(len(r) for r in raws)
    x = torch.zeros(B, ldx)
    for b, r in enumerate(raws):
        x[b, :len(r)] = torch.from_numpy(r)
    aug = WaveAugment(clip_samples=L, ir_bank=IRBank(irs), ir_augment=0.5)
    params = (np.array(c["gain_db"]), np.array(c["shift"]), np.array(c["partner"]), np.array(c["lam"], np.float32), np.array(c["ir_idx"]))
    wave, tgt = aug(x.to(DEV), torch.eye(B).to(DEV), torch.tensor([len(r) for r in raws], dtype=I32), params)
    assert wave.shape == (B, 1, L)
    got = wave[:, 0].cpu().numpy().astype(np.float64)
    conv_cap = np.zeros(B)
    for b in range(B):
        if c["ir_idx"][b] >= 0:
            h = irs[c["ir_idx"][b]]
            want, _ = IC.truth(raws[b], h, L)
            conv_cap[b] = max(IC.CAP_FACTOR * IC.reference_error(raws[b], h, L, want), IC.CAP_FLOOR * IC.unit(raws[b], h))
    own = conv_cap * 10.0 ** (np.array(c["gain_db"]) / 20.0)
    worst = 0.0
    for b in range(B):
        cap = own[b]
        if c["partner"][b] >= 0:
            w = max(c["lam"][b], 1.0 - c["lam"][b])
            cap = 2.0 * (w * own[b] + (1.0 - w) * own[c["partner"][b]])
        cap += g["ref_err"][b] + 4 * IC.EPS * np.abs(g["out"][b]).max()
        err = np.abs(got[b] - g["out"][b]).max()
        print(f"clip {b}: |err| {err:.3e}, cap {cap:.3e}")
        assert err <= cap, (b, err, cap)
        worst = max(worst, err / cap)
    record("wave_augment_ir", worst)
    assert float((tgt.cpu() - torch.from_numpy(g["target"])).abs().max()) < 1e-6
    # the 4-tuple form and a batch without a hit take today's path: the same as a WaveAugment without a bank
    plain, _ = WaveAugment(clip_samples=L)(x.to(DEV), None, torch.tensor([len(r) for r in raws], dtype=I32), params[:4])
    nohit, _ = aug(x.to(DEV), None, torch.tensor([len(r) for r in raws], dtype=I32), params[:4] + (np.full(B, -1),))
    four, _ = aug(x.to(DEV), None, torch.tensor([len(r) for r in raws], dtype=I32), params[:4])
    assert torch.equal(plain, nohit) and torch.equal(plain, four)


def test_draw_order():
    """the host draws of WaveAugment(ir_augment=...) in the reference's order (needs no device: tests/test_ir_cases_cpu.py holds it)"""
    from tests.test_ir_cases_cpu import test_draw_order as check
    check()

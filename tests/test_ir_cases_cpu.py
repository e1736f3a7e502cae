"""tests/ir_cases.py's checkers against a plain float32 numpy overlap-save (they must pass) and against five wrong variants of it (each
must be rejected); every PA_EINVAL refusal of pa_ir_conv_plan, pa_ir_bank_prepare and pa_wave_ir_convolve through the built library,
which launches nothing and therefore needs no device; the geometry pa_ir_conv_plan reports; the ABI's declarations; and the argument
errors of IRBank / WaveAugment."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import ir_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pa_ir_conv_plan", "pa_ir_bank_floats", "pa_ir_bank_prepare", "pa_wave_ir_convolve")


@pytest.fixture(scope="module")
def sizes():
    return IC.compiled_sizes()


@pytest.fixture(scope="module")
def cases(sizes):
    return {n: IC.operand_case(m) for n, m in sizes.items()}


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def test_plan_geometry(sizes):
    assert 1 <= len(sizes) <= 2, sizes                      # at most two compiled tile sizes
    prev_n = 0
    for m in range(1, IC.IR_MAX_TAPS + 1):
        n, hop = IC.plan(m)
        assert n >= prev_n, f"fft_n shrinks at max_taps {m}"
        prev_n = n
        eff = n - hop + 1                                   # the tap count the tile is laid out for
        assert hop >= 1 and eff >= m, (m, n, hop)
        assert n & (n - 1) == 0
    for n, m in sizes.items():
        assert (n + n // 16) * 4 * 2 <= 160 * 1024, "two workgroups' exchange buffers must fit one CU's LDS"
    assert IC.plan(0) is None and IC.plan(IC.IR_MAX_TAPS + 1) is None


def test_bank_floats():
    from passt_amd import _lib
    lib = _lib.load()
    for m in (1, 700, 1024, 1025, 8192):
        n, _ = IC.plan(m)
        assert lib.pa_ir_bank_floats(3, m) >= 3 * 2 * n
        assert lib.pa_ir_bank_floats(4, m) > lib.pa_ir_bank_floats(3, m)
    assert lib.pa_ir_bank_floats(0, 700) == 0 and lib.pa_ir_bank_floats(3, 0) == 0 and lib.pa_ir_bank_floats(3, 8193) == 0


# ---- the checkers accept an honest float32 overlap-save and reject wrong ones -------------------------------------------------------------
def test_checkers_accept_numpy_overlap_save(cases):
    for n, case in cases.items():
        out, len_out = IC.numpy_overlap_save(case)
        worst = IC.check_all(out, len_out, case)
        assert 0 < worst <= 1.0
        # the cap is the reference's: where scipy ran its FFT method the cap follows it, elsewhere the 48 u floor holds
        assert (case.cap >= IC.CAP_FLOOR * case.unit).all()


def test_checkers_accept_truncation_case(sizes):
    for n, m in sizes.items():
        case = IC.truncation_case(m)
        assert case.lens[0] + case.taps[0] - 1 > case.L >= case.lens[0] and case.lens[1] > case.L
        assert (case.len_out == case.L).all()
        IC.check_all(*IC.numpy_overlap_save(case), case)


@pytest.mark.parametrize("fault", IC.FAULTS)
def test_checkers_reject(cases, fault):
    for n, case in cases.items():
        out, len_out = IC.numpy_overlap_save(case, fault)
        with pytest.raises(AssertionError):
            IC.check_all(out, len_out, case)


def test_operand_case_reaches_the_tile_edges(cases):
    for n, case in cases.items():
        hop = case.hop
        assert list(case.len_out[:5]) == [1, hop - 1, hop, hop + 1, 2 * hop + 1]
        assert case.lens[5] < case.taps[5]
        assert list(case.taps[:3]) == [1, 2, 3] and case.taps[3] % 2 == 1 and list(case.taps[4:]) == [case.max_taps - 1, case.max_taps]
        assert np.isnan(case.x[:, -1]).all() and np.isnan(case.irs[0, 1:]).all()


def test_golden_case_is_what_the_fixture_holds():
    c = IC.IR_AUG_CASE
    g = np.load(os.path.join(ROOT, "tests", "golden", "ir_augment.npz"))
    assert g["out"].shape == (4, c["L"]) and g["out"].dtype == np.float32 and g["ref_err"].shape == (4,)
    assert sorted(g.files) == ["out", "ref_err", "target"]
    assert sum(i >= 0 for i in c["ir_idx"]) == 2 and c["ir_idx"][c["partner"][1]] >= 0
    assert np.isfinite(g["out"]).all() and (g["ref_err"] < 1e-5).all()


# ---- refusals through the built library: nothing is launched -------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from passt_amd import _lib
    lib = _lib.load()
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 15) & ~15
    rows = IC.refusal_table(base)
    assert len(rows) >= 27
    for what, entry, args, want in rows:
        assert getattr(lib, entry)(*args) == want, what


def test_abi_declares_the_entries():
    from passt_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    for e in ENTRIES:
        assert re.search(r"\b" + e + r"\(", hdr), e
        assert e in _lib.SIGNATURES, e
    assert "#define PA_IR_MAX_TAPS 8192" in hdr
    assert len(_lib.SIGNATURES["pa_wave_ir_convolve"][1]) == 14 and len(_lib.SIGNATURES["pa_ir_bank_prepare"][1]) == 6
    assert _lib.load().pa_abi_version() == 6


# ---- public interface ------------------------------------------------------------------------------------------------------------------------
def test_irbank_argument_errors():
    from passt_amd.augment import IRBank
    with pytest.raises(ValueError, match="empty"):
        IRBank([])
    with pytest.raises(ValueError, match="non-empty"):
        IRBank([np.ones(4, np.float32), np.zeros(0, np.float32)])
    with pytest.raises(ValueError, match="truncate"):
        IRBank([np.ones(8193, np.float32)])
    import torch
    bank = IRBank([np.ones(5), torch.ones(8192), [1.0, 2.0]])
    assert len(bank) == 3 and bank.max_taps == 8192 and list(bank.ir_len) == [5, 8192, 2]
    assert bank.irs.dtype == np.float32 and bank.irs.shape == (3, 8192) and bank.irs[2, 2:].sum() == 0


def test_waveaugment_argument_errors():
    from passt_amd.augment import IRBank, WaveAugment
    with pytest.raises(ValueError, match="ir_bank"):
        WaveAugment(ir_augment=0.5)
    with pytest.raises(ValueError, match="IRBank"):
        WaveAugment(ir_bank=[np.ones(3)], ir_augment=0.5)
    aug = WaveAugment(ir_bank=IRBank([np.ones(3)]), ir_augment=0.0)
    assert len(aug.draw(3)) == 4
    assert len(WaveAugment(ir_bank=IRBank([np.ones(3)]), ir_augment=0.25).draw(3)) == 5


def test_draw_order():
    """draw(B) consumes the host generators in the reference's per-item order: torch.rand(1) for the IR decision, np.random.randint(0,
    n_ir) only on a hit, torch.randint for the gain, np.random.randint for the roll; then the mixing draws.  With ir_augment = 0 the
    4-tuple and both generators' states afterwards are those of the sequence without the IR branch."""
    import torch
    from passt_amd.augment import IRBank, WaveAugment
    B, n_ir = 16, 3
    bank = IRBank([np.ones(k) for k in (4, 5, 6)])

    def replay(p):
        gain, shift, ir = np.zeros(B, np.int32), np.zeros(B, np.int32), np.full(B, -1, np.int32)
        for b in range(B):
            if p and float(torch.rand(1)) < p:
                ir[b] = int(np.random.randint(0, n_ir))
            gain[b] = int(torch.randint(14, (1,)).item()) - 7
            shift[b] = int(np.random.randint(-50, 51))
        partner, lam = np.full(B, -1, np.int32), np.ones(B, np.float32)
        for b in range(B):
            if float(torch.rand(1)) < 0.5:
                partner[b] = int(torch.randint(B, (1,)).item())
                lam[b] = np.random.beta(2.0, 2.0)
        return gain, shift, partner, lam, ir

    def seeded(fn):
        torch.manual_seed(123)
        np.random.seed(321)
        got = fn()
        return got, torch.get_rng_state(), np.random.get_state()[1].copy()

    for p in (0.5, 0.0):
        want, t_want, n_want = seeded(lambda: replay(p))
        got, t_got, n_got = seeded(lambda: WaveAugment(ir_bank=bank, ir_augment=p).draw(B))
        assert len(got) == (5 if p else 4)
        for a, w in zip(got, want):
            assert np.array_equal(a, w)
        assert torch.equal(t_got, t_want) and np.array_equal(n_got, n_want)
        if p:
            assert (got[4] >= 0).any() and (got[4] < 0).any() and got[4].max() < n_ir
    # without a bank at all: today's class, today's draws
    want, t_want, n_want = seeded(lambda: replay(0.0))
    got, t_got, n_got = seeded(lambda: WaveAugment().draw(B))
    assert len(got) == 4 and all(np.array_equal(a, w) for a, w in zip(got, want))
    assert torch.equal(t_got, t_want) and np.array_equal(n_got, n_want)

"""The 16x16x32 K loop of the role-split NT kernels on the CPU (tools/emulate_nt_mfma16.py: the kernel's address functions
transcribed): accumulator layout after the shuffle, bank conflicts of every fragment read, DMA placement against the reads --
and that the emulation notices what it is there to notice."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("emulate_nt_mfma16", os.path.join(ROOT, "tools", "emulate_nt_mfma16.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)


@pytest.mark.parametrize("TR", (False, True))
@pytest.mark.parametrize("TM", (2, 3, 4))
def test_layout_banks_placement(TM, TR):
    """(a) four MFMAs + swap == acc_row() / col = lane & 31 for every (register, lane); (b) every ds_read_b128 conflict-free;
    (c) every (row, k-chunk) read from where the DMA wrote it -- in the shipped four-pair form and the two-pair form"""
    for phases in (4, 2):
        assert E.check(TM, TR, phases) == 1


def test_the_shared_swizzle_would_conflict(monkeypatch):
    """with swz_f128 (the image the weight-gradient and attention kernels read transposed) the 16-row x 4-chunk reads are 2-way"""
    def swz_f128(row):
        y = (row >> 1) & 7
        return ((y & 1) << 2) | (y & 2) | (y >> 2)
    monkeypatch.setattr(E, "swz_nt128", swz_f128)
    with pytest.raises(AssertionError, match="2-way bank conflict"):
        E.check(3, False)


def test_the_other_swap_pairing_is_noticed(monkeypatch):
    """a v_permlane16_swap that exchanged the EVEN rows of X with the ODD rows of Y misplaces registers: (a) fails"""
    def other(x, y):
        x, y = x.copy(), y.copy()
        for base in (0, 32):
            lo, hi = slice(base, base + 16), slice(base + 16, base + 32)
            x[lo], y[hi] = y[hi].copy(), x[lo].copy()
        return x, y
    monkeypatch.setattr(E, "permlane16_swap", other)
    with pytest.raises(AssertionError):
        E.check(2, False)


def test_unpermuted_row_operand_is_noticed(monkeypatch):
    monkeypatch.setattr(E, "perm16", lambda x: x)
    with pytest.raises(AssertionError):
        E.check(2, True)


def test_emulation_matches_the_kernel_source():
    """the transcribed formulas are the ones in the sources (a change there must be made here too)"""
    mma = open(os.path.join(ROOT, "passt_amd", "csrc", "pa_mma.h")).read()
    gemm = open(os.path.join(ROOT, "passt_amd", "csrc", "gemm.hip")).read()
    assert "int swz_nt128(int row) { return (row >> 1) & 7; }" in mma
    assert "int perm16(int x) { return (x & 3) | ((x & 4) << 1) | ((x & 8) >> 1); }" in mma
    flat = re.sub(r"\s+", " ", gemm)
    assert "offA16[s] = (wr * (TM * 32) + rA16) * 128 + (((4 * s + (lane >> 4)) ^ swz_nt128(rA16)) << 4);" in flat
    assert "offB16[s] = (wc * 64 + rB16) * 128 + (((4 * s + (lane >> 4)) ^ swz_nt128(rB16)) << 4);" in flat
    assert "rA16 = TR ? (lane & 15) : perm16(lane & 15), rB16 = TR ? perm16(lane & 15) : (lane & 15);" in flat
    assert flat.count("const int c = (q & 7) ^ nt_swz<T>(row);") == 2

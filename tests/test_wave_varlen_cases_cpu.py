"""The checkers of tests/wave_varlen_cases.py without a device: they pass on the plain float32 numpy restatement (against the float64
definition and against oracle.wave_oracle run clip by clip), they reject every fault model; WaveAugment(..., ragged=True) refuses what
it must before it draws, and draws what the fixed call draws; the built library exports pa_wave_augment_varlen with the header's
signature and refuses every bad argument without a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from passt_amd import _lib, augment
from passt_amd.augment import WaveAugment
from tests import wave_varlen_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.name)
def test_numpy_restatement_passes(case):
    worst = WC.check_case(WC.NumpyWave(), case)
    print(f"{case.name}: worst |error| / bound on the mixed rows {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.name)
def test_numpy_restatement_matches_the_oracle_clip_by_clip(case):
    worst = WC.check_oracle(WC.NumpyWave(), case)
    print(f"{case.name}: worst |error| against the oracle at L = n_b {worst:.3e} (cap {WC.ORACLE_CAP})")


def test_equal_lengths_against_the_fixed_form():
    assert WC.check_equal_lengths(WC.NumpyWave()) is True


def test_the_truth_is_the_oracle_pair_at_its_own_length():
    """the float64 definition against the oracle, row by row: the definition itself is what the oracle gives for (b, p) at L = n_b"""
    for case in WC.CASES:
        x, want, _, exact = WC.truth(case)
        for b, ref in enumerate(WC.oracle_rows(x, case)):
            n = case.olen[b]
            assert float(np.abs(want[b, :n] - ref).max()) < WC.ORACLE_CAP
            if case.partner[b] < 0:
                assert np.array_equal(exact[b, :n], ref)
            assert not want[b, n:].any()


@pytest.mark.parametrize("fault", WC.FAULTS, ids=lambda f: f.__name__)
def test_fault_models_are_rejected(fault):
    with pytest.raises(AssertionError):
        WC.check_case(fault(), WC.RAGGED)


def test_cases_cover_what_they_claim():
    r = WC.RAGGED
    rel = {"longer": False, "shorter": False, "self": False, "mixed partner": False, "unmixed partner": False, "unmixed": False}
    for b, p in enumerate(r.partner):
        if p < 0:
            rel["unmixed"] = True
            continue
        rel["longer"] |= r.lens[p] > r.olen[b]
        rel["shorter"] |= r.lens[p] < r.olen[b]
        rel["self"] |= p == b
        rel["mixed partner"] |= r.partner[p] >= 0 and p != b
        rel["unmixed partner"] |= r.partner[p] < 0
    assert all(rel.values()), rel
    assert any(n < l for n, l in zip(r.olen, r.lens))                           # the cap cuts a clip
    assert all(n == WC.EQUAL.L for n in WC.EQUAL.olen) and any(p >= 0 and p != b for b, p in enumerate(WC.EQUAL.partner))
    assert (WC.SKEW.ldo - WC.SKEW.L) % 4 and WC.SKEW.o_off % 4
    shifts = set()
    for c in WC.CASES:
        for n, s in zip(c.olen, c.shift):
            shifts |= {k for k, v in (("0", 0), ("1", 1), ("-1", -1), ("n-1", n - 1), ("n", n), ("n+7", n + 7), ("-(2n+3)", -(2 * n + 3)),
                                      ("50", 50)) if v == s}
        assert set(np.float32(c.lam).tolist()) <= set(np.float32([0, 1, 0.5, 0.3]).tolist())
        assert all(-7 <= g <= 6 for g in c.gain_db)
    assert shifts == {"0", "1", "-1", "n-1", "n", "n+7", "-(2n+3)", "50"}, shifts


# ---- WaveAugment(..., ragged=True) on the host -------------------------------------------------------------------------------------------
def _states():
    return torch.get_rng_state().clone(), np.random.get_state()


def _same_states(before):
    after = _states()
    return torch.equal(before[0], after[0]) and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))


@pytest.mark.parametrize("what, lengths", [
    ("no lengths", None), ("too few", [100, 200, 300]), ("too many", [100, 200, 300, 400, 500]), ("zero", [100, 0, 300, 400]),
    ("negative", [100, 200, -5, 400]), ("longer than the row", [100, 200, 300, 501]), ("a tensor, too few", torch.tensor([100, 200])),
    ("a tensor, zero", torch.tensor([0, 1, 2, 3], dtype=torch.int32))])
def test_ragged_refusals_draw_nothing(what, lengths):
    torch.manual_seed(3)
    np.random.seed(3)
    aug = WaveAugment(clip_samples=400)
    raw = torch.full((4, 500), 7.0)
    keep = raw.clone()
    before = _states()
    with pytest.raises(ValueError):
        aug(raw, torch.eye(4), lengths, ragged=True)
    assert _same_states(before), f"{what}: a refusal consumed random numbers"
    assert torch.equal(raw, keep)


class _Recorder:
    """stands in for passt_amd.ops inside passt_amd.augment: records what the launches would be given"""

    def __init__(self):
        self.calls = []

    def wave_augment(self, raw, L, lengths, amp, sh, pt, lm):
        self.calls.append(("fixed", L, lengths, amp, sh, pt, lm))
        return torch.zeros(raw.shape[0], L)

    def wave_augment_varlen(self, raw, L, lengths, out_lengths, amp, sh, pt, lm):
        self.calls.append(("ragged", L, lengths, amp, sh, pt, lm, out_lengths))
        return torch.zeros(raw.shape[0], L)

    def mixup(self, target, perm, w):
        self.calls.append(("mixup", perm, w))
        return target


def test_ragged_call_draws_what_the_fixed_call_draws(monkeypatch):
    lens = [300, 77, 500, 412, 1]
    raw = torch.zeros(5, 500)
    aug = WaveAugment(clip_samples=400)
    runs = []
    for ragged in (False, True):
        rec = _Recorder()
        monkeypatch.setattr(augment, "ops", rec)
        torch.manual_seed(11)
        np.random.seed(11)
        res = aug(raw, torch.eye(5), lens, ragged=True) if ragged else aug(raw, torch.eye(5), torch.tensor(lens))
        runs.append((rec.calls, _states(), res))
    (fixed, st_f, res_f), (ragged, st_r, res_r) = runs
    assert torch.equal(st_f[0], st_r[0]) and all(np.array_equal(a, b) for a, b in zip(st_f[1], st_r[1]))
    assert [c[0] for c in fixed] == ["fixed", "mixup"] and [c[0] for c in ragged] == ["ragged", "mixup"]
    for a, b in zip(fixed[0][3:7], ragged[0][3:7]):                            # amp, shift, partner, lam
        assert torch.equal(a, b)
    assert torch.equal(fixed[1][1], ragged[1][1]) and torch.equal(fixed[1][2], ragged[1][2])
    # the geometry: nothing padded, the cap cuts, n is a list of ints
    n = [300, 77, 400, 400, 1]
    assert len(res_f) == 2 and len(res_r) == 3 and res_r[2] == n and all(type(v) is int for v in res_r[2])
    assert res_r[0].shape == (5, 1, 400) and ragged[0][1] == 400
    assert ragged[0][2].tolist() == lens and ragged[0][7].tolist() == n and ragged[0][7].dtype == torch.int32
    # lengths as a tensor give the same call
    rec = _Recorder()
    monkeypatch.setattr(augment, "ops", rec)
    assert aug(raw, None, torch.tensor(lens), ragged=True)[2] == n


# ---- the built library ---------------------------------------------------------------------------------------------------------------
def test_symbol_and_signature():
    assert "pa_wave_augment_varlen" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "pa_wave_augment_varlen") and lib.pa_abi_version() == 6           # additive: the version stays
    header = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    decl = re.search(r"int\s+pa_wave_augment_varlen\s*\(([^)]*)\)\s*;", header)
    assert decl, "include/passt_amd.h does not declare pa_wave_augment_varlen"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    res, args = _lib.SIGNATURES["pa_wave_augment_varlen"]
    assert res is _lib.i32 and len(params) == len(args) == 14
    want = {"int": _lib.i32, "int64_t": _lib.i64}
    for p, a in zip(params, args):
        assert a is (_lib.vp if "*" in p else want[p.split()[0]]), (p, a)
    assert params[4] == "const int32_t* olen" and params[11:13] == ["int64_t ldo", "int64_t L"]


def test_refusals_launch_nothing():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for what, args, want in WC.refusal_table(p):
        assert lib.pa_wave_augment_varlen(*args) == want, what

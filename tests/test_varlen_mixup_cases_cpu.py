"""CPU tests of the ragged spectrogram mixup and of the host side of ``TrainStep.step(..., lengths=)``: the checkers of
tests/varlen_mixup_cases.py accept a plain-torch restatement of the definition and reject the fault models a kernel of this kind can
have; the C ABI addition (exported, declared, its refusals without a device); the documented order of the step's host draws; a
refusal that leaves both generators where they were."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from passt_amd import _lib
from passt_amd.passt import draw_patchout
from tests import varlen_mixup_cases as M
from tests.varlen_mixup_cases import TorchMixup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMPL = TorchMixup()
PA_EINVAL = -1


# ---- the checkers and the honest restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_restatement_passes(case):
    worst = M.check_case(IMPL, case)
    assert worst <= 1.0


@pytest.mark.parametrize("case", M.FULL_CASES, ids=[c.id for c in M.FULL_CASES])
def test_full_lengths_are_the_fixed_mixup(case):
    M.check_full(IMPL, case)


def test_case_list_holds_what_it_claims():
    assert {c.ldt for c in M.CASES} == {40, 37} and {c.family for c in M.CASES} == {"exact", "graded"}
    assert any(c.offset for c in M.CASES if c.ldt % 4 == 0)                    # 4-byte accesses chosen by the pointers
    assert any(c.ldt % 4 and (c.rows * c.ldt) % 4 == 0 for c in M.CASES)        # 16-byte groups over the rows' ends
    assert all((c.rows * c.ldt) % 4 for c in M.CASES if c.ldt % 4 and c.rows == M.ROWS)     # ... and the scalar pitch stays scalar
    for ldt in M.LDTS:
        lens = M.lengths(ldt)
        assert lens == (1, ldt, 18, 5) and 18 % 4 and 5 % 4                       # both inside a 16-byte group
        pairs = {(lens[i], lens[j]) for p in M.PERMS.values() for i, j in enumerate(p)}
        assert (1, ldt) in pairs                                                  # the full-length clip as partner of the 1-frame clip
        assert any(a < b for a, b in pairs) and any(a > b for a, b in pairs)      # a longer and a shorter partner
    assert any(i == j for p in M.PERMS.values() for i, j in enumerate(p))         # a clip with itself
    assert all(sorted(p) == list(range(M.B)) for p in M.PERMS.values())
    x, lens, perm, lam, pad = M.operands(M.CASES[0])
    for i, n in enumerate(lens.tolist()):
        assert bool(torch.isnan(x[i, :, n:]).all()) and bool(torch.isfinite(x[i, :, :n]).all())
    assert set(M.EXACT_LAM) == {0.5, 0.75, 1.0} and M.EXACT_PAD == -3.0
    from passt_amd import train
    assert train.MIXUP_PAD == M.DEFAULT_PAD and abs(M.DEFAULT_PAD - (np.log(1e-5) + 4.5) / 5) < 1e-7
    assert np.float32(M.DEFAULT_PAD) == M.DEFAULT_PAD                             # one float32 constant


# ---- fault models ------------------------------------------------------------------------------------------------------------------
class PartnerNotCut(TorchMixup):
    def partner(self, x, perm, t, nj, pad):
        return x[perm.long()]


class PadIgnored(TorchMixup):
    def partner(self, x, perm, t, nj, pad):
        return super().partner(x, perm, t, nj, 0.0)


class TailUnwritten(TorchMixup):
    def tail(self, mix, t, ni, out):
        return torch.where(t < ni, mix, out)


class TailMultiplied(TorchMixup):
    def tail(self, mix, t, ni, out):
        return mix * (t < ni).float()


class PartnerByInversePermutation(TorchMixup):
    """perm on the wrong operand, first form: out[perm[i]] mixes in x[i] (a scatter where a gather is meant)"""

    def partner(self, x, perm, t, nj, pad):
        inv = torch.empty_like(perm)
        inv[perm.long()] = torch.arange(perm.numel(), dtype=perm.dtype)
        lens = torch.empty_like(nj)
        lens[perm.long()] = nj                       # nj[i] = lens[perm[i]]; the lengths follow the partner actually read
        return torch.where(t < lens[inv.long()], x[inv.long()], torch.full((), pad, dtype=torch.float32))


class LamOfThePartner(TorchMixup):
    """perm on the wrong operand, second form: lam[perm[i]] where lam[i] is meant"""

    def mixup_varlen(self, xbuf, x_lo, obuf, o_lo, shape, lens, perm, lam, pad):
        return super().mixup_varlen(xbuf, x_lo, obuf, o_lo, shape, lens, perm, lam[perm.long()], pad)


class LamSwapped(TorchMixup):
    def mix(self, a, c, l):
        return a * (1.0 - l) + c * l


class GroupByFirstLane(TorchMixup):
    """a whole 16-byte group decided by its first lane (rows of a multiple of four elements only)"""

    def partner(self, x, perm, t, nj, pad):
        return super().partner(x, perm, t - t % 4 if x.shape[-1] % 4 == 0 else t, nj, pad)

    def tail(self, mix, t, ni, out):
        return super().tail(mix, t - t % 4 if mix.shape[-1] % 4 == 0 else t, ni, out)


class RowEndNotWrapped(TorchMixup):
    """a 16-byte group that runs over a row's end (a clip of a multiple of four floats whose rows are not): the lanes in the next
    row are taken for columns ldt.. of the row the group began in, i.e. for cells behind every length"""

    def _t(self, t, shape):
        rows, ldt = shape[-2], shape[-1]
        if ldt % 4 == 0 or (rows * ldt) % 4:
            return t
        flat = torch.arange(rows)[None, :, None] * ldt + t
        return torch.where((flat - flat % 4) // ldt == torch.arange(rows)[None, :, None], t.expand(1, rows, ldt), torch.full((), ldt))

    def partner(self, x, perm, t, nj, pad):
        return super().partner(x, perm, self._t(t, x.shape), nj, pad)

    def tail(self, mix, t, ni, out):
        return super().tail(mix, self._t(t, mix.shape), ni, out)


FAULTS = (PartnerNotCut, PadIgnored, TailUnwritten, TailMultiplied, PartnerByInversePermutation, LamOfThePartner, LamSwapped,
          GroupByFirstLane, RowEndNotWrapped)


@pytest.mark.parametrize("cls", FAULTS, ids=[c.__name__ for c in FAULTS])
def test_fault_model_is_rejected(cls):
    caught = []
    for case in M.CASES:
        try:
            M.check_case(cls(), case)
        except AssertionError:
            caught.append(case.id)
    assert caught, f"{cls.__name__}: no case of the list sees it"
    print(cls.__name__, "rejected by", len(caught), "of", len(M.CASES), "cases")


def test_every_family_and_pitch_rejects_a_swapped_lam_and_only_the_vector_pitch_the_group_fault():
    for case in M.CASES:
        if case.perm != "self":                       # (under "self" two clips mix with themselves: lam does not matter there)
            with pytest.raises(AssertionError):
                M.check_case(LamSwapped(), case)
    for case in M.CASES:
        if case.ldt % 4:
            M.check_case(GroupByFirstLane(), case)      # nothing to get wrong on the scalar pitch
        else:
            with pytest.raises(AssertionError):
                M.check_case(GroupByFirstLane(), case)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_declared():
    assert "pa_mixup_varlen" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "pa_mixup_varlen") and lib.pa_abi_version() == 6            # additive: the version stays
    header = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    decl = re.search(r"int\s+pa_mixup_varlen\s*\(([^)]*)\)\s*;", header)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(_lib.SIGNATURES["pa_mixup_varlen"][1]) == 10
    assert params[4] == "float pad" and _lib.SIGNATURES["pa_mixup_varlen"][1][4] is _lib.f32
    from passt_amd import ops
    assert callable(ops.mixup_varlen)


def test_refusals_launch_nothing():
    """every PA_EINVAL of the header, on host addresses the library never dereferences: no device is needed, nothing is launched"""
    lib = _lib.load()
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 15) & ~15
    x, lens, perm, lam, out = base, base + 512, base + 1024, base + 1536, base + 2048
    ok = dict(x=x, lens=lens, perm=perm, lam=lam, pad=-1.0, out=out, B=4, rows=3, ldt=40)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pa_mixup_varlen(a["x"], a["lens"], a["perm"], a["lam"], a["pad"], a["out"], a["B"], a["rows"], a["ldt"], None)
    for name in ("x", "lens", "perm", "lam", "out"):
        assert call(**{name: None}) == PA_EINVAL, name
    for name in ("B", "rows", "ldt"):
        assert call(**{name: 0}) == PA_EINVAL and call(**{name: -1}) == PA_EINVAL, name
    assert call(out=x) == PA_EINVAL                                                  # the partner's row is read while others are written
    assert call(rows=1 << 16, ldt=1 << 15) == PA_EINVAL                              # one clip is indexed with 32 bits
    assert bytes(raw) == bytes(4096)


# ---- the host draws of a ragged step ---------------------------------------------------------------------------------------------
def _net(**patchout):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 256), stride=10, num_classes=5, embed_dim=64, depth=1, num_heads=1, distilled=True, **patchout)
    return net.train()


def _mel():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.AugmentMelSTFT(n_mels=128, sr=32000, win_length=800, hopsize=320, n_fft=1024, freqm=48, timem=20, fmin=0.0, fmax=None,
                                     fmin_aug_range=10, fmax_aug_range=2000)
    return m.train()


def test_host_draw_order_of_a_ragged_step_is_the_documented_one():
    """[varlen_clip_draws; randperm; beta; varlen_geometry_train] against the same sequence spelled with the raw RNG calls: per clip
    randint, randint, rand x 2 (frequency band), rand x 2 (time band); then randperm(B) and numpy's beta; then per clip the Patchout
    calls of the fixed path.  The same values and the same final state of both generators -- and another order gives other values."""
    mel, net = _mel(), _net(s_patchout_t=2, s_patchout_f=3, u_patchout=7)
    samples, alpha = [16000, 48000, 33000], 0.3
    frames = [1 + (n - 1) // 320 for n in samples]
    torch.manual_seed(31)
    np.random.seed(31)
    d = M.host_draws(mel, net, samples, alpha)
    state_t, state_n = torch.get_rng_state(), np.random.get_state()
    assert d["frames"] == frames

    torch.manual_seed(31)
    np.random.seed(31)
    for i, T in enumerate(frames):
        fmin = mel.fmin + torch.randint(10, (1,)).item()
        fmax = mel.fmax + 1000 - torch.randint(2000, (1,)).item()
        v = torch.rand(1) * 48
        s = int((torch.rand(1) * (128 - v)).long())
        fm = (s, s + int(v.long()))
        v = torch.rand(1) * 20
        s = int((torch.rand(1) * (T - v)).long())
        tm = (s, s + int(v.long()))
        assert (d["front"]["fmin"][i], d["front"]["fmax"][i], d["front"]["fmask"][i], d["front"]["tmask"][i]) == (fmin, fmax, fm, tm), i
    perm = torch.randperm(3)
    lam = np.random.beta(alpha, alpha, 3).astype(np.float32)
    assert torch.equal(perm, d["perm"]) and np.array_equal(np.maximum(lam, 1 - lam), d["lam"])
    toffs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for T in frames:
            toffs.append(draw_patchout(net, 12, (T - 16) // 10 + 1)[0])
    assert toffs == d["geometry"]["toff"].tolist()
    assert torch.equal(torch.get_rng_state(), state_t)
    sn = np.random.get_state()
    assert sn[0] == state_n[0] and np.array_equal(sn[1], state_n[1]) and sn[2:] == state_n[2:]

    # the order is observable: with the permutation drawn first the same seed gives other draws
    from passt_amd.preprocess import varlen_clip_draws
    torch.manual_seed(31)
    p2 = torch.randperm(3)
    f2 = varlen_clip_draws(mel, samples)
    assert (p2.tolist(), f2["fmin"], f2["fmax"], f2["fmask"]) != (d["perm"].tolist(), d["front"]["fmin"], d["front"]["fmax"], d["front"]["fmask"])


def test_a_refused_batch_consumes_no_random_number():
    """the factored Patchout check: the ValueErrors of varlen_geometry_train, with both generators untouched"""
    from passt_amd.passt import check_patchout_varlen, varlen_geometry_train
    net = _net(s_patchout_t=2, s_patchout_f=3)
    torch.manual_seed(5)
    np.random.seed(5)
    state_t, state_n = torch.get_rng_state(), np.random.get_state()
    msgs = []
    for fn in (check_patchout_varlen, varlen_geometry_train):
        with pytest.raises(ValueError, match="clip 1:") as e:
            fn(net, [106, 26])                                   # 2 patch columns, s_patchout_t = 2
        msgs.append(str(e.value))
        with pytest.raises(ValueError, match="clip 0: 12 frames are shorter than one patch"):
            fn(net, [12, 106])
        with pytest.raises(ValueError, match="exceeds the input's 100 frames"):
            fn(net, [56, 106], T_max=100)
    assert msgs[0] == msgs[1]
    assert torch.equal(torch.get_rng_state(), state_t)
    sn = np.random.get_state()
    assert sn[0] == state_n[0] and np.array_equal(sn[1], state_n[1]) and sn[2:] == state_n[2:]
    # what it returns for a batch that passes: patch columns per clip and the clips the time embedding cuts
    assert check_patchout_varlen(net.eval(), [16, 56, 300]) == ([1, 5, 29], [2])
    assert torch.equal(torch.get_rng_state(), state_t)

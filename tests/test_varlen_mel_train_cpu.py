"""CPU tests of the training-mode front end on ragged batches (``mel.varlen_train = True``): the host draws and their RNG order against
the reference's recorded draws (tests/golden/varlen_mel_train.npz) and against the oracle's clip-by-clip loop, the calls that are
rejected before any draw, the fixture, the C ABI additions, the public switch."""
import copy
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from oracle import ref_import
from oracle import passt_oracle as O
from passt_amd import _lib
from passt_amd._lib import PasstAmdError
from passt_amd.preprocess import varlen_clip_draws
from tests.golden import make_varlen_mel_train_golden as MT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pa_mel_frontend_fwd_varlen_aug", "pa_mel_frontend_bwd_varlen_aug")
FIELDS = (("mel_low", "float"), ("inv_mel_delta", "float"), ("fmask_start", "int32_t"), ("fmask_end", "int32_t"),
          ("tmask_start", "int32_t"), ("tmask_end", "int32_t"))


def _mel(train=True, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.AugmentMelSTFT(**dict(MT.MEL_KW, **kw))
    return m.train(train)


def _table_rows(table):
    return [(c.mel_low, c.inv_mel_delta, c.fmask_start, c.fmask_end, c.tmask_start, c.tmask_end) for c in table]


def test_draws_reproduce_the_reference_draws_of_the_fixture(golden_dir):
    gold = np.load(os.path.join(golden_dir, "varlen_mel_train.npz"))
    torch.manual_seed(MT.TORCH_SEED)
    d = varlen_clip_draws(_mel(), MT.LENGTHS)
    assert np.array_equal(torch.get_rng_state().numpy(), gold["rng"])           # the generator ends where the reference's loop left it
    assert d["frames"] == gold["frames"].tolist()
    f32 = lambda v: C.c_float(v).value                                          # noqa: E731
    for i in range(len(MT.LENGTHS)):
        fmin, fmax, fs, fe, ts, te = gold[f"draw.{i}"].tolist()
        assert (d["fmin"][i], d["fmax"][i], *d["fmask"][i], *d["tmask"][i]) == (fmin, fmax, fs, fe, ts, te), i
        lo, hi = 1127.0 * np.log1p(fmin / 700.0), 1127.0 * np.log1p(fmax / 700.0)
        row = _table_rows(d["table"])[i]
        assert row[2:] == (fs, fe, ts, te) and row[0] == f32(lo) and row[1] == f32(129 / (hi - lo)), i
    MT.check_draws([gold[f"draw.{i}"] for i in range(len(MT.LENGTHS))])          # the fixture shows what it is there to show
    assert gold["draw.3"][4] < 0 and gold["draw.3"][5] >= 2                      # 2 frames: negative start, band over the whole clip


@pytest.mark.parametrize("kw", [dict(), dict(freqm=0), dict(timem=0), dict(freqm=0, timem=0)])
def test_generator_ends_where_the_clip_by_clip_oracle_loop_leaves_it(kw):
    lengths = [3000, 640, 5120]
    m = _mel(**kw)
    torch.manual_seed(77)
    d = varlen_clip_draws(m, lengths)
    state = torch.get_rng_state()
    torch.manual_seed(77)
    aux = []
    for n in lengths:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            aux.append(O.mel_frontend(torch.zeros(1, n), training=True, return_aux=True, **dict(MT.MEL_KW, **kw))[1])
    assert torch.equal(torch.get_rng_state(), state)
    assert d["fmin"] == [a["fmin"] for a in aux] and d["fmax"] == [a["fmax"] for a in aux]
    # skipped draws leave an empty band; the draws that are made are the reference's calls in its order
    torch.manual_seed(77)
    for i, n in enumerate(lengths):
        torch.randint(10, (1,)), torch.randint(2000, (1,))
        fm = O.draw_mask_params(kw.get("freqm", MT.MEL_KW["freqm"]), 128)
        tm = O.draw_mask_params(kw.get("timem", MT.MEL_KW["timem"]), MT.frames_of(n))
        assert d["fmask"][i] == fm and d["tmask"][i] == tm, i
    if kw.get("freqm") == 0:
        assert all(b == (0, 0) for b in d["fmask"])
    if kw.get("timem") == 0:
        assert all(b == (0, 0) for b in d["tmask"])


def test_eval_settings_do_not_matter_to_the_draw_function_and_the_time_band_uses_the_clips_own_frames():
    """a band drawn against 2 frames with timem = 40 starts at or below 0; against 150 frames it cannot end behind 150"""
    m = _mel()
    for seed in range(20):
        torch.manual_seed(seed)
        d = varlen_clip_draws(m, [640, 48000])
        assert d["tmask"][0][0] <= 1 and 0 <= d["tmask"][1][0] and d["tmask"][1][1] <= 150


@pytest.mark.parametrize("lengths,kw,exc", [
    ([48000, 513], {}, PasstAmdError),                                   # a clip too short to reflect
    ([48000, 48001], dict(L=48000), ValueError),                         # longer than the batch's rows
    ([48000], dict(B=2), ValueError),                                    # one length for two rows
    (torch.tensor([48000.0, 640.0]), {}, ValueError),                    # floating-point lengths
    (torch.tensor([[48000, 640]]), {}, ValueError),                      # not 1-D
])
def test_a_rejected_call_consumes_no_rng(lengths, kw, exc):
    torch.manual_seed(5)
    state = torch.get_rng_state()
    with pytest.raises(exc):
        varlen_clip_draws(_mel(), lengths, **kw)
    assert torch.equal(torch.get_rng_state(), state)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_fixture_is_small_and_complete(golden_dir):
    path = os.path.join(golden_dir, "varlen_mel_train.npz")
    assert os.path.getsize(path) < 1 << 20
    gold = np.load(path)
    assert gold["frames"].tolist() == [150, 16, 63, 2, 150]
    for i, n in enumerate(MT.LENGTHS):
        assert gold[f"draw.{i}"].shape == (6,)
        covered = bool(MT.masked_cells(gold[f"draw.{i}"], MT.frames_of(n)).all())
        assert covered == (i == 3)                                       # the 2-frame clip lies wholly under its time band
        for k in (f"mel.{i}", f"dwave.{i}"):
            nrm, mx = gold[k + ".stats"]
            assert np.isfinite(gold[k]).all() and np.isfinite(nrm) and np.isfinite(mx), k
            if covered and k.startswith("dwave"):
                assert nrm == 0 and mx == 0                              # ... so nothing of it reaches the waveform
            else:
                assert nrm > 0 and mx > 0, k


@pytest.mark.skipif(not ref_import.reference_available(), reason="needs the reference checkout")
def test_fixture_regenerates_bit_identically(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setattr(MT, "HERE", str(tmp_path))
    state = torch.get_rng_state()
    MT.main()
    torch.set_rng_state(state)
    a, b = np.load(os.path.join(golden_dir, "varlen_mel_train.npz")), np.load(os.path.join(str(tmp_path), "varlen_mel_train.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


# ---- C ABI and public surface ------------------------------------------------------------------------------------------------------
def test_clip_struct_is_24_bytes_with_the_documented_offsets_on_both_sides():
    header = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} pa_mel_clip_params;", header)
    assert m, "pa_mel_clip_params is not declared in include/passt_amd.h"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    declared = []
    for stmt in body.split(";"):
        if stmt.strip():
            typ, names = stmt.split(None, 1)
            declared += [(n.strip(), typ) for n in names.split(",")]
    assert tuple(declared) == FIELDS                                     # six 4-byte fields in this order: offsets 0, 4, ..., 20
    # (mel.hip carries the static_assert of the same layout, so a library that was built has it)
    assert C.sizeof(_lib.MelClipParams) == 24
    for k, (name, typ) in enumerate(FIELDS):
        f = getattr(_lib.MelClipParams, name)
        assert (f.offset, f.size) == (4 * k, 4), name
        assert dict(_lib.MelClipParams._fields_)[name] is (C.c_float if typ == "float" else C.c_int32), name


def test_new_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert re.search(r"#define PA_ABI_VERSION 6\b", header)
    lib = _lib.load()
    assert lib.pa_abi_version() == 6
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name + " is not declared in include/passt_amd.h"
        assert name in _lib.SIGNATURES, name + " has no ctypes row"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name + ": argument count differs between header and ctypes"
        base = name[:-len("_aug")]
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[base][1]) + 1          # the _varlen list plus the table
    from passt_amd import ops
    assert callable(ops.mel_frontend_varlen_aug) and callable(ops.mel_frontend_bwd_varlen_aug) and callable(ops.upload_mel_clips)
    # host-side checks (no device needed: they return before any launch): the _varlen codes, and PA_EINVAL for a null table
    p = _lib.MelParams()
    p.n_fft, p.hop, p.n_mels, p.n_frames = 1024, 320, 128, 100
    one = 1 << 12          # any non-null address: the checks fail before anything is touched
    assert lib.pa_mel_frontend_fwd_varlen_aug(one, 1, 32000, one, one, one, one, one, 100, 0.0, p, None, None) == -1
    assert lib.pa_mel_frontend_bwd_varlen_aug(one, 1, 32000, one, one, one, one, one, 100, one, None, 0, p, None, None) == -1
    assert lib.pa_mel_frontend_fwd_varlen_aug(one, 1, 32000, None, one, one, one, one, 100, 0.0, p, one, None) == -1
    assert lib.pa_mel_frontend_fwd_varlen_aug(one, 1, 400, one, one, one, one, one, 100, 0.0, p, one, None) == -2
    assert lib.pa_mel_frontend_fwd_varlen_aug(one, 1, 32000, one, one, one, one, one, 101, 0.0, p, one, None) == -1
    assert lib.pa_mel_frontend_bwd_varlen_aug(one, 1, 32000, one, one, one, one, one, 101, one, None, 0, p, one, None) == -1
    p.n_mels = 200
    assert lib.pa_mel_frontend_fwd_varlen_aug(one, 1, 32000, one, one, one, one, one, 100, 0.0, p, one, None) == -2
    assert lib.pa_mel_frontend_bwd_varlen_aug(one, 1, 32000, one, one, one, one, one, 100, one, None, 0, p, one, None) == -2


def test_switch_is_off_by_default_and_documented():
    m = _mel()
    assert m.varlen_train is False
    torch.manual_seed(3)
    state = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="varlen_train"):
        m(torch.zeros(2, 48000), lengths=[48000, 640])
    assert torch.equal(torch.get_rng_state(), state)
    doc = passt_amd.AugmentMelSTFT.forward.__doc__ or ""
    assert "varlen_train" in doc and "its own" in doc
    m.varlen_train = True
    assert copy.deepcopy(m).varlen_train is True
    with pytest.raises(PasstAmdError, match="HIP device"):              # the switch does not open a CPU path
        m(torch.zeros(2, 48000), lengths=[48000, 640])
    assert torch.equal(torch.get_rng_state(), state)

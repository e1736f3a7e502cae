"""CPU tests of Patchout training on ragged batches (``net.varlen_train = True``): the host geometry and its RNG order against the
per-clip draw loop and against the reference's recorded draws (tests/golden/varlen_train.npz), the ValueError cases, the fixture, the
C ABI additions, the public switch."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from oracle import ref_import
from passt_amd import _lib
from passt_amd.passt import draw_patchout, kept_patches, varlen_geometry, varlen_geometry_train
from tests.golden import make_varlen_train_golden as VT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pa_patch_bwd_rows", "pa_patch_input_bwd_rows")


def _net(train=True, **patchout):
    """a tiny model with the fixture's geometry: 12 frequency rows, 25 time positions"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 256), stride=10, num_classes=5, embed_dim=64, depth=1, num_heads=1, distilled=True, **patchout)
    return net.train(train)


def _loop(net, lengths):
    """what the contract names: the clips one after the other, each with the fixed path's own draw calls"""
    rows = dict(row_clip=[], row_f=[], row_t=[], row_tpos=[])
    cu, toffs, kept = [0], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i, n in enumerate(lengths):
            toff, T_eff, idx_t, idx_f, idx_u = draw_patchout(net, 12, (n - 16) // 10 + 1)
            pf, pt = kept_patches(12, T_eff, idx_t, idx_f, idx_u)
            rows["row_clip"] += [i] * (2 + pf.size)
            rows["row_f"] += [-1, -1] + pf.tolist()
            rows["row_t"] += [0, 1] + pt.tolist()
            rows["row_tpos"] += [0, 1] + (pt + toff).tolist()
            cu.append(len(rows["row_f"]))
            toffs.append(toff)
            kept.append((pf, pt))
    return {k: np.array(v, np.int32) for k, v in rows.items()}, np.array(cu, np.int32), np.array(toffs, np.int32), kept


@pytest.mark.parametrize("patchout,lengths", [
    (dict(u_patchout=7), (16, 56, 106, 300)),
    (dict(s_patchout_t=2, s_patchout_f=3), (56, 106, 250, 256)),
    (dict(s_patchout_t=2, s_patchout_f=3, u_patchout=7), (106, 250)),
    (dict(), (33, 300, 16)),
])
def test_geometry_is_the_per_clip_draw_loop(patchout, lengths):
    net = _net(**patchout)
    torch.manual_seed(99)
    g = varlen_geometry_train(net, lengths, T_max=300)
    state = torch.get_rng_state()
    torch.manual_seed(99)
    rows, cu, toffs, kept = _loop(net, lengths)
    assert torch.equal(torch.get_rng_state(), state)                    # the generator ends where the loop leaves it
    for k, v in rows.items():
        assert g[k].dtype == np.int32 and np.array_equal(g[k], v), k
    assert np.array_equal(g["cu_tok"], cu) and np.array_equal(g["toff"], toffs) and g["toff"].dtype == np.int32
    assert g["max_N"] == int(np.diff(cu).max()) and g["Tg"] == max(g["T_eff"])
    assert g["cut"] == [i for i, n in enumerate(lengths) if (n - 16) // 10 + 1 >= 25]
    # the slot table: exactly the kept patches, each pointing at its own packed row
    slot = g["slot"]
    assert slot.dtype == np.int32 and slot.shape == (len(lengths), 12, g["Tg"])
    want = np.full_like(slot, -1)
    for i, (pf, pt) in enumerate(kept):
        want[i, pf, pt] = cu[i] + 2 + np.arange(pf.size)
    assert np.array_equal(slot, want)
    live = slot[slot >= 0]
    assert live.size == rows["row_f"].size - 2 * len(lengths) and np.unique(live).size == live.size
    assert np.array_equal(g["row_f"][live], np.nonzero(slot >= 0)[1]) and np.array_equal(g["row_t"][live], np.nonzero(slot >= 0)[2])
    assert int(g["row_tpos"].max()) < 25                                # every offset column lies inside the time embedding


def test_geometry_in_eval_mode_is_the_eval_geometry():
    net = _net(False, u_patchout=7, s_patchout_t=2)
    lengths = (16, 56, 300)
    state = torch.get_rng_state()
    g, e = varlen_geometry_train(net, lengths), varlen_geometry(lengths, 16, 10, 12, 25)
    assert torch.equal(torch.get_rng_state(), state)
    for k in ("row_clip", "row_f", "row_t", "cu_tok"):
        assert np.array_equal(g[k], e[k]), k
    assert np.array_equal(g["row_tpos"], g["row_t"]) and not g["toff"].any() and g["T_eff"] == e["T_eff"] and g["cut"] == e["cut"]


@pytest.mark.parametrize("patchout,lengths,clip", [
    (dict(s_patchout_t=5), (106, 56, 250), 1),                          # 5 patch columns <= s_patchout_t
    (dict(s_patchout_f=12), (106, 56), 0),                              # 12 frequency rows <= s_patchout_f
    (dict(u_patchout=12), (106, 16, 56), 1),                            # 12 patches left, u_patchout takes them all
    (dict(s_patchout_t=2, s_patchout_f=3, u_patchout=27), (106, 56), 1),        # (12 - 3) * (5 - 2) = 27 patches left
    (dict(s_patchout_t=2), (106, 300), 1),                              # 29 columns, cut to 25: the reference's index error
    (dict(u_patchout=7), (106, 15), 1),                                 # shorter than one patch
    (dict(u_patchout=7), (106, 301), 1),                                # longer than the input
])
def test_clips_that_cannot_satisfy_the_counts_are_named_before_any_draw(patchout, lengths, clip):
    net = _net(**patchout)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match=f"clip {clip}:"):
        varlen_geometry_train(net, lengths, T_max=300)
    assert torch.equal(torch.get_rng_state(), state)                    # a rejected batch consumes nothing
    with pytest.raises(ValueError, match="empty"):
        varlen_geometry_train(net, ())


def test_counts_at_their_limits_are_accepted():
    """one more column / row / patch than is dropped; structured time Patchout on a clip of exactly the embedding's 25 columns"""
    for patchout, lengths in ((dict(s_patchout_t=4), (56,)), (dict(s_patchout_f=11), (56,)), (dict(u_patchout=11), (16,)),
                              (dict(s_patchout_t=2), (256,))):
        g = varlen_geometry_train(_net(**patchout), lengths)
        assert g["row_f"].size > 2


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_fixture_is_small_and_complete(golden_dir):
    path = os.path.join(golden_dir, "varlen_train.npz")
    assert os.path.getsize(path) < 1 << 20
    gold = np.load(path)
    for name, case in VT.CASES.items():
        B = len(case["lengths"])
        assert gold[f"{name}.logits"].shape == (B, case["cfg"]["num_classes"]) and gold[f"{name}.features"].shape == (B, 768)
        assert gold[f"{name}.rng"].dtype == np.uint8 and gold[f"{name}.rng"].size == torch.get_rng_state().numel()
        for i in range(B):
            nrm, mx = gold[f"{name}.dx.{i}.stats"]
            assert np.isfinite(nrm) and nrm > 0 and mx > 0
        assert sorted(k[len(name) + 6:] for k in gold.files if k.startswith(f"{name}.grad.") and not k.endswith(".stats")) \
            == sorted(VT.param_grads(case["cfg"]))
    # what case (a) is there to show
    cu, toff = gold["a.cu_tok"], gold["a.toff"]
    assert np.diff(cu).tolist() == [2 + 5, 2 + 53, 2 + 113, 2 + 293] and toff[3] == 0


@pytest.mark.parametrize("name", list(VT.CASES))
def test_geometry_reproduces_the_reference_draws_of_the_fixture(golden_dir, name):
    """The index part of the fixture was rebuilt from what the reference's own RNG calls returned, clip after clip under one seed:
    the same seed through varlen_geometry_train gives the same rows, offsets and final generator state; and the pixels the kept
    patches cover are as many as the reference's dx has non-zero entries."""
    gold = np.load(os.path.join(golden_dir, "varlen_train.npz"))
    case = VT.CASES[name]
    cfg = case["cfg"]
    net = _net(u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"], s_patchout_f=cfg["s_patchout_f"])
    torch.manual_seed(case["torch_seed"])
    g = varlen_geometry_train(net, case["lengths"])
    assert np.array_equal(torch.get_rng_state().numpy(), gold[f"{name}.rng"])
    for k in VT.INDEX_KEYS:
        assert np.array_equal(g[k], gold[f"{name}.{k}"]), k
    for i, n in enumerate(case["lengths"]):
        rows = slice(int(g["cu_tok"][i]) + 2, int(g["cu_tok"][i + 1]))
        assert int(VT.covered(cfg, n, g["row_f"][rows], g["row_t"][rows]).sum()) == int(gold[f"{name}.dx.{i}.nonzero"]), i


@pytest.mark.skipif(not ref_import.reference_available(), reason="needs the reference checkout")
def test_fixture_regenerates_bit_identically(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setattr(VT, "HERE", str(tmp_path))
    state = torch.get_rng_state()
    VT.main()
    torch.set_rng_state(state)
    a, b = np.load(os.path.join(golden_dir, "varlen_train.npz")), np.load(os.path.join(str(tmp_path), "varlen_train.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k


# ---- C ABI and public surface ------------------------------------------------------------------------------------------------------
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
    from passt_amd import ops
    assert callable(ops.patch_bwd_rows) and callable(ops.patch_input_bwd_rows)
    # host-side checks (no device needed: they return before any launch)
    assert lib.pa_patch_input_bwd_rows(None, _lib.PA_F32, 10, None, 2, 5, 16, 10, 10, 128, 300, None, None) == -1
    assert lib.pa_patch_bwd_rows(None, 10, 64, None, None, None, 2, 5, 25, 12, None, None, None, None, None, None, 0, None) == -1


def test_switch_is_off_by_default_and_documented():
    net = _net()
    assert net.varlen_train is False
    x = torch.zeros(2, 1, 128, 106)
    with pytest.raises(NotImplementedError, match="ragged"):
        net(x, lengths=[106, 56])
    doc = passt_amd.PaSST.forward.__doc__ or ""
    assert "varlen_train" in doc and "batch size 1" in doc
    import copy
    net.varlen_train = True
    assert copy.deepcopy(net).varlen_train is True

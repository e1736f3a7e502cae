"""CPU tests of the gradients through the ragged-batch forward: the fixture against the reference and the oracle, the C ABI additions,
the public switches."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import torch

from oracle import detgen, ref_import
from oracle import passt_oracle as O
from passt_amd import _lib
from tests.golden import make_golden as G
from tests.golden import make_varlen_grad_golden as VG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pa_attention_bwd_varlen", "pa_attention_bwd_varlen_ws_floats", "pa_patch_input_bwd_varlen", "pa_patch_bwd_varlen")


def test_fixture_is_small_and_numeric(golden_dir):
    path = os.path.join(golden_dir, "varlen_grad.npz")
    assert os.path.getsize(path) < 1 << 20
    gold = np.load(path)
    assert all(gold[k].dtype.kind == "f" for k in gold.files)
    for name, case in VG.MODELS.items():
        for i in range(len(VG.LENGTHS)):
            for variant in VG.VARIANTS:
                nrm, mx = gold[f"{name}.{variant}.dx.{i}.stats"]
                assert np.isfinite(nrm) and nrm > 0 and mx > 0                      # every clip gives a finite, non-zero dx
        assert not any(k.startswith(f"{name}.frozen.grad.") for k in gold.files)
        assert sorted(k[len(name) + 16:] for k in gold.files if k.startswith(f"{name}.trainable.grad.") and not k.endswith(".stats")) \
            == sorted(VG.param_grads(case["cfg"]))


@pytest.mark.skipif(not ref_import.reference_available(), reason="needs the reference checkout")
def test_fixture_regenerates_bit_identically(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setattr(VG, "HERE", str(tmp_path))
    VG.main()
    a, b = np.load(os.path.join(golden_dir, "varlen_grad.npz")), np.load(os.path.join(str(tmp_path), "varlen_grad.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k


def _oracle(case, trainable):
    sd = O.to_torch(detgen.passt_state_dict(case["cfg"], case["seed"]), requires_grad=trainable)
    return VG.per_clip(case, trainable, lambda xt: O.passt_forward(sd, xt, case["cfg"], training=False)[:2], sd)


@pytest.mark.parametrize("variant", list(VG.VARIANTS))
@pytest.mark.parametrize("name", list(VG.MODELS))
def test_oracle_one_clip_at_a_time_matches_reference_fixture(golden_dir, name, variant):
    """the oracle's autograd, one clip at a time, against the fixture: sample entries, largest magnitude and L2 norm within 1e-5 of the
    clip's own largest entry / norm"""
    gold = dict(np.load(os.path.join(golden_dir, "varlen_grad.npz")))
    case = VG.MODELS[name]
    dxs, grads = _oracle(case, variant == "trainable")

    def check(key, got):
        got = np.ascontiguousarray(got, np.float32)
        nrm, scale = (float(v) for v in gold[key + ".stats"])
        assert np.abs(G.pin_sample(got, VG.DX_SAMPLE) - gold[key]).max() <= 1e-5 * scale, key
        assert abs(float(np.abs(got).max()) - scale) <= 1e-5 * scale, key
        assert abs(float(np.linalg.norm(got.astype(np.float64))) - nrm) <= 1e-5 * nrm, key
    for i, dx in enumerate(dxs):
        check(f"{name}.{variant}.dx.{i}", dx)
    for k, g in grads.items():
        check(f"{name}.{variant}.grad.{k}", g)
    if name == "small" and variant == "frozen":
        # what the length mix is there to show: the 1203-frame clip is cut (99 columns: frames 0 .. 995), the 33-frame clip has two
        # patch columns (26 frames)
        # (frequency rows 126, 127 lie behind the last patch row: 11 * 10 + 16)
        assert float(np.abs(dxs[2][..., 996:]).max()) == 0.0 and float(np.abs(dxs[2][..., :126, :996]).min()) > 0.0
        assert int((np.abs(dxs[7]).max(axis=(0, 1, 2)) > 0).sum()) == 26


def test_new_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert re.search(r"#define PA_ABI_VERSION 6\b", header)
    lib = _lib.load()
    assert lib.pa_abi_version() == 6
    for name in NEW_SYMBOLS:
        m = re.search(r"\b(?:int|int64_t) %s\(([^;]*)\);" % name, header)
        assert m, name + " is not declared in include/passt_amd.h"
        assert name in _lib.SIGNATURES, name + " has no ctypes row"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name + ": argument count differs between header and ctypes"
    args = re.search(r"int pa_attention_bwd_varlen\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["qkv", "ldqkv", "o", "d_o", "ldo", "lse", "ws", "dqkv", "lddqkv", "cu_tok", "B",
                                                                   "H", "max_N", "nq", "scale", "dtype", "flags", "stream"]
    from passt_amd import ops
    for fn in ("attention_bwd_varlen", "patch_input_bwd_varlen", "patch_bwd_varlen"):
        assert callable(getattr(ops, fn))
    # host-side checks (no device needed: they return before any launch)
    assert lib.pa_attention_bwd_varlen_ws_floats(5398, 8, 12, 1190) >= 2 * 12 * 5398
    assert lib.pa_attention_bwd_varlen_ws_floats(5398, 8, 12, 2) >= 2 * 8 * 12 * 2
    assert lib.pa_attention_bwd_varlen_ws_floats(0, 8, 12, 2) == 0
    assert lib.pa_attention_bwd_varlen(None, 2304, None, None, 768, None, None, None, 2304, None, 8, 12, 1190, 1190, 0.125, _lib.PA_BF16, 1, None) == -1
    assert lib.pa_patch_input_bwd_varlen(None, _lib.PA_F32, None, 8, 16, 10, 10, 128, 1203, None, None) == -1
    assert lib.pa_patch_bwd_varlen(None, 10, 64, None, 2, 99, 12, None, None, None, None, None, None, 0, None) == -1


def test_public_switches_and_signatures():
    import passt_amd
    from passt_amd import passt
    p = inspect.signature(passt_amd.PaSST.forward).parameters
    assert "lengths" in p and p["lengths"].default is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 100), stride=10, num_classes=5, embed_dim=64, depth=1, num_heads=1, distilled=True)
    assert net.varlen_grad is False and net.input_grad is False
    sig = inspect.signature(passt.passt_backward_varlen).parameters
    assert list(sig) == ["model", "ctx", "dlogits", "dfeat", "grads", "on_block_done", "want_dx"]
    assert sig["on_block_done"].default is None and sig["want_dx"].default is False
    assert list(inspect.signature(passt.passt_backward).parameters) == list(sig)
    s2 = inspect.signature(passt.passt_forward_varlen).parameters
    assert list(s2) == ["model", "x", "lengths", "save"] and s2["save"].default is False
    assert "varlen_grad" in (passt_amd.PaSST.forward.__doc__ or "")

"""CPU tests of the ragged-batch eval forward: the fixture against the oracle, the host geometry, the C ABI additions."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import detgen
from oracle import passt_oracle as O
from passt_amd import _lib
from passt_amd.passt import varlen_geometry
from tests.golden import make_varlen_golden as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pa_attention_fwd_varlen", "pa_patch_gather_varlen", "pa_patch_pos_table_varlen", "pa_mel_frontend_fwd_varlen")


@pytest.mark.parametrize("name", list(V.MODELS))
def test_oracle_one_clip_at_a_time_matches_reference_fixture(golden_dir, name):
    """oracle.passt_oracle.passt_forward, one clip at a time, against the real reference's per-clip outputs (the bound
    tests/test_oracle_pinned.py::test_model_oracle_vs_golden uses: atol 3e-5, rtol 1e-4)."""
    import warnings
    gold = dict(np.load(os.path.join(golden_dir, "varlen_eval.npz")))
    case = V.MODELS[name]
    sd = O.to_torch(detgen.passt_state_dict(case["cfg"], case["seed"]))
    x = V.model_input(case)
    for i, n in enumerate(V.LENGTHS):
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = O.passt_forward(sd, torch.from_numpy(np.ascontiguousarray(x[i:i + 1, :, :, :n])), case["cfg"], training=False)
        logits, feat = out[0], out[1]
        np.testing.assert_allclose(logits[0].numpy(), gold[name + ".logits"][i], atol=3e-5, rtol=1e-4, err_msg=f"clip {i} ({n} frames)")
        np.testing.assert_allclose(feat[0].numpy(), gold[name + ".features"][i], atol=3e-5, rtol=1e-4, err_msg=f"clip {i} ({n} frames)")


def _geometry_numpy(lengths, P, ts, F_dim, Tpe):
    """Plain restatement: clip after clip, [cls, dist, patches in frequency-major order], columns cut to Tpe."""
    rows, cu = [], [0]
    for i, n in enumerate(lengths):
        T = min((n - P) // ts + 1, Tpe)
        rows += [(i, -1, 0), (i, -1, 1)] + [(i, f, t) for f in range(F_dim) for t in range(T)]
        cu.append(len(rows))
    return np.array(rows, np.int32), np.array(cu, np.int32)


def test_varlen_geometry():
    g = varlen_geometry(V.LENGTHS, 16, 10, 12, 99, T_max=1203)
    rows, cu = _geometry_numpy(V.LENGTHS, 16, 10, 12, 99)
    assert np.array_equal(g["cu_tok"], cu) and g["cu_tok"].dtype == np.int32
    for k, col in (("row_clip", 0), ("row_f", 1), ("row_t", 2)):
        assert g[k].dtype == np.int32 and np.array_equal(g[k], rows[:, col]), k
    assert g["T_eff"] == [99, 43, 99, 1, 24, 63, 99, 2]
    assert g["cut"] == [0, 2, 6]                       # the reference warns when the columns REACH the embedding's length (:523)
    assert g["max_N"] == 2 + 12 * 99
    # other stride / a single clip / all equal
    g = varlen_geometry([100], 16, 16, 8, 7)
    rows, cu = _geometry_numpy([100], 16, 16, 8, 7)
    assert np.array_equal(g["row_t"], rows[:, 2]) and np.array_equal(g["cu_tok"], cu) and g["cut"] == [] and g["T_eff"] == [6]
    g = varlen_geometry(np.array([50, 50]), 16, 10, 3, 99)
    assert g["cu_tok"].tolist() == [0, 14, 28]
    g = varlen_geometry(torch.tensor([50, 16]), 16, 10, 3, 99)
    assert g["cu_tok"].tolist() == [0, 14, 19]
    with pytest.raises(ValueError, match="clip 1"):
        varlen_geometry([16, 15], 16, 10, 12, 99)
    with pytest.raises(ValueError, match="clip 0"):
        varlen_geometry([300, 16], 16, 10, 12, 99, T_max=299)
    with pytest.raises(ValueError):
        varlen_geometry([], 16, 10, 12, 99)


def test_new_entry_points_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert re.search(r"#define PA_ABI_VERSION 6\b", header)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared in include/passt_amd.h"
        assert name in _lib.SIGNATURES, name + " has no ctypes row"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name + ": argument count differs between header and ctypes"
    from passt_amd import ops
    for fn in ("attention_fwd_varlen", "patch_gather_varlen", "patch_pos_table_varlen", "mel_frontend_varlen"):
        assert callable(getattr(ops, fn))


def test_forward_signatures_take_lengths():
    import inspect

    import passt_amd
    for cls in (passt_amd.PaSST, passt_amd.AugmentMelSTFT, passt_amd.passt.EnsembelerModel):
        p = inspect.signature(cls.forward).parameters
        assert "lengths" in p and p["lengths"].default is None, cls.__name__

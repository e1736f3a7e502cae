"""CPU tests of the gradient w.r.t. the input spectrogram: the fixture against the oracle's own autograd, the C ABI addition."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

from oracle import detgen
from oracle import passt_oracle as O
from passt_amd import _lib
from tests.golden import make_golden as G
from tests.golden import make_input_grad_golden as IG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pa_patch_input_bwd", "pa_patch_input_bwd_ws_ints")


def oracle_step(case):
    """(logits, features, dx, {parameter: tensor}) of the oracle under the fixture's loss."""
    sd = O.to_torch(detgen.passt_state_dict(case["cfg"], case["seed"]), requires_grad=not case["frozen"])
    x, a, b = IG.inputs(case)
    xt = torch.from_numpy(x).requires_grad_()
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, feat = O.passt_forward(sd, xt, case["cfg"], training=case["training"])
    IG.loss_of(logits, feat, torch.from_numpy(a), torch.from_numpy(b)).backward()
    return logits.detach(), feat.detach(), xt.grad, sd


def _check_pinned(gold, key, got, what):
    """the oracle pinning tests' gradient rule (tests/test_oracle_pinned.py::_check_grads): stored entries within 2e-4 of the
    reference's largest magnitude, that magnitude within the same bound, the L2 norm within 1e-4"""
    got = np.ascontiguousarray(got, np.float32)
    nrm, scale = (float(v) for v in gold[key + ".stats"])
    ref = gold[key]
    smp = G.pin_sample(got, IG.DX_SAMPLE)
    assert smp.shape == ref.shape, what
    assert np.abs(smp - ref).max() <= 2e-4 * scale + 1e-9, what
    assert abs(float(np.abs(got).max()) - scale) <= 2e-4 * scale + 1e-9, what
    assert abs(float(np.linalg.norm(got.astype(np.float64))) - nrm) <= 1e-4 * nrm + 1e-9, what


@pytest.mark.parametrize("name", list(IG.CASES))
def test_oracle_autograd_dx_matches_reference_fixture(golden_dir, name):
    gold = dict(np.load(os.path.join(golden_dir, "input_grad.npz")))
    case = IG.CASES[name]
    logits, feat, dx, sd = oracle_step(case)
    np.testing.assert_allclose(logits.numpy(), gold[name + ".logits"], atol=3e-5, rtol=1e-4)
    np.testing.assert_allclose(feat.numpy(), gold[name + ".features"], atol=3e-5, rtol=1e-4)
    _check_pinned(gold, name + ".dx", dx.numpy(), name)
    for k in IG.PARAM_GRADS:
        if case["frozen"]:
            assert sd[k].grad is None and f"{name}.grad.{k}" not in gold
        else:
            _check_pinned(gold, f"{name}.grad.{k}", sd[k].grad.numpy(), (name, k))


def test_fixture_gradient_is_zero_where_no_kept_patch_reaches():
    """what the fixture's cases are there to show, on the oracle: behind the time cut and behind the last patch row / column"""
    case = IG.CASES["time_cut"]
    _, _, dx, _ = oracle_step(case)
    Tpe, P, ts = case["cfg"]["grid"][1], case["cfg"]["patch"], case["cfg"]["stride"][1]
    last = (Tpe - 1) * ts + P                       # first frame no kept patch column covers
    fl = (case["cfg"]["grid"][0] - 1) * case["cfg"]["stride"][0] + P
    assert last < case["T"] and dx[..., last:].abs().max().item() == 0.0
    assert fl < dx.shape[2] and dx[:, :, fl:, :].abs().max().item() == 0.0
    assert dx[:, :, :fl, :last].abs().min().item() > 0.0


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
    from passt_amd import ops
    assert callable(ops.patch_input_bwd)
    # host-side argument checks of the entry point (no device needed: they return before any launch)
    assert lib.pa_patch_input_bwd_ws_ints(128, 998, 16, 10, 10) == 12 * 99
    assert lib.pa_patch_input_bwd_ws_ints(128, 15, 16, 10, 10) == 0
    assert lib.pa_patch_input_bwd(None, _lib.PA_F32, 1, 1, None, None, 16, 10, 10, 128, 998, None, None, None) == -1


def test_backward_takes_the_input_gradient_switch():
    import inspect

    import passt_amd
    p = inspect.signature(passt_amd.passt.passt_backward).parameters
    assert "want_dx" in p and p["want_dx"].default is False

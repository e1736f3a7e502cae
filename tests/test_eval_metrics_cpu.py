"""CPU-only checks of the validation-metric feature: the NumPy restatement of the kernels' arithmetic reproduces the
scikit-learn values stored in tests/golden/eval_metrics.npz (and scikit-learn itself where it is installed), the fixture can be
made again bit for bit, the C entries exist and refuse bad arguments before they touch a device, and the Python layer has no CPU
path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import eval_metrics_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def inputs():
    return dict(np.load(K.GOLDEN))


def _close(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-12), (what, float(np.abs(got[ok] - want[ok]).max()))


@pytest.mark.parametrize("kind", K.KINDS)
def test_restatement_reproduces_the_fixture(inputs, kind):
    for n in K.NS:
        for C in K.CS:
            s, t, m = K.case(inputs, kind, n, C)
            r = K.restate(s, t, m)
            ap, auc = K.expected(inputs, kind, n, C)
            _close(r["ap"], ap, (kind, n, C, "ap"))
            _close(r["auc"], auc, (kind, n, C, "auc"))
            # the conventions for degenerate classes, on whatever classes of the case have them
            assert np.all(r["ap"][(r["n_pos"] == 0) & ~np.isnan(r["ap"])] == 0.0)
            assert np.all(np.isnan(r["auc"][(r["n_pos"] == 0) | (r["n_neg"] == 0)]))
    if kind == "nan":
        s, t, m = K.case(inputs, kind, 257, 20)
        r = K.restate(s, t, m)
        assert np.isnan(r["ap"][19]) and np.isnan(r["auc"][19]) and not np.isnan(r["ap"][:19]).any()
        assert r["n_pos"][19] + r["n_neg"][19] == 256


def test_restatement_reproduces_the_sigmoid_members(inputs):
    _, target, _ = K.base(inputs)
    r = K.restate(inputs["sigmoid_f32"], target[:, :K.SIGMOID_C])
    _close(r["ap"], inputs["ap_sigmoid"], "ap_sigmoid")
    _close(r["auc"], inputs["auc_sigmoid"], "auc_sigmoid")


def test_cases_cover_what_they_claim(inputs):
    s, t, m = K.case(inputs, "denormal", 1000, 3)
    bits = s.view(np.uint32)
    assert set(np.unique(bits)) == {0, 1, 2, 3, 0x80000000, 0x80000001, 0x80000002, 0x80000003}
    k = K.score_key(s)
    assert np.all(k[bits == 0x80000000] == k[bits == 0][0]) and len(np.unique(k)) == 7          # -0 ties with +0, nothing else ties
    assert np.array_equal(K.key_score(K.score_key(inputs["sigmoid_f32"])), inputs["sigmoid_f32"])
    order = np.argsort(inputs["sigmoid_f32"][:, 0], kind="stable")
    assert np.all(np.diff(K.score_key(inputs["sigmoid_f32"][order, 0]).astype(np.int64)) >= 0)
    s, t, m = K.case(inputs, "masked", 1000, 20)
    assert 0.55 < m.mean() < 0.65 and not (m[:, 19] * t[:, 19]).any() and t[:, 19].any()
    s, t, m = K.case(inputs, "ties8", 1000, 1)
    assert len(np.unique(s)) == 8
    z = K.sigmoid_sweep()
    assert np.all(np.diff(z) >= 0) and z.min() == -103 and z.max() == 103 and np.signbit(z[z == 0]).tolist() == [True, False]
    assert {K.batch_size(n, C) for n in K.NS for C in K.CS} == set(K.BS)


def test_restatement_against_scikit_learn_live(inputs):
    pytest.importorskip("sklearn")
    for kind, n, C in (("random", 257, 20), ("ties8", 1000, 3), ("masked", 256, 65), ("degenerate", 64, 3), ("equal", 65, 1)):
        s, t, m = K.case(inputs, kind, n, C)
        r = K.restate(s, t, m)
        ap, auc = K.sklearn_expected(s, t, m)
        _close(r["ap"], ap, (kind, "ap"))
        _close(r["auc"], auc, (kind, "auc"))


def test_fixture_regenerates_bit_identically(tmp_path):
    pytest.importorskip("sklearn")
    out = str(tmp_path / "again.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_eval_metrics_golden.py"), out], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == open(K.GOLDEN, "rb").read()
    assert os.path.getsize(K.GOLDEN) < 512 * 1024


def test_entries_exist_and_refuse_bad_arguments_without_a_device():
    from passt_amd import _lib
    lib = _lib.load()
    assert lib.pa_abi_version() == 6
    buf = (ctypes.c_uint64 * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    app = lib.pa_eval_append
    # (scores, target, mask, B, C, n0, capacity, mode, keys, state, stream)
    assert app(None, q, None, 1, 1, 0, 4, 1, q, q, None) == -1 and app(q, None, None, 1, 1, 0, 4, 1, q, q, None) == -1
    assert app(q, q, None, 1, 1, 0, 4, 1, None, q, None) == -1 and app(q, q, None, 1, 1, 0, 4, 1, q, None, None) == -1
    assert app(q, q, None, 0, 1, 0, 4, 1, q, q, None) == -1 and app(q, q, None, 1, 0, 0, 4, 1, q, q, None) == -1
    assert app(q, q, None, 2, 1, 3, 4, 1, q, q, None) == -1            # n0 + B > capacity
    assert app(q, q, None, 1, 1, -1, 4, 1, q, q, None) == -1 and app(q, q, None, 1, 1, 0, 4, 2, q, q, None) == -1
    assert app(q, q, None, 1, 1, 0, 1 << 31, 1, q, q, None) == -2
    rank = lib.pa_eval_rank
    # (keys, state, C, n, capacity, ws, n_pos, n_neg, auc_num, ap, auc, stream)
    good = [q, q, 1, 4, 4, q, q, q, q, q, q, None]
    for i in (0, 1, 5, 6, 7, 8, 9, 10):
        bad = list(good)
        bad[i] = None
        assert rank(*bad) == -1, i
    for i, v in ((2, 0), (3, -1), (3, 5), (4, 0)):
        bad = list(good)
        bad[i] = v
        assert rank(*bad) == -1, (i, v)
    assert rank(q, q, 1, 4, 1 << 31, q, q, q, q, q, q, None) == -2
    # the workspace: two u32 key rows per class, counts, the tile map, 16 bytes per tile
    ws = lib.pa_eval_ws_bytes
    assert ws(0, 16) == 0 and ws(1, 0) == 0 and ws(1, 1 << 31) == 0
    assert ws(1, 1) >= 2 * 4 + 16 + 8 + 16 and ws(527, 32768) >= 2 * 527 * 32768 * 4 + 527 * 128 * 16
    assert ws(527, 32768) < 2 * 527 * 32768 * 4 + 527 * 128 * 16 + 527 * 32 + 256 and ws(3, 100) % 16 == 0


def test_python_layer_has_no_cpu_path():
    from passt_amd import ops
    from passt_amd._lib import PasstAmdError
    from passt_amd.metrics import EvalAccumulator
    acc = EvalAccumulator(5)
    with pytest.raises(PasstAmdError):
        acc.update(torch.zeros(4, 5), torch.zeros(4, 5))
    with pytest.raises(PasstAmdError):
        ops.eval_append(torch.zeros(4, 5), torch.zeros(4, 5), torch.zeros(5, 8, dtype=torch.int32), torch.zeros(5, 8, dtype=torch.uint8), 0)
    with pytest.raises(PasstAmdError):
        ops.eval_rank(torch.zeros(5, 8, dtype=torch.int32), torch.zeros(5, 8, dtype=torch.uint8), 4)
    with pytest.raises(ValueError):
        EvalAccumulator(5, scores="softmax")
    if not torch.cuda.is_available():
        with pytest.raises(PasstAmdError):
            acc.compute()

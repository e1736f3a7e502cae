"""Host side of sliding-window inference (PaSST.forward_windows): the window geometry against a brute-force rule, every refusal of
the method and of the two C entries without a device, the ABI, and the checkers of tests/windows_cases.py run against plain torch
-- they must pass a correct implementation and reject the fault models a window gather and a per-recording pool invite."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from passt_amd import _lib
from passt_amd._lib import PA_BF16, PA_F32
from passt_amd.passt import check_window_rule, window_chunks, window_geometry, window_spans
from tests import windows_cases as W
from tests.golden import make_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PA_EINVAL = -1


# ---- geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,window,hop,tail", W.GEOMETRY_TABLE)
def test_geometry_against_brute_force(n, window, hop, tail):
    g = W.check_geometry(window_geometry, [n], window, hop, tail)
    assert window_spans(n, window, hop, tail, W.P_) == W.brute_windows(n, window, hop, tail)
    if n > window:
        assert len(g["win_src"]) + len(g["dropped"]) == -(-(n - window) // hop) + 1


def test_geometry_table_holds_the_cases_it_claims():
    t = [r for r in W.GEOMETRY_TABLE if r[3] == "short"]
    assert any(n == w for n, w, h, _ in t) and any(n == w + 1 for n, w, h, _ in t)
    assert any(n > w and (n - w) % h == 0 for n, w, h, _ in t) and any(n > w and (n - w) % h for n, w, h, _ in t)
    assert any(h == 1 for _, _, h, _ in t) and any(h == w and n > w for n, w, h, _ in t) and any(n == W.P_ for n, *_ in t)
    tails = [W.brute_windows(n, w, h, "short") for n, w, h, _ in t]
    assert any(gone and gone[0][1] == W.P_ - 1 for _, gone in tails), "no dropped tail of P - 1 frames"
    assert any(not gone and spans[-1][1] == W.P_ for spans, gone in tails if len(spans) > 1), "no kept tail of P frames"


@pytest.mark.parametrize("tail", ["align", "short"])
@pytest.mark.parametrize("hop", [100, 37, 1])
def test_geometry_of_the_recordings(tail, hop):
    g = W.check_geometry(window_geometry, W.RECORDINGS, W.WINDOW, hop, tail)
    assert g["offsets"][-1] == len(g["win_src"]) and (np.diff(g["offsets"]) >= 1).all()


def test_geometry_large_case_and_chunks():
    g = window_geometry([60000], 998, 499, "align", 16, 10, 12)
    assert len(g["win_src"]) == 120 and g["row_f"].size == 142800 and g["max_N"] == 1190
    ntok = np.diff(g["cu_tok"]).tolist()
    ch = window_chunks(ntok, 32 * 1190)
    assert ch == [(0, 32), (32, 64), (64, 96), (96, 120)]
    assert window_chunks(ntok, None) == [(0, 120)] and window_chunks(ntok, 1) == [(w, w + 1) for w in range(120)]
    assert window_chunks([290, 290, 290, 30, 290], 3 * 290) == [(0, 3), (3, 5)]


def test_window_rule_refusals():
    for bad in (dict(window=15), dict(hop=0), dict(hop=251), dict(tail="pad"), dict(window=250.5), dict(hop=True)):
        kw = dict(window=250, hop=100, tail="align", P=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_window_rule(**kw)
    with pytest.raises(ValueError, match="recording 1"):
        window_geometry([250, 15], 250, 100, "align", 16, 10, 12)
    with pytest.raises(ValueError):
        window_geometry([], 250, 100, "align", 16, 10, 12)


# ---- refusals of forward_windows: a CPU model, nothing can be launched ---------------------------------------------------------------
def _cpu_model():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return passt_amd.PaSST(img_size=G.SMALL["img_size"], stride=10, num_classes=37, embed_dim=128, depth=2, num_heads=2, distilled=True).eval()


def test_forward_windows_refusals(monkeypatch):
    from passt_amd import ops
    m = _cpu_model()
    x = torch.zeros(2, 1, 128, 600)

    def no_launch(*a, **k):
        raise AssertionError("a refused call reached a kernel wrapper")
    for name in ("patch_gather_windows", "window_pool", "upload_small", "gemm_nt"):
        monkeypatch.setattr(ops, name, no_launch)
    m.train()
    with pytest.raises(NotImplementedError):
        m.forward_windows(x)
    m.eval()
    for kw in (dict(window=15), dict(hop=0), dict(hop=251), dict(window=100, hop=101), dict(tail="pad"), dict(pool="sum"),
               dict(pool_of="softmax"), dict(max_tokens=0), dict(max_tokens=2.5),
               dict(window=266)):                       # (266 - 16) // 10 + 1 = 26 patch columns > the time embedding's 25
        with pytest.raises(ValueError):
            m.forward_windows(x, **kw)
    with pytest.raises(ValueError, match="recording 1"):
        m.forward_windows(x, [600, 15])
    with pytest.raises(ValueError, match="recording 0"):
        m.forward_windows(x, [601, 300])
    with pytest.raises(ValueError):
        m.forward_windows(x, [600])
    with pytest.raises(ValueError):
        m.forward_windows(x, torch.tensor([600.0, 300.0]))
    with pytest.raises(ValueError):
        m.forward_windows(x[0])
    # everything valid: the first thing that needs the device refuses the CPU tensor -- after every host check, before any launch
    with pytest.raises(_lib.PasstAmdError, match="HIP device only"):
        m.forward_windows(x, [600, 300], window=265, hop=7, tail="short", pool="max", pool_of="sigmoid", max_tokens=500)
    ens = passt_amd.EnsembelerModel([m, _cpu_model()]).eval()
    with pytest.raises(ValueError):
        ens.forward_windows(x, hop=0)
    with pytest.raises(ValueError, match="recording 1"):
        ens.forward_windows(x, [600, 15])
    ens.models[1].train()
    with pytest.raises(NotImplementedError):
        ens.forward_windows(x)


def test_window_pool_wrapper_refusals():
    from passt_amd import ops
    rows = torch.zeros(5, 3)
    for off in ([0, 2, 2, 5], [1, 5], [0, 4], [0], [0, 3, 2, 5]):
        with pytest.raises(ValueError):
            ops.window_pool(rows, off)
    with pytest.raises(ValueError):
        ops.window_pool(rows, [0, 5], mode="sum")
    with pytest.raises(ValueError):
        ops.window_pool(rows, [0, 5], act="tanh")


def test_tag_converts_seconds_with_the_front_ends_hop():
    from passt_amd import windows

    class Mel:
        sr, hopsize = 32000, 320
    assert windows.seconds_to_frames(Mel, 10.0) == 1000 and windows.seconds_to_frames(Mel, 2.5) == 250
    assert windows.seconds_to_frames(Mel, 0.014) == 1
    assert "spectrogram" in windows.__doc__.lower() and "reflect" in windows.__doc__.lower()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_entries():
    header = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert re.search(r"#define PA_ABI_VERSION 6\b", header)
    lib = _lib.load()
    assert lib.pa_abi_version() == 6
    for name in ("pa_patch_gather_windows", "pa_window_pool"):
        assert re.search(r"\bint %s\(" % name, header), name + " is not declared in include/passt_amd.h"
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert "windows.hip" in open(os.path.join(ROOT, "passt_amd", "csrc", "Makefile")).read()


def test_c_entries_refuse_without_a_device():
    lib = _lib.load()
    raw = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(raw) + 15) & ~15               # never dereferenced: every call below is refused before a launch
    good = dict(x=p, B=2, F=128, T=1203, win_src=p, win_t0=p, win_len=p, W=3, row_win=p, row_f=p, row_t=p, M=10, P=16, fs=10, ts=10,
                cols=p, dtype=PA_F32, stream=None)
    order = list(good)
    bad = [dict(x=None), dict(win_src=None), dict(win_t0=None), dict(win_len=None), dict(row_win=None), dict(row_f=None), dict(row_t=None),
           dict(cols=None), dict(B=0), dict(F=0), dict(T=0), dict(W=0), dict(M=0), dict(P=0), dict(fs=0), dict(ts=0), dict(B=-1),
           dict(dtype=2), dict(dtype=-1)]
    for b in bad:
        a = dict(good, **b)
        assert lib.pa_patch_gather_windows(*[a[k] for k in order]) == PA_EINVAL, b
    assert lib.pa_patch_gather_windows(*[dict(good, P=33)[k] for k in order]) == -2       # PA_EUNSUPPORTED: 33 * 33 threads
    good = dict(inp=p, W=5, C=3, offsets=p, B=2, mode=_lib.POOL_MEAN, act=_lib.POOL_ACT_NONE, out=p, stream=None)
    order = list(good)
    bad = [dict(inp=None), dict(offsets=None), dict(out=None), dict(W=0), dict(C=0), dict(B=0), dict(mode=2), dict(mode=-1), dict(act=2),
           dict(act=-1), dict(B=6)]                      # B > W: some recording has no window
    for b in bad:
        a = dict(good, **b)
        assert lib.pa_window_pool(*[a[k] for k in order]) == PA_EINVAL, b


# ---- the checkers on plain torch, and the fault models they must reject ----------------------------------------------------------
def _gather_case(hop=37, tail="align", lengths=None):
    lengths = lengths or [437, 16, 251]
    g = window_geometry(lengths, W.WINDOW, hop, tail, W.P_, W.TS, W.F_DIM)
    return g, lengths


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
def test_checkers_pass_plain_torch(dt):
    impl = W.TorchWindows()
    for tail in ("align", "short"):
        g, lengths = _gather_case(tail=tail)
        x = W.nan_behind(W.code_x(len(lengths), W.F_BINS, max(lengths), dt), lengths)
        W.check_gather(impl.gather, x, g, dt, what=tail)
    for k, (off, C) in enumerate(W.POOL_CASES):
        for mode in ("mean", "max"):
            for act in (None, "sigmoid"):
                W.check_pool(impl.pool, W.pool_rows(off[-1], C, k), off, mode, act)
    W.check_pool(impl.pool, W.pool_rows(30, 37, 9, negative=True), W.POOL_CASES[0][0], "max", None)
    for tail in ("align", "short"):
        W.check_geometry(impl.geometry, W.RECORDINGS, W.WINDOW, 100, tail)


def test_sigmoid_restatement_is_within_the_allowance():
    z = W.sigmoid_family()
    err = (W.TorchWindows().sigmoid(z).double() - torch.sigmoid(z.double())).abs().max()
    assert 0 < float(err) <= W.SIGMOID_ALLOWANCE < 1e-6


class RoundsT0(W.TorchWindows):
    def first_frame(self, t0, ts):
        return t0 // ts * ts


class IndexesByWindow(W.TorchWindows):
    def recording(self, w, win_src):
        return min(w, int(max(win_src)))


class LargestCount(W.TorchWindows):
    def count(self, lo, hi, offsets):
        return int(np.diff(np.asarray(offsets)).max())


class TakesNextRow(W.TorchWindows):
    def last_row(self, hi):
        return hi + 1


class MaxFromZero(W.TorchWindows):
    def max_start(self, first):
        return torch.zeros_like(first)


class UnanchoredAlign(W.TorchWindows):
    def geometry(self, lengths, window, hop, tail, P, ts, F_dim):
        from passt_amd import passt
        g = passt.window_geometry(lengths, window, hop, tail, P, ts, F_dim)
        if tail == "align":                              # the last window stays on the hop grid and loses its end
            off = g["offsets"]
            t0 = g["win_t0"].copy()
            for b in range(len(lengths)):
                k = off[b + 1] - off[b]
                if k > 1:
                    t0[off[b + 1] - 1] = (k - 1) * hop
            g = dict(g, win_t0=t0)
        return g


def test_fault_models_are_rejected():
    g, lengths = _gather_case(hop=37)
    for dt in (PA_F32, PA_BF16):
        x = W.nan_behind(W.code_x(len(lengths), W.F_BINS, max(lengths), dt), lengths)
        for bad in (RoundsT0(), IndexesByWindow()):
            with pytest.raises(AssertionError):
                W.check_gather(bad.gather, x, g, dt, what=type(bad).__name__)
    off, C = W.POOL_CASES[0]
    rows = W.pool_rows(off[-1], C, 0)
    with pytest.raises(AssertionError):
        W.check_pool(LargestCount().pool, rows, off, "mean", None)
    for mode in ("mean", "max"):
        with pytest.raises(AssertionError):
            W.check_pool(TakesNextRow().pool, rows, off, mode, None)
    with pytest.raises(AssertionError):
        W.check_pool(MaxFromZero().pool, W.pool_rows(off[-1], C, 0, negative=True), off, "max", None)
    W.check_pool(W.TorchWindows().pool, W.pool_rows(off[-1], C, 0, negative=True), off, "max", None)
    with pytest.raises(AssertionError):
        W.check_geometry(UnanchoredAlign().geometry, W.RECORDINGS, W.WINDOW, 100, "align")

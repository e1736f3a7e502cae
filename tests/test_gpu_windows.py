"""GPU tests of sliding-window inference: pa_patch_gather_windows and pa_window_pool through the C ABI, and PaSST.forward_windows on
top of the packed trunk.

Contract: window w of recording b gets what ``net(x[b:b+1, :, :, s:e])`` returns alone at batch size 1 in eval mode; for the same
windows the outputs equal the ragged forward on explicitly unfolded copies bit for bit; nothing behind a recording's length is read
(the tests fill it with NaN).  Reference values: tests/golden/windows_eval.npz (the real reference run window by window,
tests/golden/make_windows_golden.py).  Checkers and operands: tests/windows_cases.py.
"""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from passt_amd import _lib, ops, windows  # noqa: E402
from passt_amd._lib import PA_BF16, PA_F32  # noqa: E402
from passt_amd.passt import window_geometry  # noqa: E402
from tests import windows_cases as W  # noqa: E402
from tests.golden import make_varlen_golden as V  # noqa: E402
from tests.golden import make_windows_golden as WG  # noqa: E402
from tests.row_kernel_cases import GuardedOut, guarded_in  # noqa: E402
from tests.test_gpu_model import BF16_LOGITS, build, record, rel  # noqa: E402

DEV = "cuda"
I32 = torch.int32


def _lim(precision):
    return 1e-3 if precision == "fp32" else BF16_LOGITS


@functools.lru_cache(maxsize=None)
def _model(name, precision, seed=None):
    case = WG.CASES[name] if seed is None else dict(WG.CASES[name], seed=seed)
    return build(case, precision).eval()


@functools.lru_cache(maxsize=None)
def _input(name, fill=float("nan")):
    case = WG.CASES[name]
    return W.nan_behind(torch.from_numpy(WG.model_input(case)), case["recordings"], fill).to(DEV)


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "windows_eval.npz")))


def _quiet(fn, *a, **k):
    with warnings.catch_warnings(), torch.no_grad():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


# ---- 1. the gather through the C ABI, exact ------------------------------------------------------------------------------------------
def kernel_gather(x, win_src, win_t0, win_len, row_win, row_f, row_t, P, fs, ts, dt):
    """pa_patch_gather_windows on guarded buffers: NaN around x, sentinels around cols"""
    B, _, F, T = x.shape
    xd = guarded_in(x.contiguous(), DEV)
    idx = [guarded_in(torch.from_numpy(np.ascontiguousarray(a)).to(I32), DEV) for a in (win_src, win_t0, win_len, row_win, row_f, row_t)]
    M = len(row_f)
    out = GuardedOut((M, P * P), W.TD[dt], DEV)
    rc = _lib.load().pa_patch_gather_windows(xd.data_ptr(), B, F, T, idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(), len(win_src),
                                             idx[3].data_ptr(), idx[4].data_ptr(), idx[5].data_ptr(), M, P, fs, ts, out.ptr(), dt,
                                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.take("pa_patch_gather_windows")


GATHER_CASES = {
    # name: (recordings' lengths, window, hop, tail); the buffer is (6, 1, 128, 1203) for all of them: T_pitch 1203, odd
    "hop100": (W.RECORDINGS, 250, 100, "align"),
    "hop100_short": (W.RECORDINGS, 250, 100, "short"),
    "hop37": (W.RECORDINGS, 250, 37, "align"),
    "hop37_short": (W.RECORDINGS, 250, 37, "short"),
    "hop1": ([min(n, 283) for n in W.RECORDINGS], 250, 1, "align"),
    "ends_on_last_frame": (W.RECORDINGS, 246, 100, "align"),         # (246 - 16) % 10 == 0: the last patch column ends at frame n - 1
    "ends_one_earlier": (W.RECORDINGS, 247, 100, "align"),
    "one_column": ([min(n, 100) for n in W.RECORDINGS], 16, 16, "short"),
    "one_column_hop7": ([min(n, 60) for n in W.RECORDINGS], 16, 7, "align"),
}


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
@pytest.mark.parametrize("name", list(GATHER_CASES))
def test_gather_windows_exact(name, dt):
    lengths, window, hop, tail = GATHER_CASES[name]
    g = window_geometry(lengths, window, hop, tail, W.P_, W.TS, W.F_DIM)
    x = W.nan_behind(W.code_x(len(lengths), W.F_BINS, max(W.RECORDINGS), dt), lengths)
    assert x.shape[-1] == 1203
    if name.startswith("ends_on"):
        last = g["win_t0"] + (np.asarray(g["T_eff"]) - 1) * W.TS + W.P_
        assert any(int(e) == lengths[int(b)] for e, b in zip(last, g["win_src"]))
    got = W.check_gather(kernel_gather, x, g, dt, what=name)
    # the same rows as the ragged gather on explicitly unfolded copies
    u = W.unfold(x, g).to(DEV)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    ref = ops.patch_gather_varlen(u, dev(g["row_clip"]), dev(g["row_f"]), dev(g["row_t"]), W.P_, W.FS, W.TS, dt)
    assert torch.equal(got, ref.cpu()), name


@pytest.mark.parametrize("dt", [PA_F32, PA_BF16])
def test_gather_windows_single_window_single_recording(dt):
    g = window_geometry([250], 250, 100, "align", W.P_, W.TS, W.F_DIM)
    assert len(g["win_src"]) == 1
    x = W.code_x(1, W.F_BINS, 251, dt)                   # pitch 251: one frame behind the recording, NaN
    W.check_gather(kernel_gather, W.nan_behind(x, [250]), g, dt, what="W=1,B=1")
    # through the wrapper as well
    dev = lambda a: torch.from_numpy(a).to(DEV)
    cols = ops.patch_gather_windows(W.nan_behind(x, [250]).to(DEV), dev(g["win_src"]), dev(g["win_t0"]), dev(g["win_len"]), dev(g["row_clip"]),
                                    dev(g["row_f"]), dev(g["row_t"]), W.P_, W.FS, W.TS, dt)
    W.check_gather(lambda *a: cols.cpu(), W.nan_behind(x, [250]), g, dt, what="wrapper")


# ---- 2. windows == the unfolded ragged path, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("tail", ["align", "short"])
@pytest.mark.parametrize("hop", [100, 37])
def test_windows_equal_unfolded_ragged_forward(hop, tail, precision):
    m, x = _model("small", precision), _input("small")
    lo, fe, win = m.forward_windows(x, W.RECORDINGS, window=W.WINDOW, hop=hop, tail=tail, pool=None)
    assert lo is win.logits and fe is win.features
    assert lo.grad_fn is None and fe.grad_fn is None and not lo.requires_grad
    g = W.check_geometry(window_geometry, W.RECORDINGS, W.WINDOW, hop, tail)
    assert win.offsets.tolist() == g["offsets"].tolist() and win.start.tolist() == g["win_t0"].tolist()
    assert win.length.tolist() == g["win_len"].tolist() and win.dropped == g["dropped"]
    assert win.offsets.dtype == win.start.dtype == win.length.dtype == torch.int64 and not win.offsets.is_cuda
    assert lo.shape == (len(g["win_src"]), 37) and fe.shape == (len(g["win_src"]), 128)
    u = W.unfold(x.cpu(), g).to(DEV)
    l1, f1 = _quiet(m, u, lengths=win.length)
    torch.cuda.synchronize()
    assert torch.isfinite(lo).all() and torch.isfinite(fe).all()
    assert torch.equal(lo, l1) and torch.equal(fe, f1)


# ---- 3. windows against the reference and against the plain forward on the slice --------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(WG.CASES))
def test_windows_vs_reference_and_single(name, precision):
    gold, case = _gold(), WG.CASES[name]
    m, x = _model(name, precision), _input(name)
    worst = dict(logits=0.0, features=0.0, logits_vs_single=0.0, features_vs_single=0.0)
    for hop, tail in case["rules"]:
        k = f"{name}.{hop}.{tail}"
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            lo, fe, win = m.forward_windows(x, case["recordings"], window=case["window"], hop=hop, tail=tail, pool=None)
        assert not [c for c in caught if "will be cut" in str(c.message)]
        assert win.start.tolist() == gold[k + ".start"].tolist() and win.length.tolist() == gold[k + ".length"].tolist()
        assert win.offsets.tolist() == gold[k + ".offsets"].tolist()
        lo, fe = lo.cpu(), fe.cpu()
        assert torch.isfinite(lo).all() and torch.isfinite(fe).all()
        single = hop == case["rules"][0][0]                  # the batch-1 loop over the slices: the first hop's windows
        for w, (b, s, n) in enumerate(zip(np.repeat(np.arange(len(case["recordings"])), np.diff(win.offsets.numpy())), win.start.tolist(),
                                          win.length.tolist())):
            errs = [rel(lo[w], gold[k + ".logits"][w]), rel(fe[w], gold[k + ".features"][w])]
            if single:
                l1, f1 = _quiet(m, x[b:b + 1, :, :, s:s + n].contiguous())
                errs += [rel(lo[w], l1[0].cpu()), rel(fe[w], f1[0].cpu())]
            for key, v in zip(worst, errs):
                worst[key] = max(worst[key], v)
    print(f"windows {name}[{precision}]: {worst}")
    record(f"windows_eval_{name}[{precision}]", **worst)
    assert all(v < _lim(precision) for v in worst.values()), worst


# ---- 4. nothing behind a length is read ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_nothing_behind_a_length_is_read(precision):
    m = _model("small", precision)
    for tail in ("align", "short"):
        a = m.forward_windows(_input("small"), W.RECORDINGS, window=W.WINDOW, hop=37, tail=tail, pool="mean")
        b = m.forward_windows(_input("small", 1e30), W.RECORDINGS, window=W.WINDOW, hop=37, tail=tail, pool="mean")
        for p, q in zip(a[:2] + (a[2].logits, a[2].features), b[:2] + (b[2].logits, b[2].features)):
            assert torch.isfinite(p).all() and torch.equal(p, q)


# ---- 5. pooling -------------------------------------------------------------------------------------------------------------------
def kernel_pool(rows, offsets, mode, act):
    return ops.window_pool(rows.to(DEV), offsets, mode, act).cpu()


def test_sigmoid_error_is_within_the_allowance():
    z = W.sigmoid_family()
    got = kernel_pool(z.view(-1, 1), list(range(z.numel() + 1)), "mean", "sigmoid").view(-1)       # one row per recording: the sigmoid itself
    err = float((got.double() - torch.sigmoid(z.double())).abs().max())
    print(f"kernel sigmoid: largest error {err:.3e} over {z.numel()} logits; allowance {W.SIGMOID_ALLOWANCE:.3e}")
    record("windows_sigmoid", error=err, allowance=W.SIGMOID_ALLOWANCE)
    assert err <= W.SIGMOID_ALLOWANCE < 1e-6


@pytest.mark.parametrize("act", [None, "sigmoid"])
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_window_pool_kernel(mode, act):
    for k, (off, C) in enumerate(W.POOL_CASES):
        W.check_pool(kernel_pool, W.pool_rows(off[-1], C, k), off, mode, act, what=f"case {k}", show=True)
    W.check_pool(kernel_pool, W.pool_rows(30, 37, 9, negative=True), W.POOL_CASES[0][0], mode, act, what="negative", show=True)
    # guarded buffers through the C ABI: nothing outside out is written, every element of out is
    off, C = W.POOL_CASES[0]
    rows = W.pool_rows(off[-1], C, 3)
    out = GuardedOut((len(off) - 1, C), torch.float32, DEV)
    rows_d, off_d = guarded_in(rows, DEV), guarded_in(torch.tensor(off, dtype=I32), DEV)
    rc = _lib.load().pa_window_pool(rows_d.data_ptr(), off[-1], C, off_d.data_ptr(),
                                    len(off) - 1, _lib.POOL_MAX if mode == "max" else _lib.POOL_MEAN,
                                    _lib.POOL_ACT_SIGMOID if act else _lib.POOL_ACT_NONE, out.ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out.take("pa_window_pool"), kernel_pool(rows, off, mode, act))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_windows_pooling(precision):
    m, x = _model("small", precision), _input("small")
    _, _, win = m.forward_windows(x, W.RECORDINGS, window=W.WINDOW, hop=100, pool=None)
    off = win.offsets.tolist()
    assert 1 in np.diff(off).tolist() and max(np.diff(off)) > 2
    for pool in ("mean", "max"):
        for pool_of in ("logits", "sigmoid"):
            lo, fe, win2 = m.forward_windows(x, W.RECORDINGS, window=W.WINDOW, hop=100, pool=pool, pool_of=pool_of)
            assert torch.equal(win2.logits, win.logits) and torch.equal(win2.features, win.features)
            act = "sigmoid" if pool_of == "sigmoid" else None
            assert lo.shape == (len(W.RECORDINGS), 37) and fe.shape == (len(W.RECORDINGS), 128)
            assert torch.equal(lo, ops.window_pool(win.logits, win.offsets, pool, act)) and torch.equal(fe, ops.window_pool(win.features, win.offsets, pool))
            W.check_pool(lambda *a: lo.cpu(), win.logits.cpu(), off, pool, act, what=f"logits {pool_of}", show=True)
            W.check_pool(lambda *a: fe.cpu(), win.features.cpu(), off, pool, None, what="features", show=True)


# ---- 6. chunking ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_windows_chunked(precision):
    m, x = _model("small", precision), _input("small")
    whole = {}
    for tail in ("align", "short"):
        a = whole[tail] = m.forward_windows(x, W.RECORDINGS, window=W.WINDOW, hop=100, tail=tail)
        b = m.forward_windows(x, W.RECORDINGS, window=W.WINDOW, hop=100, tail=tail, max_tokens=3 * 290)
        for k in ("offsets", "start", "length"):
            assert torch.equal(getattr(a[2], k), getattr(b[2], k))
        assert a[2].dropped == b[2].dropped
        errs = [rel(b[2].logits.cpu(), a[2].logits.cpu()), rel(b[2].features.cpu(), a[2].features.cpu()), rel(b[0].cpu(), a[0].cpu()),
                rel(b[1].cpu(), a[1].cpu())]
        print(f"chunked[{precision},{tail}]: {errs}")
        assert all(e < _lim(precision) for e in errs), errs
    c = m.forward_windows(x, W.RECORDINGS, window=W.WINDOW, hop=100, max_tokens=1)          # every window its own pass
    assert rel(c[2].logits.cpu(), whole["align"][2].logits.cpu()) < _lim(precision)


# ---- 7. the wave entry ----------------------------------------------------------------------------------------------------------------
def test_tag_equals_front_end_then_forward_windows():
    m = _model("small", "fp32")
    mel = passt_amd.AugmentMelSTFT(**V.MEL_KW).to(DEV).eval()
    keep = [i for i, n in enumerate(V.WAVE_LENGTHS) if n >= 16 * 320]
    wave = torch.from_numpy(V.wave_input())[keep]
    samples = [V.WAVE_LENGTHS[i] for i in keep]
    for i, n in enumerate(samples):
        wave[i, n:] = float("nan")
    wave = wave.to(DEV)
    a = windows.tag(mel, m, wave, lengths=samples, window_s=2.5, hop_s=1.0, tail="short", pool="max", pool_of="sigmoid")
    spec, frames = mel(wave, lengths=samples)
    assert windows.seconds_to_frames(mel, 2.5) == 250 and windows.seconds_to_frames(mel, 1.0) == 100
    b = m.forward_windows(spec[:, None], frames, window=250, hop=100, tail="short", pool="max", pool_of="sigmoid")
    assert max(np.diff(a[2].offsets.numpy())) > 1
    for p, q in zip(a[:2] + tuple(a[2][:5]), b[:2] + tuple(b[2][:5])):
        assert torch.equal(p, q)
    assert torch.isfinite(a[0]).all() and a[2].dropped == b[2].dropped


# ---- 8. no side effects; the ensemble ---------------------------------------------------------------------------------------------------
def test_forward_windows_leaves_the_other_paths_alone():
    m, x = _model("small", "fp32"), _input("small")
    xf = _input("small")[:2, :, :, :250].contiguous()
    l0, f0 = _quiet(m, xf)
    r0 = _quiet(m, x, lengths=W.RECORDINGS)
    m.forward_windows(x, W.RECORDINGS, window=W.WINDOW, hop=37, tail="short", pool="max", pool_of="sigmoid", max_tokens=1000)
    l1, f1 = _quiet(m, xf)
    r1 = _quiet(m, x, lengths=W.RECORDINGS)
    assert torch.equal(l0, l1) and torch.equal(f0, f1) and torch.equal(r0[0], r1[0]) and torch.equal(r0[1], r1[1])
    assert not m.training


def test_ensemble_windows_is_the_mean_of_its_members():
    a, b = _model("small", "fp32"), _model("small", "fp32", seed=77)
    ens = passt_amd.EnsembelerModel([a, b]).eval()
    x = _input("small")
    lo, fe, win = ens.forward_windows(x, W.RECORDINGS, hop=100, pool="mean")          # window: the members' img_size[1] = 250
    wa, wb = (mm.forward_windows(x, W.RECORDINGS, window=250, hop=100, pool=None)[2] for mm in (a, b))
    want = (wb.logits + wa.logits) / 2
    assert torch.equal(win.logits, want) and win.features is win.logits and torch.equal(win.offsets, wa.offsets)
    assert torch.equal(lo, ops.window_pool(want, wa.offsets, "mean")) and torch.equal(fe, lo)

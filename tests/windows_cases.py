"""Checkers and operands of the sliding-window entries (PaSST.forward_windows, pa_patch_gather_windows, pa_window_pool), shared by
tests/test_windows_cpu.py (plain torch implementations and fault models go through them) and tests/test_gpu_windows.py (the
kernels go through them).

  geometry   brute_windows: the window rule restated as a loop over start frames -- no closed form for the window count
  gather     ref_gather_windows: the slicing definition -- cut the window out of its recording, cut the patch out of the window
  pool       ref_pool: float64, with the bound of an f32 sum in row order.  For the mean of n terms v_k the kernel makes n - 1 f32
             additions and one division: |error| <= (n + 1) 2^-24 sum_k |v_k| / n (first order; every partial sum is below
             sum |v_k|).  The max is exact.  With act = "sigmoid" every term carries the kernel's own sigmoid error on top:
             SIGMOID_ALLOWANCE per term, so the same figure on a mean or a max of such terms.
"""
import numpy as np
import torch

from tests.row_kernel_cases import PA_BF16, PA_F32, TD  # noqa: F401

F32, F64, I32 = torch.float32, torch.float64, torch.int32

# The sigmoid's own error cannot be derived from the project: measured on an MI355X (tools/bench_windows.py, profiles/windows.txt)
# as the largest |kernel sigmoid - float64 torch.sigmoid| over sigmoid_family(): 8.890e-8; the allowance is twice that.
SIGMOID_MEASURED = 8.89043e-8
SIGMOID_ALLOWANCE = 2 * SIGMOID_MEASURED
assert SIGMOID_ALLOWANCE < 1e-6

# the small model's geometry (tests/golden/make_golden.py SMALL): patch 16, stride 10, 128 mel bins
P_, FS, TS, F_BINS = 16, 10, 10, 128
F_DIM = (F_BINS - P_) // FS + 1
RECORDINGS = [1203, 250, 437, 16, 731, 251]          # frames, in a (6, 1, 128, 1203) buffer
WINDOW = 250

# (n, window, hop, tail): n == window, window + 1, (n - window) % hop == 0 and != 0, hop 1, hop == window, n == P, n < window, a
# "short" tail of P - 1 frames (dropped) and of P frames (kept)
GEOMETRY_TABLE = [(n, w, h, tail) for tail in ("align", "short") for (n, w, h) in [
    (250, 250, 125), (251, 250, 125), (450, 250, 100), (451, 250, 100), (449, 250, 100), (1203, 250, 100), (1203, 250, 37),
    (300, 250, 1), (40, 16, 1), (750, 250, 250), (751, 250, 250), (16, 250, 100), (16, 16, 16), (100, 250, 100),
    (255, 250, 240),                                   # the last "short" window [240, 255) has P - 1 = 15 frames: dropped
    (256, 250, 240),                                   # ... and P = 16 frames: kept
    (998, 998, 499), (2400, 998, 499), (1500, 998, 499), (60000, 998, 499)]]


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def brute_windows(n, window, hop, tail, P=P_):
    """([(start, length)], [(start, length) dropped]) of one recording of n >= P frames, by walking the start frames"""
    assert n >= P
    if n <= window:
        return [(0, n)], []
    starts, s = [], 0
    while True:
        starts.append(s)
        if s + window >= n:              # this window reaches the recording's end: the last one
            break
        s += hop
    if tail == "align":
        starts[-1] = n - window
        return [(s, window) for s in starts], []
    spans = [(s, min(window, n - s)) for s in starts]
    if spans[-1][1] < P:
        return spans[:-1], spans[-1:]
    return spans, []


def covered(spans, n):
    c = np.zeros(n, dtype=bool)
    for s, m in spans:
        assert 0 <= s and s + m <= n, (s, m, n)
        c[s:s + m] = True
    return c


def check_geometry(geometry, lengths, window, hop, tail, P=P_, ts=TS, F_dim=F_DIM):
    """``geometry(lengths, window, hop, tail, P, ts, F_dim)`` (window_geometry's contract) against the brute-force rule: the window
    arrays, the coverage property, and every token row of the packed batch"""
    g = geometry(lengths, window, hop, tail, P, ts, F_dim)
    src, t0, ln, dropped, offsets = [], [], [], [], [0]
    for b, n in enumerate(lengths):
        spans, gone = brute_windows(n, window, hop, tail, P)
        cov = covered(spans, n)
        if tail == "align":
            assert cov.all(), (b, n)
            assert all(m == min(window, n) for _, m in spans)
        else:
            lo = min([s for s, _ in gone], default=n)
            assert cov[:lo].all(), (b, n)                 # only frames of the dropped tail may be left out
        src += [b] * len(spans)
        t0 += [s for s, _ in spans]
        ln += [m for _, m in spans]
        dropped += [(b, s, m) for s, m in gone]
        offsets.append(len(src))
    assert g["win_src"].tolist() == src and g["win_t0"].tolist() == t0 and g["win_len"].tolist() == ln, (lengths, window, hop, tail)
    assert all(g[k].dtype == np.int32 for k in ("win_src", "win_t0", "win_len", "row_clip", "row_f", "row_t", "cu_tok"))
    assert np.asarray(g["offsets"]).tolist() == offsets and list(g["dropped"]) == dropped
    # token rows: window w owns cls, dist and its F_dim x T_w patches, frequency-major
    row_w, row_f, row_t, cu = [], [], [], [0]
    for w, m in enumerate(ln):
        T = (m - P) // ts + 1
        row_w += [w] * (2 + F_dim * T)
        row_f += [-1, -1] + [f for f in range(F_dim) for _ in range(T)]
        row_t += [0, 1] + [t for _ in range(F_dim) for t in range(T)]
        cu.append(len(row_w))
    assert g["row_clip"].tolist() == row_w and g["row_f"].tolist() == row_f and g["row_t"].tolist() == row_t
    assert g["cu_tok"].tolist() == cu and g["max_N"] == max(np.diff(cu))
    return g


# ---- gather -------------------------------------------------------------------------------------------------------------------
def code_x(B, F, T, dt):
    """recordings of distinct integers (f32: every element its own value below 2^24; bf16: |v| <= 256, neighbours in time, in
    frequency and across recordings differ)"""
    if dt == PA_F32:
        assert B * F * T < 2 ** 24
        return (torch.arange(B * F * T, dtype=F32) + 1).view(B, 1, F, T)
    b, f, t = torch.arange(B)[:, None, None], torch.arange(F)[None, :, None], torch.arange(T)[None, None, :]
    return (((b * 89 + f * 37 + t) % 513) - 256).to(F32).view(B, 1, F, T)


def nan_behind(x, lengths, fill=float("nan")):
    x = x.clone()
    for b, n in enumerate(lengths):
        x[b, :, :, n:] = fill
    return x


def ref_gather_windows(x, win_src, win_t0, win_len, row_win, row_f, row_t, P=P_, fs=FS, ts=TS):
    """cols (M, P*P) f32 by slicing: the window out of its recording, the patch out of the window; a prefix row is zero.  x: (B, 1, F, T)"""
    M = len(row_f)
    cols = torch.zeros(M, P * P, dtype=F32)
    for r in range(M):
        w, f, t = int(row_win[r]), int(row_f[r]), int(row_t[r])
        if f < 0:
            continue
        s, m = int(win_t0[w]), int(win_len[w])
        window = x[int(win_src[w]), 0, :, s:s + m]
        patch = window[f * fs:f * fs + P, t * ts:t * ts + P]
        assert patch.shape == (P, P), "the geometry asked for a patch that leaves its window"
        cols[r] = patch.reshape(-1)
    return cols


def check_gather(impl, x, g, dt, P=P_, fs=FS, ts=TS, what=""):
    """``impl(x, win_src, win_t0, win_len, row_win, row_f, row_t, P, fs, ts, dt)`` -> cols (CPU, TD[dt]) against the slicing definition,
    bit for bit (the operands are exact in dt); NaN behind a length must not show"""
    got = impl(x, g["win_src"], g["win_t0"], g["win_len"], g["row_clip"], g["row_f"], g["row_t"], P, fs, ts, dt)
    want = ref_gather_windows(x, g["win_src"], g["win_t0"], g["win_len"], g["row_clip"], g["row_f"], g["row_t"], P, fs, ts).to(TD[dt])
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype)
    assert not torch.isnan(want).any(), "the definition itself read behind a length"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r = int(bad[0, 0])
        raise AssertionError(f"{what}: {bad.shape[0]} elements differ, first in row {r} (window {int(g['row_clip'][r])}, f {int(g['row_f'][r])}, "
                             f"t {int(g['row_t'][r])}) at {int(bad[0, 1])}: got {float(got[r, bad[0, 1]])}, want {float(want[r, bad[0, 1]])}")
    prefix = torch.from_numpy(np.asarray(g["row_f"]) < 0)
    assert not got[prefix].float().abs().sum().item(), f"{what}: a prefix row is not zero"
    return got


def unfold(x, g):
    """the explicit copies: (W, 1, F, max length), window w in its first win_len[w] frames, NaN behind"""
    W, L = len(g["win_src"]), int(max(g["win_len"]))
    u = torch.full((W, 1, x.shape[2], L), float("nan"), dtype=x.dtype)
    for w in range(W):
        s, m = int(g["win_t0"][w]), int(g["win_len"][w])
        u[w, 0, :, :m] = x[int(g["win_src"][w]), 0, :, s:s + m]
    return u


# ---- pool ---------------------------------------------------------------------------------------------------------------------
def sigmoid_family():
    """the logits the sigmoid is measured over: a dense sweep of [-30, 30], the values around 0 and the saturating ends"""
    sweep = torch.linspace(-30.0, 30.0, 240001, dtype=F32)
    ends = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 1e-8, 20.0, -20.0, 87.0, -87.0, 88.0, -88.0, 100.0, -100.0, 104.0, -104.0, 1e4, -1e4], dtype=F32)
    return torch.cat([sweep, ends])


def pool_rows(W, C, seed, negative=False):
    """per-window rows: logits-like values in about [-12, 12] (sigmoid_family's range), all below zero when asked"""
    g = torch.Generator().manual_seed(1000 + seed)
    v = torch.randn(W, C, generator=g, dtype=F32) * 4.0
    return -v.abs() - 0.25 if negative else v


POOL_CASES = [                       # (offsets, C)
    ([0, 13, 14, 19, 20, 28, 30], 37),       # the small case's window counts (hop 100): single-window recordings among them
    ([0, 1], 1), ([0, 1, 2, 3], 5), ([0, 120], 527), ([0, 3, 4, 300], 257)]


def ref_pool(rows, offsets, mode, act):
    """(want f64 (B, C), bound (B, C)) of pa_window_pool"""
    v = rows.to(F64)
    if act == "sigmoid":
        v = torch.sigmoid(v)
    want, bound = [], []
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        lo, hi = int(lo), int(hi)
        assert hi > lo
        seg, n = v[lo:hi], hi - lo
        if mode == "max":
            want.append(seg.max(dim=0).values)
            bound.append(torch.zeros(v.shape[1], dtype=F64))
        else:
            want.append(seg.sum(dim=0) / n)
            bound.append((n + 1) * 2.0 ** -24 * seg.abs().sum(dim=0) / n if n > 1 else torch.zeros(v.shape[1], dtype=F64))
        if act == "sigmoid":
            bound[-1] = bound[-1] + SIGMOID_ALLOWANCE
    return torch.stack(want), torch.stack(bound)


def check_pool(impl, rows, offsets, mode, act, what="", show=False):
    """``impl(rows, offsets, mode, act)`` -> (B, C) f32 on the CPU against the float64 reference within the derived bound; a recording
    with a single window returns that row exactly (act None).  Returns the worst error / bound ratio."""
    got = impl(rows, offsets, mode, act)
    want, bound = ref_pool(rows, offsets, mode, act)
    assert got.shape == want.shape and got.dtype == F32, (what, got.shape, got.dtype)
    err = (got.to(F64) - want).abs()
    if show:
        print(f"{what} {mode}/{act}: worst error {float(err.max()):.3e}, worst bound {float(bound.max()):.3e}")
    over = err > bound
    assert not over.any(), (f"{what} {mode}/{act}: {int(over.sum())} outputs over the bound, first {over.nonzero()[0].tolist()}: error "
                            f"{float(err[over][0]):.3e} bound {float(bound[over][0]):.3e}")
    if act is None:
        for b, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
            if hi - lo == 1:
                assert torch.equal(got[b], rows[int(lo)]), f"{what}: recording {b} has one window and does not return its row"
    return float((err / bound.clamp_min(1e-300)).max())


# ---- the entries in plain torch (the CPU tests run the checkers on these; the fault models override one method each) ----------------
class TorchWindows:
    def geometry(self, lengths, window, hop, tail, P, ts, F_dim):
        from passt_amd.passt import window_geometry
        return window_geometry(lengths, window, hop, tail, P, ts, F_dim)

    # gather
    def first_frame(self, t0, ts):
        return t0

    def recording(self, w, win_src):
        return int(win_src[w])

    def gather(self, x, win_src, win_t0, win_len, row_win, row_f, row_t, P, fs, ts, dt):
        B, _, F, T = x.shape
        M = len(row_f)
        cols = torch.zeros(M, P * P, dtype=F32)
        i, j = torch.arange(P)[:, None], torch.arange(P)[None, :]
        for r in range(M):
            w, f = int(row_win[r]), int(row_f[r])
            if f < 0:
                continue
            t0, n = self.first_frame(int(win_t0[w]), ts), int(win_len[w])
            ff, dtm = f * fs + i, int(row_t[r]) * ts + j
            ok = (ff < F) & (dtm < n) & (t0 + dtm < T)
            v = x[self.recording(w, win_src), 0][ff.clamp(max=F - 1).expand(P, P), (t0 + dtm).clamp(max=T - 1).expand(P, P)]
            cols[r] = torch.where(ok.expand(P, P), v, torch.zeros(())).reshape(-1)
        return cols.to(TD[dt])

    # pool
    def sigmoid(self, v):
        """the kernel's: exp(-z) rounded to f32 once from f64, an f32 add, an f32 division"""
        return 1.0 / (1.0 + torch.exp(-v.to(F64)).to(F32))

    def count(self, lo, hi, offsets):
        return hi - lo

    def last_row(self, hi):
        return hi

    def max_start(self, first):
        return first

    def pool(self, rows, offsets, mode, act):
        out = []
        for lo, hi in zip(offsets[:-1], offsets[1:]):
            lo, hi = int(lo), int(hi)
            seg = rows[lo:min(self.last_row(hi), rows.shape[0])]
            if act == "sigmoid":
                seg = self.sigmoid(seg)
            acc = self.max_start(seg[0]) if mode == "max" else seg[0]
            for k in range(1, seg.shape[0]):
                acc = torch.maximum(acc, seg[k]) if mode == "max" else acc + seg[k]
            if mode == "max":
                acc = torch.maximum(acc, seg[0])
            out.append(acc if mode == "max" else acc / float(self.count(lo, hi, offsets)))
        return torch.stack(out)

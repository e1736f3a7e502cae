"""Shapes, inputs and checkers of the row-kernel parity suite (LayerNorm, head, losses, partial-sum reductions).

Used by tests/test_gpu_row_kernels.py (the HIP kernels, through the C ABI) and tests/test_row_kernels_cpu.py (the same checkers
run against a plain f32 torch implementation: every bound below is one an honest f32 implementation meets).  A checker takes an
`impl` object -- `TorchF32` here, `Hip` in the GPU file -- hands it CPU tensors and gets CPU tensors back; it neither knows nor
cares where the arithmetic ran.  Three techniques:

  guarded buffers   every kernel input is a view into a larger allocation whose GUARD elements (at least one whole row) on
                    either side hold NaN, every output a view into an allocation filled with a finite SENTINEL no result can
                    equal.  An access one row off stays inside a live allocation, so nothing can fault: a read past the last
                    row turns the result into NaN, a write past the end breaks a guard, an element the header promises but the
                    kernel skips keeps the sentinel.
  exact sums        tensors of small integers (exact in bf16 and f32) whose every partial sum stays below 2^24: an f32
                    reduction of them is exact in ANY order, so the check is torch.equal against an int64 sum, no tolerance.
                    A dropped, doubled or misattributed row cannot hide in rounding.
  per-row metrics   max_d |got - ref| / max_d |ref| per row, then the worst row; the random inputs give row m the scale
                    2^(m mod 7 - 3), so a wrong small row is not hidden behind a large one.
"""
import math

import torch
import torch.nn.functional as F

PA_F32, PA_BF16 = 0, 1
PA_EUNSUPPORTED = -2
TD = {PA_F32: torch.float32, PA_BF16: torch.bfloat16}
REDUCE_SLABS, REDUCE_ROWS = 0, 1

GUARD = 256
SENTINEL = -1.5 * 2.0 ** 100      # finite, exact in bf16 and f32, no integer sum or normalised value comes near it
EXACT_LIMIT = 2 ** 24

# ---- shape lists ---------------------------------------------------------------------------------------------------------
# LayerNorm widths: kernel instances 1, 2, 3, 4 and 8 float4 per lane, each with a full and a partly filled last vector column
LN_D = (4, 128, 256, 260, 384, 512, 516, 768, 1020, 1024, 1028, 1280, 2048)
LN_D_ROWS = 37
# LayerNorm row counts at D = 128 and the backward workgroups (= partial rows) each must give
LN_M_WORKGROUPS = {1: 1, 3: 1, 5: 1, 128: 16, 136: 17, 512: 64, 520: 65, 8200: 1024}
LN_M_WIDTH = 128
LN_EXACT = [(M, D) for M in (5, 520, 8200) for D in (260, 768)]
LN_CONDITIONING = ((300.0, 0.5), (-1000.0, 2.0), (0.0, 1e-3))
LN_CONDITIONING_SHAPES = ((37, 260), (37, 768))
LN_CONSTANT_D = (260, 768, 2048)
HEAD_SHAPES = ((1, 2, 64), (5, 3, 768), (3, 9, 1024), (2, 4, 1100), (2, 2, 2048))
HEAD_FWD_ONLY = (3, 3, 130)
LINEAR_SHAPES = ((1, 1, 64), (5, 3, 68), (13, 50, 1024), (7, 37, 1100), (64, 527, 768))
BCE_SHAPES = ((1, 1), (5, 51), (16, 16), (1, 257), (64, 527), (130, 527))      # B * C = 1, 255, 256, 257, 64*527, 130*527
BCE_EXTREME = (0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4)
CE_SHAPES = ((1, 2), (4, 64), (5, 65), (13, 527), (12, 50))
# slab lengths; the last needs two trips of the 4096 workgroups pa_reduce_partials launches at most
SLAB_SPLITS, SLAB_N = (1, 2, 7), (1, 3, 4, 5, 1027, 768 * 768, 4096 * 256 + 5)
ROWS_SPLITS, ROWS_N = (1, 15, 16, 17, 63, 64, 65, 1024), (1, 16, 17, 768)
ROWS_WIDE = (17, 40000)           # more than 2048 * 16 columns: a second trip of the capped grid
COLSUM_F32_R, COLSUM_F32_C = (1, 3, 4, 13, 16, 17, 100), (1, 64, 65, 527)
COLSUM_R, COLSUM_C = (1, 255, 256, 257, 8193, 33 * 256), (8, 72, 768)
ROWSUM_C, ROWSUM_R = (1, 63, 64, 65, 1000), (1, 5)


def ln_instance(D):
    """float4 per lane of the LayerNorm kernel instance that runs width D"""
    nvl = -(-D // 256)
    return nvl if nvl <= 4 else 8


def ln_bwd_workgroups(M):
    """documented launch geometry of the LayerNorm backward: two rows per wave, four waves, at most 1024 workgroups"""
    return max(1, min(1024, -(-M // 8)))


# ---- guarded buffers -----------------------------------------------------------------------------------------------------
def guard_elems(shape):
    """GUARD elements, or one whole row where that is more: an access one row past the end stays inside the allocation"""
    return max(GUARD, int(shape[-1]) if len(shape) else 1)


def guarded_in(t, device, offset=0):
    """`t` on `device` as a view into a larger allocation; NaN in front of and behind it (0 for integer tensors, a valid index).
    offset: extra elements in front, to take the view off 16-byte alignment."""
    if t is None:
        return None
    n, guard = t.numel(), guard_elems(t.shape)
    buf = torch.empty(guard + offset + n + guard, dtype=t.dtype, device=device)
    buf.fill_(float("nan") if t.is_floating_point() else 0)
    view = buf[guard + offset:guard + offset + n].view(t.shape)
    view.copy_(t)
    return view


class GuardedOut:
    """An output view with GUARD (at least one row of) sentinel elements on both sides.  init: start values (accumulate), else
    the view holds the sentinel too, so an element that was never written shows."""

    def __init__(self, shape, dtype, device, init=None, offset=0):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        n, guard = int(math.prod(shape)), guard_elems(shape)
        self.buf = torch.full((guard + offset + n + guard,), SENTINEL, dtype=dtype, device=device)
        self.lo, self.n = guard + offset, n
        self.view = self.buf[self.lo:self.lo + n].view(shape)
        if init is not None:
            self.view.copy_(init)

    def ptr(self):
        return self.view.data_ptr()

    def take(self, what, written=None):
        """the result on the CPU, after the guard check.  written: number of leading elements that must have been written
        (default all of them)"""
        buf = self.buf.cpu()
        front, back = buf[:self.lo], buf[self.lo + self.n:]
        assert bool((front == SENTINEL).all()), f"{what}: a write in front of the output"
        assert bool((back == SENTINEL).all()), f"{what}: a write behind the output"
        flat = buf[self.lo:self.lo + self.n]
        w = self.n if written is None else written
        assert not bool((flat[:w] == SENTINEL).any()), f"{what}: elements the kernel never wrote"
        assert bool((flat[w:] == SENTINEL).all()), f"{what}: a write past the promised extent"
        return flat.view(self.view.shape).clone()


# ---- inputs --------------------------------------------------------------------------------------------------------------
def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def randn(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def row_scales(M):
    """2^(m mod 7 - 3): exact scalings, so bf16 rounding commutes with them"""
    return (2.0 ** ((torch.arange(M) % 7) - 3).float())[:, None]


def small_ints(*shape, seed=0, lo=-8, hi=8, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def exact_sum_safe(t, dim):
    """every partial sum of `t` along `dim`, in any order, stays below 2^24 in magnitude"""
    return float(t.double().abs().sum(dim).max()) < EXACT_LIMIT


def int_sum(t, dim):
    return t.double().sum(dim).float()        # integers below 2^24: the f64 sum is the exact one and fits f32


def padded(t, ld, fill=float("nan")):
    """[R][C] -> [R][ld] with NaN in the columns a kernel must not read"""
    R, C = t.shape
    out = torch.full((R, ld), fill, dtype=t.dtype)
    out[:, :C] = t
    return out


# ---- metrics -------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def row_err(got, ref):
    """max over rows of max_d |got - ref| / max_d |ref|; a NaN anywhere gives inf"""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    e = (got - ref).abs().amax(1) / (ref.abs().amax(1) + 1e-30)
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    return float(e.max())


def elem_rel(got, ref):
    got, ref = got.double(), ref.double()
    e = (got - ref).abs() / (ref.abs() + 1e-30)
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    return float(e.max())


def _rec(rec, name, **figs):
    if rec is not None:
        rec(name, **figs)


def f32_eps(eps):
    return float(torch.tensor(eps, dtype=torch.float32))     # what the kernel receives


# ---- f64 references ------------------------------------------------------------------------------------------------------
def ln_reference(x, g, b, eps, dy, dres=None, dres2=None):
    D = x.shape[1]
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, g, b))
    y = F.layer_norm(xr, (D,), gr, br, f32_eps(eps))
    y.backward(dy.double())
    dx = xr.grad.clone()
    for a in (dres, dres2):
        if a is not None:
            dx = dx + a.double()
    xd = x.double()
    return dict(y=y.detach(), mean=xd.mean(1), rstd=(xd.var(1, unbiased=False) + f32_eps(eps)).rsqrt(), dx=dx, dg=gr.grad, db=br.grad,
                dcol=dx.sum(0))


def head_reference(x, ng, nb, hg, hb, dhn, dfeat, eps_n=1e-6, eps_h=1e-5):
    D = x.shape[2]
    leaf = [t.double().requires_grad_(True) for t in (x, ng, nb, hg, hb)]
    xn = F.layer_norm(leaf[0][:, :2], (D,), leaf[1], leaf[2], f32_eps(eps_n))
    feat = (xn[:, 0] + xn[:, 1]) / 2
    hn = F.layer_norm(feat, (D,), leaf[3], leaf[4], f32_eps(eps_h))
    obj = (hn * dhn.double()).sum()
    if dfeat is not None:
        obj = obj + (feat * dfeat.double()).sum()
    obj.backward()
    xd, fd = x.double(), feat.detach()
    stats = torch.stack([xd[:, 0].mean(1), (xd[:, 0].var(1, unbiased=False) + f32_eps(eps_n)).rsqrt(),
                         xd[:, 1].mean(1), (xd[:, 1].var(1, unbiased=False) + f32_eps(eps_n)).rsqrt(),
                         fd.mean(1), (fd.var(1, unbiased=False) + f32_eps(eps_h)).rsqrt()], 1)
    return dict(feat=fd, hn=hn.detach(), stats=stats, dx=leaf[0].grad, dng=leaf[1].grad, dnb=leaf[2].grad, dhg=leaf[3].grad,
                dhb=leaf[4].grad)


def ce_reference(z, t, t2, lam, scale, dtype=torch.float64):
    zr = z.detach().clone().to(dtype).requires_grad_(True)
    if t2 is None:
        loss = F.cross_entropy(zr, t.long())
    else:
        loss = (F.cross_entropy(zr, t.long(), reduction="none") * lam.to(dtype)
                + F.cross_entropy(zr, t2.long(), reduction="none") * (1 - lam.to(dtype))).mean()
    (loss * scale).backward()
    return loss.detach(), zr.grad


def bce_reference(z, y, scale, dtype=torch.float64):
    zr = z.detach().clone().to(dtype).requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(zr, y.to(dtype), reduction="none").mean()
    (loss * scale).backward()
    return loss.detach(), zr.grad


# ---- the plain f32 torch implementation ----------------------------------------------------------------------------------
class TorchF32:
    """Every operation of the suite in plain f32 torch on the CPU, with the kernels' calling conventions: the self-check of the
    checkers and the baseline behind the measured tolerances."""
    name = "torch_f32"

    def ln_fwd(self, x, g, b, eps, dt):
        y = F.layer_norm(x, (x.shape[1],), g, b, f32_eps(eps))
        return y.to(TD[dt]), x.mean(1), (x.var(1, unbiased=False) + f32_eps(eps)).rsqrt()

    def ln_bwd(self, dy, x, g, mean, rstd, dres, dres2, dt, eps=1e-6, partial=False, accumulate=False, start=None, want_dcol=True):
        xr, gr = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
        br = torch.zeros_like(g).requires_grad_(True)
        F.layer_norm(xr, (x.shape[1],), gr, br, f32_eps(eps)).backward(dy.float())
        dx = xr.grad
        for a in (dres, dres2):
            if a is not None:
                dx = dx + a
        dg, db, dcol = gr.grad, br.grad, dx.sum(0)
        if accumulate:
            dg, db, dcol = start[0] + dg, start[1] + db, start[2] + dcol
        return dict(dx=dx, dx_lp=dx.to(TD[dt]), dg=dg, db=db, dcol=dcol if want_dcol else None)

    def head_fwd(self, x, ng, nb, hg, hb, eps_n=1e-6, eps_h=1e-5):
        D = x.shape[2]
        xn = F.layer_norm(x[:, :2], (D,), ng, nb, f32_eps(eps_n))
        feat = (xn[:, 0] + xn[:, 1]) / 2
        hn = F.layer_norm(feat, (D,), hg, hb, f32_eps(eps_h))
        st = [x[:, 0].mean(1), (x[:, 0].var(1, unbiased=False) + f32_eps(eps_n)).rsqrt(), x[:, 1].mean(1),
              (x[:, 1].var(1, unbiased=False) + f32_eps(eps_n)).rsqrt(), feat.mean(1), (feat.var(1, unbiased=False) + f32_eps(eps_h)).rsqrt()]
        return feat, hn, torch.stack(st, 1)

    def head_bwd(self, dhn, dfeat, x, feat, ng, hg, stats, eps_n=1e-6, eps_h=1e-5):
        D = x.shape[2]
        xr = x.clone().requires_grad_(True)
        xn = F.layer_norm(xr[:, :2], (D,), ng, torch.zeros_like(ng), f32_eps(eps_n))
        fr = (xn[:, 0] + xn[:, 1]) / 2
        fr = fr + (feat - fr.detach())          # the norm's bias is not an argument of the backward: the saved feat carries it
        fr.retain_grad()
        hn = F.layer_norm(fr, (D,), hg, torch.zeros_like(hg), f32_eps(eps_h))
        obj = (hn * dhn).sum()
        if dfeat is not None:
            obj = obj + (fr * dfeat).sum()
        obj.backward()
        s = stats
        xh = (feat - s[:, 4:5]) * s[:, 5:6]
        dy = 0.5 * fr.grad
        xa, xb = (x[:, 0] - s[:, 0:1]) * s[:, 1:2], (x[:, 1] - s[:, 2:3]) * s[:, 3:4]
        part = torch.stack([dhn * xh, dhn, dy * (xa + xb), 2 * dy], 1)
        return xr.grad, part

    def head_bwd_rc(self, *a):
        return None                            # no error codes here

    def linear_fwd(self, x, W, b):
        return F.linear(x, W, b)

    def linear_bwd(self, dy, x, W, accumulate=False, start=None, want_dw=True):
        dx = dy @ W
        if not want_dw:
            return dx, None, None
        dW, db = dy.t() @ x, dy.sum(0)
        if accumulate:
            dW, db = start[0] + dW, start[1] + db
        return dx, dW, db

    def bce(self, z, y, scale):
        loss, dz = bce_reference(z, y, scale, torch.float32)
        return loss.reshape(1), dz

    def ce(self, z, t, t2, lam, scale):
        loss, dz = ce_reference(z, t, t2, lam, scale, torch.float32)
        return loss.reshape(1), dz

    def reduce(self, descs, single=False, offsets=None):
        outs = []
        for d in descs:
            p = d["partial"]
            s = p.sum(0) if d["mode"] == REDUCE_SLABS else p[:, :d["n"]].sum(0)
            outs.append((d["start"] + s) if d["accumulate"] else s)
        return outs

    def colsum_f32(self, a, C, accumulate, start):
        s = a[:, :C].sum(0)
        return start + s if accumulate else s

    def colsum(self, a, C, dt, accumulate, start):
        s = a[:, :C].float().sum(0)
        return start + s if accumulate else s

    def colsum_rc(self, *a):
        return None

    def rowsum(self, a, C, dt, accumulate, start):
        s = a[:, :C].float().sum(1)
        return start + s if accumulate else s


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------
LN_TOL = {PA_F32: dict(fwd=1e-5, lp=0.0), PA_BF16: dict(fwd=6e-3, lp=5e-3)}
LN_BWD_TOL = 2e-5


def ln_inputs(M, D, dt, seed=100):
    sc = row_scales(M)
    return dict(x=(rnd(M, D, seed=seed, scale=3.0) + 0.5) * sc, g=rnd(D, seed=seed + 1) * 0.3 + 1, b=rnd(D, seed=seed + 2),
                dy=(rnd(M, D, seed=seed + 3) * sc).to(TD[dt]), dres=rnd(M, D, seed=seed + 4) * sc,
                dres2=rnd(M, D, seed=seed + 5, scale=2.0) * sc, start=rnd(3, D, seed=seed + 6, scale=4.0))


def _ln_bwd_figures(out, ref, start, accumulate, want_dcol):
    off = start.double() if accumulate else torch.zeros(3, ref["dg"].numel(), dtype=torch.float64)
    figs = dict(dx=row_err(out["dx"], ref["dx"]), dgamma=rel_err(out["dg"], ref["dg"] + off[0]), dbeta=rel_err(out["db"], ref["db"] + off[1]),
                lp=row_err(out["dx_lp"], out["dx"]))
    if want_dcol:
        figs["dcol"] = rel_err(out["dcol"], ref["dcol"] + off[2])
    else:
        assert out["dcol"] is None
    return figs


def check_layernorm(impl, M, D, dt, rec=None):
    """forward, then every backward entry (full / partial, one / two addends) with dres NULL and given, dcolsum NULL and given,
    accumulate 0 and 1; f64 layer_norm and its autograd on the same f32 / bf16-rounded inputs"""
    i = ln_inputs(M, D, dt)
    x, g, b, dy, start = i["x"], i["g"], i["b"], i["dy"], i["start"]
    y, mean, rstd = impl.ln_fwd(x, g, b, 1e-6, dt)
    worst = {}
    refs = {}

    def ref_for(dres, dres2):
        k = (dres is not None, dres2 is not None)
        if k not in refs:
            refs[k] = ln_reference(x, g, b, 1e-6, dy, dres, dres2)
        return refs[k]

    r0 = ref_for(i["dres"], None)
    fwd = dict(fwd=row_err(y, r0["y"]), mean=float(((mean.double() - r0["mean"]).abs() / x.double().abs().amax(1)).max()),
               rstd=elem_rel(rstd, r0["rstd"]))
    worst.update(fwd)
    assert fwd["fwd"] < LN_TOL[dt]["fwd"], fwd
    assert fwd["mean"] < 1e-5 and fwd["rstd"] < 1e-5, fwd
    #           dres        dres2       partial accumulate dcol
    variants = ((i["dres"], None,       False,  False,     True),
                (None,      None,       False,  True,      False),
                (i["dres"], None,       True,   False,     True),
                (i["dres"], i["dres2"], False,  True,      True),
                (None,      i["dres2"], True,   False,     True),
                (i["dres"], i["dres2"], True,   True,      False))
    outs = []
    for dres, dres2, partial, acc, dcol in variants:
        out = impl.ln_bwd(dy, x, g, mean, rstd, dres, dres2, dt, partial=partial, accumulate=acc, start=start, want_dcol=dcol)
        outs.append(out)
        figs = _ln_bwd_figures(out, ref_for(dres, dres2), start, acc, dcol)
        for k, v in figs.items():
            worst[k] = max(worst.get(k, 0.0), v)
        tag = (dres is not None, dres2 is not None, partial, acc, dcol)
        assert max(figs["dx"], figs["dgamma"], figs["dbeta"], figs.get("dcol", 0.0)) < LN_BWD_TOL, (tag, figs)
        if dt == PA_F32:
            assert torch.equal(out["dx_lp"], out["dx"]), tag          # the f32 "copy" is the same value
        else:
            assert figs["lp"] < LN_TOL[dt]["lp"], (tag, figs)
    # the partial form finished with the ROWS reduction against the full form: the same rows, the same kernel
    full, part = outs[0], outs[2]
    assert torch.equal(full["dx"], part["dx"]) and torch.equal(full["dx_lp"], part["dx_lp"])
    pf = max(rel_err(part[k], full[k]) for k in ("dg", "db", "dcol"))
    worst["partial_vs_full"] = pf
    assert pf < LN_BWD_TOL, pf
    _rec(rec, f"layernorm[{dt},{M},{D}]", **worst)
    return worst


def check_ln_exact(impl, M, D, dt, rec=None):
    """(a) dy = 0 with integer addends: dx = dres + dres2 exactly, dx_lp its exact cast, dcolsum the exact integer column sum,
    dgamma = dbeta = 0 on top of their integer start values.  (b) integer dy: dbeta the exact integer column sum.
    Full and partial forms, accumulate on integer start values: a dropped, doubled or misattributed row changes an integer."""
    x, g = (rnd(M, D, seed=200, scale=3.0) + 0.5) * row_scales(M), rnd(D, seed=201) * 0.3 + 1
    _, mean, rstd = impl.ln_fwd(x, g, torch.zeros(D), 1e-6, dt)
    dres, dres2 = small_ints(M, D, seed=202), small_ints(M, D, seed=203)
    start = small_ints(3, D, seed=204, lo=-50, hi=50)
    want = dres + dres2
    assert exact_sum_safe(want, 0) and exact_sum_safe(torch.cat([want, start[2:3]]), 0)
    zero = torch.zeros(M, D, dtype=TD[dt])
    for partial in (False, True):
        for acc in (True, False):
            o = impl.ln_bwd(zero, x, g, mean, rstd, dres, dres2, dt, partial=partial, accumulate=acc, start=start, want_dcol=True)
            s = start if acc else torch.zeros_like(start)
            tag = ("a", partial, acc)
            assert torch.equal(o["dx"], want), tag
            assert torch.equal(o["dx_lp"].float(), want.to(TD[dt]).float()), tag
            assert torch.equal(o["dcol"], s[2] + int_sum(want, 0)), tag
            assert torch.equal(o["dg"], s[0]) and torch.equal(o["db"], s[1]), tag
    dy = small_ints(M, D, seed=205, lo=-4, hi=4)
    assert exact_sum_safe(torch.cat([dy, start[1:2]]), 0)
    for partial in (False, True):
        for dr2 in (None, dres2):
            o = impl.ln_bwd(dy.to(TD[dt]), x, g, mean, rstd, None, dr2, dt, partial=partial, accumulate=True, start=start, want_dcol=True)
            assert torch.equal(o["db"], start[1] + int_sum(dy, 0)), ("b", partial, dr2 is not None)
            assert bool(torch.isfinite(o["dx"]).all())
    _rec(rec, f"layernorm_exact[{dt},{M},{D}]", mismatches=0)


def check_ln_conditioning(impl, c, sigma, M, D, rec=None, baseline=None):
    """rows x = c + sigma n.  The bound is measured: 4x the error of torch's own f32 CPU layer_norm (forward and autograd) against
    f64 on the same inputs, floor 4 * 2^-23 -- a different but equally legitimate summation order, not E[x^2] - mean^2."""
    baseline = baseline or TorchF32()
    x = c + sigma * randn(M, D, seed=300)
    g, b, dy = rnd(D, seed=301) * 0.3 + 1, rnd(D, seed=302), rnd(M, D, seed=303)
    ref = ln_reference(x, g, b, 1e-6, dy)

    def figures(im):
        y, mean, rstd = im.ln_fwd(x, g, b, 1e-6, PA_F32)
        o = im.ln_bwd(dy, x, g, mean, rstd, None, None, PA_F32, want_dcol=False)
        return dict(fwd=row_err(y, ref["y"]), rstd=elem_rel(rstd, ref["rstd"]), dx=row_err(o["dx"], ref["dx"]),
                    dgamma=rel_err(o["dg"], ref["dg"]), dbeta=rel_err(o["db"], ref["db"]))
    base, got = figures(baseline), figures(impl)
    floor = 4 * 2.0 ** -23
    tol = {k: max(4 * v, floor) for k, v in base.items()}
    _rec(rec, f"layernorm_conditioning[{c:g},{sigma:g},{M},{D}]", **{k: v for k, v in got.items()},
         **{"torch_f32_" + k: v for k, v in base.items()})
    for k in got:
        assert got[k] <= tol[k], (k, got[k], "torch f32:", base[k], "allowed:", tol[k])
    return got, base


def check_ln_constant_rows(impl, D, rec=None):
    """variance 0: y = beta bit for bit, rstd = eps^-1/2 to 2 ulp, a finite backward"""
    consts = torch.tensor([3.0, -7.0, 0.0, 1024.0, 0.5])
    M = consts.numel()
    x = consts[:, None].expand(M, D).contiguous()
    assert exact_sum_safe(x, 1)
    g, b, dy = rnd(D, seed=311) * 0.3 + 1, rnd(D, seed=312), rnd(M, D, seed=313)
    want = 1.0 / math.sqrt(f32_eps(1e-6))
    ulp = 2.0 ** (math.floor(math.log2(want)) - 23)
    for dt in (PA_F32, PA_BF16):
        y, mean, rstd = impl.ln_fwd(x, g, b, 1e-6, dt)
        assert torch.equal(y, b.to(TD[dt]).expand(M, D)), dt
        assert torch.equal(mean, consts)
        e = float((rstd.double() - want).abs().max()) / ulp
        assert e <= 2.0, e
        o = impl.ln_bwd(dy.to(TD[dt]), x, g, mean, rstd, None, None, dt, want_dcol=True)
        for k in ("dx", "dg", "db", "dcol"):
            assert bool(torch.isfinite(o[k]).all()), (dt, k)
        _rec(rec, f"layernorm_constant_rows[{dt},{D}]", rstd_ulp=e)


# ---- head ----------------------------------------------------------------------------------------------------------------
def head_inputs(B, Ntok, D, seed=400):
    sc = row_scales(B)[:, :, None]
    return dict(x=rnd(B, Ntok, D, seed=seed, scale=2.0) * sc, ng=rnd(D, seed=seed + 1) * 0.3 + 1, nb=rnd(D, seed=seed + 2),
                hg=rnd(D, seed=seed + 3) * 0.3 + 1, hb=rnd(D, seed=seed + 4), dhn=rnd(B, D, seed=seed + 5) * sc[:, 0],
                dfeat=rnd(B, D, seed=seed + 6) * sc[:, 0])


def check_head_fwd(impl, B, Ntok, D, rec=None):
    i = head_inputs(B, Ntok, D)
    feat, hn, stats = impl.head_fwd(i["x"], i["ng"], i["nb"], i["hg"], i["hb"])
    ref = head_reference(i["x"], i["ng"], i["nb"], i["hg"], i["hb"], i["dhn"], None)
    xd = i["x"].double()
    mags = torch.stack([xd[:, 0].abs().amax(1), xd[:, 1].abs().amax(1), ref["feat"].abs().amax(1)], 1)
    figs = dict(feat=row_err(feat, ref["feat"]), hn=row_err(hn, ref["hn"]),
                mean=float(((stats[:, 0::2].double() - ref["stats"][:, 0::2]).abs() / mags).max()),
                rstd=elem_rel(stats[:, 1::2], ref["stats"][:, 1::2]))
    _rec(rec, f"head_fwd[{B},{Ntok},{D}]", **figs)
    assert figs["feat"] < 1e-5 and figs["hn"] < 1e-5 and figs["mean"] < 1e-5 and figs["rstd"] < 1e-5, figs
    return i, feat, hn, stats


def check_head(impl, B, Ntok, D, rec=None):
    i, feat, hn, stats = check_head_fwd(impl, B, Ntok, D, rec)
    for dfeat in (None, i["dfeat"]):
        ref = head_reference(i["x"], i["ng"], i["nb"], i["hg"], i["hb"], i["dhn"], dfeat)
        dx, part = impl.head_bwd(i["dhn"], dfeat, i["x"], feat, i["ng"], i["hg"], stats)
        assert dx.shape == (B, Ntok, D)
        assert torch.equal(dx[:, 2:], torch.zeros(B, Ntok - 2, D)), "rows past the two prefix tokens must be exactly 0"
        assert torch.equal(part[:, 1], i["dhn"])
        sums = part.double().sum(0)
        figs = dict(dx=row_err(dx[:, :2], ref["dx"][:, :2]), dhg=rel_err(sums[0], ref["dhg"]), dhb=rel_err(sums[1], ref["dhb"]),
                    dng=rel_err(sums[2], ref["dng"]), dnb=rel_err(sums[3], ref["dnb"]))
        _rec(rec, f"head_bwd[{B},{Ntok},{D},dfeat{int(dfeat is not None)}]", **figs)
        assert max(figs.values()) < 2e-5, figs


# ---- head Linear ---------------------------------------------------------------------------------------------------------
def check_linear(impl, B, C, D, rec=None):
    x, W, b = rnd(B, D, seed=500), rnd(C, D, seed=501, scale=0.2), rnd(C, seed=502)
    dy = rnd(B, C, seed=503)
    start = (rnd(C, D, seed=504), rnd(C, seed=505))
    xd, Wd, dyd = x.double(), W.double(), dy.double()
    figs = dict(fwd=rel_err(impl.linear_fwd(x, W, b), xd @ Wd.t() + b.double()),
                fwd_nobias=rel_err(impl.linear_fwd(x, W, None), xd @ Wd.t()))
    for acc in (False, True):
        dx, dW, db = impl.linear_bwd(dy, x, W, accumulate=acc, start=start)
        off = (start[0].double(), start[1].double()) if acc else (0.0, 0.0)
        figs.update({f"dx{int(acc)}": rel_err(dx, dyd @ Wd), f"dW{int(acc)}": rel_err(dW, dyd.t() @ xd + off[0]),
                     f"db{int(acc)}": rel_err(db, dyd.sum(0) + off[1])})
    dx, dW, db = impl.linear_bwd(dy, x, W, want_dw=False)
    assert dW is None and db is None
    figs["dx_only"] = rel_err(dx, dyd @ Wd)
    _rec(rec, f"linear[{B},{C},{D}]", **figs)
    assert max(figs.values()) < 1e-5, figs


# ---- BCE -----------------------------------------------------------------------------------------------------------------
# dlogits: |error| of (sigmoid(z) - y) is bounded by the roundings of exp (<= 2 ulp), 1 + e (1/2), the division (<= 2.5), the
# subtraction (1/2) and the scaling (1/2), each of a value <= 1, i.e. of at most 2^-24: 6 * 2^-24; 8 * 2^-24 allowed.  The extreme
# case (saturated or near-zero logits, where those terms vanish) is held to 2 * 2^-24.
BCE_DZ_ULPS, BCE_DZ_ULPS_EXTREME = 8, 2


def _check_bce(impl, z, y, scale, name, dz_ulps, rec, baseline, loss_abs=None):
    baseline = baseline or TorchF32()
    n = z.numel()
    rl, rdz = bce_reference(z, y, scale)
    bl, _ = baseline.bce(z, y, scale)
    loss, dz = impl.bce(z, y, scale)
    assert bool(torch.isfinite(loss).all())
    base = abs(float(bl) - float(rl)) / abs(float(rl))
    got = abs(float(loss) - float(rl)) / abs(float(rl))
    tol = max(4 * base, 2e-6)
    dz_err = float((dz.double() - rdz).abs().max()) / (2.0 ** -24 * scale / n)
    _rec(rec, name, loss_rel=got, torch_f32_loss_rel=base, loss_allowed=tol, dz_ulps=dz_err)
    assert got <= tol, (got, base, tol)
    if loss_abs is not None:
        assert abs(float(loss) - float(rl)) < loss_abs
    assert dz_err <= dz_ulps, dz_err


def check_bce(impl, B, C, scale, rec=None, baseline=None):
    z, y = rnd(B, C, seed=600, scale=4.0), torch.rand(B, C, generator=torch.Generator().manual_seed(601))
    _check_bce(impl, z, y, scale, f"bce[{B * C},{scale:g}]", BCE_DZ_ULPS, rec, baseline)


def check_bce_small(impl, rec=None, baseline=None):
    """the shape and inputs the suite always had (B C = 111, hard targets, |z| <= 2) with its absolute 1e-6"""
    z, y = rnd(3, 37, seed=602, scale=2.0), (rnd(3, 37, seed=34) > 0.7).float()
    _check_bce(impl, z, y, 1.0, "bce_small[111]", BCE_DZ_ULPS, rec, baseline, loss_abs=1e-6)


def check_bce_extreme(impl, scale, rec=None, baseline=None):
    vals = torch.tensor(BCE_EXTREME)
    B, C = 7, 67
    z = vals[torch.randint(0, vals.numel(), (B, C), generator=torch.Generator().manual_seed(610))]
    y = torch.rand(B, C, generator=torch.Generator().manual_seed(611))
    _check_bce(impl, z, y, scale, f"bce_extreme[{scale:g}]", BCE_DZ_ULPS_EXTREME, rec, baseline)


# ---- cross entropy with mixup --------------------------------------------------------------------------------------------
def ce_inputs(B, C, spread, seed=700):
    g = torch.Generator().manual_seed(seed)
    z = rnd(B, C, seed=seed + 1, scale=80.0 if spread else 3.0)
    t = torch.randint(0, C, (B,), generator=g).to(torch.int32)
    t2 = torch.randint(0, C, (B,), generator=g).to(torch.int32)
    t2[::3] = t[::3]                                  # rows whose two targets coincide
    lam = torch.rand(B, generator=g) * 0.5 + 0.5
    lam[0] = 1.0
    if B > 1:
        lam[1] = 0.0
    return z, t, t2, lam


def check_ce(impl, B, C, spread, rec=None, baseline=None):
    baseline = baseline or TorchF32()
    z, t, t2, lam = ce_inputs(B, C, spread)
    for mix, scale in ((True, 1.0), (False, 0.5)):
        a2, al = (t2, lam) if mix else (None, None)
        rl, rdz = ce_reference(z, t, a2, al, scale)
        bl, bdz = baseline.ce(z, t, a2, al, scale)
        loss, dz = impl.ce(z, t, a2, al, scale)
        figs = dict(loss_abs=abs(float(loss) - float(rl)), dz_row=row_err(dz, rdz), dz_rel=rel_err(dz, rdz),
                    rowsum=float(dz.double().sum(1).abs().max()) / (scale / B),
                    torch_f32_loss_abs=abs(float(bl) - float(rl)), torch_f32_dz_row=row_err(bdz, rdz))
        if spread:
            # one f32 ulp of the log-sum-exp at |z| = 80 is already 7.6e-6
            loss_tol = 16 * 2.0 ** -24 * (float(z.abs().max()) + math.log(C))
            dz_tol = 1e-5
            if figs["torch_f32_loss_abs"] > loss_tol / 2:
                loss_tol = 2 * figs["torch_f32_loss_abs"]
            if figs["torch_f32_dz_row"] > dz_tol / 2:
                dz_tol = 2 * figs["torch_f32_dz_row"]
            figs.update(loss_allowed=loss_tol, dz_allowed=dz_tol)
            ok = figs["loss_abs"] <= loss_tol and figs["dz_row"] <= dz_tol
        else:
            ok = figs["loss_abs"] < 1e-5 and figs["dz_rel"] < 1e-5
        _rec(rec, f"ce[{B},{C},{'spread' if spread else 'scale3'},mix{int(mix)}]", **figs)
        assert ok, figs
        assert figs["rowsum"] <= 1e-6, figs


# ---- reductions: exact sums ----------------------------------------------------------------------------------------------
def slab_desc(splits, n, accumulate, seed=800):
    p = small_ints(splits, n, seed=seed + splits + n % 97)
    return dict(mode=REDUCE_SLABS, partial=p, n=n, splits=splits, pitch=n, accumulate=accumulate, start=small_ints(n, seed=seed + 1, lo=-50, hi=50))


def rows_desc(splits, n, pitch, accumulate, seed=820):
    p = padded(small_ints(splits, n, seed=seed + splits + n % 97), pitch)
    return dict(mode=REDUCE_ROWS, partial=p, n=n, splits=splits, pitch=pitch, accumulate=accumulate,
                start=small_ints(n, seed=seed + 1, lo=-50, hi=50))


def desc_want(d):
    s = int_sum(d["partial"][:, :d["n"]], 0)
    assert exact_sum_safe(torch.cat([d["partial"][:, :d["n"]], d["start"][None]]), 0)
    return d["start"] + s if d["accumulate"] else s


def check_reduce_slabs(impl, splits, n):
    for acc in (0, 1):
        d = slab_desc(splits, n, acc)
        want = desc_want(d)
        for single in (True, False):                     # pa_reduce_partials | pa_reduce_partials_batched, SLABS
            for off in ((0, 0), (1, 1), (0, 1), (1, 0)):     # out / partial 16-byte aligned, or one float off
                got, = impl.reduce([d], single=single, offsets=[off])
                assert torch.equal(got, want), (splits, n, acc, single, off)


def check_reduce_rows(impl, splits, n):
    for pitch in (n, 3 * n):
        for acc in (0, 1):
            d = rows_desc(splits, n, pitch, acc)
            got, = impl.reduce([d])
            assert torch.equal(got, desc_want(d)), (splits, n, pitch, acc)


def mixed_batch():
    """12 descriptors of both modes, different lengths, splits, pitches and accumulate flags"""
    ds = []
    for j, (splits, n) in enumerate(((1, 5), (7, 1027), (2, 4), (3, 4096), (7, 3), (2, 70000))):
        ds.append(slab_desc(splits, n, j & 1, seed=840 + j))
    for j, (splits, n, pitch) in enumerate(((17, 768, 2304), (1024, 16, 16), (65, 17, 51), (1, 1, 1), (63, 2304, 2304), (16, 40, 41))):
        ds.append(rows_desc(splits, n, pitch, (j >> 1) & 1, seed=860 + j))
    return ds[::2] + ds[1::2]


def check_reduce_batch(impl):
    ds = mixed_batch()
    assert len(ds) == 12
    together = impl.reduce(ds)
    for d, got in zip(ds, together):
        alone, = impl.reduce([d])
        assert torch.equal(got, alone) and torch.equal(got, desc_want(d)), (d["mode"], d["splits"], d["n"])


def check_colsum_f32(impl, R, C):
    for ld in (C, C + 3):
        a = padded(small_ints(R, C, seed=900 + R + C), ld)
        start = small_ints(C, seed=901, lo=-50, hi=50)
        for acc in (0, 1):
            want = int_sum(a[:, :C], 0) + (start if acc else 0)
            assert torch.equal(impl.colsum_f32(a, C, acc, start), want), (R, C, ld, acc)


def check_colsum(impl, R, C):
    for dt in (PA_F32, PA_BF16):
        for ld in (C, C + 8):
            a = padded(small_ints(R, C, seed=910 + R % 89 + C, dtype=TD[dt]), ld)
            assert exact_sum_safe(a[:, :C], 0)
            start = small_ints(C, seed=911, lo=-50, hi=50)
            for acc in (0, 1):
                want = int_sum(a[:, :C], 0) + (start if acc else 0)
                assert torch.equal(impl.colsum(a, C, dt, acc, start), want), (R, C, dt, ld, acc)


def check_rowsum(impl, R, C):
    for dt in (PA_F32, PA_BF16):
        for ld in (C, C + 3):
            a = padded(small_ints(R, C, seed=920 + R + C, dtype=TD[dt]), ld)
            start = small_ints(R, seed=921, lo=-50, hi=50)
            for acc in (0, 1):
                want = int_sum(a[:, :C], 1) + (start if acc else 0)
                assert torch.equal(impl.rowsum(a, C, dt, acc, start), want), (R, C, dt, ld, acc)


def exact_sum_inputs():
    """(name, tensor, dim) of a representative of every exact-sum input family above, for the order-independence check"""
    out = [("ln_addends", small_ints(520, 260, seed=202) + small_ints(520, 260, seed=203), 0),
           ("ln_dy", small_ints(8200, 260, seed=205, lo=-4, hi=4), 0),
           ("slabs", slab_desc(7, 1027, 0)["partial"], 0),
           ("rows", rows_desc(1024, 17, 17, 0)["partial"], 0),
           ("colsum", small_ints(33 * 256, 72, seed=910), 0),
           ("colsum_bf16", small_ints(8193, 8, seed=910, dtype=torch.bfloat16).float(), 0),
           ("rowsum", small_ints(5, 1000, seed=920), 1)]
    return out

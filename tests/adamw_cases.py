"""The guarded case and the exact model of the AdamW kernel family (tests/test_adamw_cases_cpu.py pins the model's arithmetic on the
CPU, tests/test_gpu_adamw_exact.py holds all seven pa_adamw* entries to it bit for bit; tests/test_gpu_finetune.py and
tests/test_gpu_grad_clip.py run their own comparisons on the same case).

The model restates adamw_one / clip_g of passt_amd/csrc/optim.hip rounding for rounding in numpy f32: every operation is one correctly
rounded f32 operation (numpy's), except the two moment updates, which the kernel issues as ONE fused multiply-add each -- here the
product of two f32 values taken in f64 (exact: 48 significant bits), one f64 addition and one rounding to f32.  That is a true FMA
unless the f64 sum lands within an f64 rounding error of an f32 tie: ``is_correctly_rounded`` decides it in exact rational arithmetic,
and the CPU test shows it for every element of the case.  The seven hyper floats are taken as given (the row pa_adamw_hyper writes):
the host's powf is outside the model.  f32 subnormals are outside it too (the device may flush them): ``trace`` hands every
intermediate out, the CPU test asserts they are all zero or normal."""
import functools
from fractions import Fraction

import numpy as np
import torch

from passt_amd import _lib, ops

F32 = np.float32
GUARD, SENT = 64, -1.5 * 2.0 ** 100
SCALES = {"a": [(1.0, 1.0), (0.5, 0.0), (0.75 ** 2, 1.0), (0.0, 0.0), (1.0, 0.0)],
          "b": [(0.0, 1.0), (0.75 ** 2, 0.0), (0.5, 1.0), (1.0, 0.0), (0.5, 1.0)],
          "ones": [(1.0, 1.0)] * 5}
# (rows, cols, copies, guard elements behind it): the 64-tile of the matrix has edges both ways; 4097 is one past a run; the 527
# vector is followed directly by the 768 one, whose offset (and the later guard's) is then off 16-byte alignment
PARAMS = [(100, 70, True, GUARD), (1, 4097, False, GUARD - 1), (1, 527, False, 0), (1, 768, False, GUARD), (1, 5, False, GUARD)]
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=3)
FACTORS = (None, 0.25, 0.3)


def group_case(dtype, device):
    """flat p / g / m / v (CPU) with sentinel guards around every parameter, guarded copies of ``dtype`` on ``device``"""
    gen = torch.Generator().manual_seed(17)
    offs, n = [], GUARD
    for rows, cols, _, guard in PARAMS:
        offs.append(n)
        n += rows * cols + guard
    live = torch.zeros(n, dtype=torch.bool)
    for off, (rows, cols, _, _) in zip(offs, PARAMS):
        live[off:off + rows * cols] = True
    p = torch.where(live, torch.randn(n, generator=gen) * 0.1, torch.tensor(SENT))
    g = torch.where(live, torch.randn(n, generator=gen) * 0.01, torch.tensor(float("nan")))
    m = torch.where(live, torch.randn(n, generator=gen) * 0.01, torch.tensor(SENT))
    v = torch.where(live, torch.rand(n, generator=gen) * 1e-4, torch.tensor(SENT))
    td = ops.TORCH_DTYPE[dtype]
    rows, cols = PARAMS[0][:2]
    copies = torch.full((2, GUARD + rows * cols + GUARD), SENT, dtype=td, device=device)
    dst, dst_t = copies[0, GUARD:GUARD + rows * cols].view(rows, cols), copies[1, GUARD:GUARD + rows * cols].view(cols, rows)
    return dict(p=p, g=g, m=m, v=v, live=live, offs=offs, copies=copies, dst=dst, dst_t=dst_t)


def hyper_row(h=HYPER):
    """the 7 floats pa_adamw_hyper writes for ``h`` (a host function: no GPU needed)"""
    host = torch.empty(7, dtype=torch.float32)
    ops.adamw_hyper(h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], host)
    return host


def fma32(a, b, c):
    """round_f32(a * b + c) for f32 operands: exact product in f64, one f64 addition, one rounding to f32"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def is_correctly_rounded(r, x):
    """is the f32 value ``r`` the round-to-nearest-even image of the rational ``x``?"""
    r = F32(r)
    lo, hi = np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))
    a, b = (Fraction(float(lo)) + Fraction(float(r))) / 2, (Fraction(float(r)) + Fraction(float(hi))) / 2
    even = (int(r.view(np.uint32)) & 1) == 0
    return a < x < b or (even and (x == a or x == b))


def model(p, g, m, v, row, lr_scale=None, wd_scale=None, factor=None, trace=None):
    """adamw_one on g (factor None) or clip_g(g, factor), f32 arrays in, (p, m, v) out; ``row``: the 7 hyper floats; lr_scale /
    wd_scale: the entry's pair per element (parameter groups), None: the launch has no groups (no multiplication)"""
    lr, b1, b2, eps, wd, bc1, bc2_sqrt = (F32(x) for x in row)
    one = F32(1.0)
    t = {}
    with np.errstate(all="raise", under="ignore"):
        if lr_scale is not None:
            lr, wd = lr * np.asarray(lr_scale, F32), wd * np.asarray(wd_scale, F32)
        if factor is not None:
            g = t["g"] = g * F32(factor)
        t["lr_wd"] = lr * wd
        t["keep"] = one - t["lr_wd"]
        pi = t["pi"] = p * t["keep"]
        gm = t["gm"] = (one - b1) * g
        t["gv0"] = (one - b2) * g
        gv = t["gv"] = t["gv0"] * g
        m1 = t["m"] = fma32(b1, m, gm)
        v1 = t["v"] = fma32(b2, v, gv)
        t["sqrt"] = np.sqrt(v1)
        t["sqrt_bc"] = t["sqrt"] / bc2_sqrt
        denom = t["denom"] = t["sqrt_bc"] + eps
        t["lr_bc"] = lr / bc1
        t["ratio"] = m1 / denom
        step = t["step"] = t["lr_bc"] * t["ratio"]
        p1 = t["p"] = pi - step
    assert all(np.asarray(x).dtype == F32 for x in t.values())
    if trace is not None:
        trace.update(t, moment_operands=(b1, m, gm, b2, v, gv))
    return p1, m1, v1


@functools.lru_cache(maxsize=None)
def expected(which, factor):
    """the case after one update, whole buffers: {p, m, v} as CPU tensors -- the model on the live elements, the sentinels elsewhere;
    ``which``: a key of SCALES, or None (a launch without groups)"""
    c = group_case(_lib.PA_F32, "cpu")
    live = c["live"].numpy()
    ls = ws = None
    if which is not None:
        ls, ws = np.zeros(live.size, F32), np.zeros(live.size, F32)
        for off, (rows, cols, _, _), (a, b) in zip(c["offs"], PARAMS, SCALES[which]):
            ls[off:off + rows * cols], ws[off:off + rows * cols] = a, b
        ls, ws = ls[live], ws[live]
    trace = {}
    new = model(*(c[k].numpy()[live] for k in "pgmv"), hyper_row().numpy(), ls, ws, factor, trace)
    out = {"trace": trace}
    for k, x in zip("pmv", new):
        out[k] = c[k].clone()
        out[k][c["live"]] = torch.from_numpy(x)
    return out


def expected_copies(p_full, c, dtype):
    """both guarded copies of the case's matrix after the update: the cast of p and of its transpose"""
    rows, cols = PARAMS[0][:2]
    w = p_full[c["offs"][0]:c["offs"][0] + rows * cols].view(rows, cols)
    cp = torch.full(c["copies"].shape, SENT, dtype=ops.TORCH_DTYPE[dtype])
    cp[0, GUARD:GUARD + rows * cols] = w.to(cp.dtype).reshape(-1)
    cp[1, GUARD:GUARD + rows * cols] = w.t().contiguous().to(cp.dtype).reshape(-1)
    return cp


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)

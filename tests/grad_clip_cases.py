"""References and buffer builders of the gradient-clipping / accumulation tests (tests/test_grad_clip_cpu.py pins them to torch on
the CPU, tests/test_gpu_grad_clip.py holds the kernels and the training step to them).

The norm reference is the f64 sum of squares; the factor is torch.nn.utils.clip_grad_norm_'s f32 arithmetic -- torch evaluates
``max_norm / (norm + 1e-6)`` as ``(norm + 1e-6).reciprocal() * max_norm`` (Tensor.__rdiv__), two roundings -- and the clipped AdamW
step is torch's single-tensor AdamW on ``g * factor``.

The error bound of the device norm follows from the partition of pa_grad_accum_sumsq ("Gradient norm"): every partial is
a sum of non-negative f32 terms whose longest chain of roundings is DEPTH = 24 (the squaring, 15 additions in a thread, 6 in the wave
butterfly, 2 over the four waves), so its relative error is at most gamma(24); the f64 combine of the partials adds at most
n_partials * 2^-53 (< 2^-38 for any buffer below 2^27 elements); the square root halves a relative error (to first order: the second
order term gamma^2 / 2 is below 2^-38) and the rounding of the result to f32 adds 2^-24."""
import math
from fractions import Fraction

import numpy as np
import torch

CHUNK = 4096                    # pa_grad_norm_partials(n) == ceil(n / CHUNK)
DEPTH = 24
U = 2.0 ** -24
GUARD = 64                      # elements around every span: 256 bytes, so the span's alignment is its element offset alone
SENT = -1.5 * 2.0 ** 100


def gamma(d):
    return d * U / (1.0 - d * U)


PARTIAL_BOUND = gamma(DEPTH)                                  # relative, per partial
NORM_BOUND = 0.5 * gamma(DEPTH) + 2.0 ** -24 + 2.0 ** -36     # relative, of out[0] against the f64 reference


def n_partials(n):
    return (n + CHUNK - 1) // CHUNK


def ref_partials(g):
    """f64 sums of squares of the chunks of the 1-D f32 array ``g``"""
    g = np.asarray(g, np.float64).reshape(-1)
    return np.array([np.sum(g[i:i + CHUNK] ** 2) for i in range(0, g.size, CHUNK)], np.float64)


def ref_norm(g):
    """the L2 norm of ``g`` in f64"""
    return float(np.sqrt(np.sum(np.asarray(g, np.float64) ** 2)))


def ref_coef(norm_f32, max_norm):
    """clip_grad_norm_'s factor for an f32 norm, in f32, rounding for rounding; NaN in, NaN out"""
    with np.errstate(all="ignore"):
        c = (np.float32(1.0) / (np.float32(norm_f32) + np.float32(1e-6))) * np.float32(max_norm)
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def ref_clipped_adamw(p, g, m, v, coef, lr, b1, b2, eps, wd, step):
    """one torch.optim.AdamW step (single-tensor form, f32 CPU tensors) on g * coef -> (p, m, v), the inputs untouched"""
    p, m, v = p.clone(), m.clone(), v.clone()
    g = g * torch.tensor(float(coef), dtype=torch.float32)
    p.mul_(1.0 - lr * wd)
    m.lerp_(g, 1.0 - b1)
    v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)
    return p, m, v


def is_correctly_rounded_sqrt(r, s):
    """is the f32 value ``r`` the correctly rounded square root of the non-negative integer ``s``?  Exact rational arithmetic."""
    r = np.float32(r)
    lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
    a, b = (Fraction(float(lo)) + Fraction(float(r))) / 2, (Fraction(float(r)) + Fraction(float(hi))) / 2
    return (a < 0 or a * a <= s) and s <= b * b


def integer_grads(n, seed):
    """n integer-valued f32 gradients in [-3, 3]: every square and every sum below 2^24 is exact in f32"""
    return torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(seed)).to(torch.float32)


def random_grads(n, seed, scale=1e-2):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def guarded(values, offset, fill, device):
    """``values`` (1-D f32 CPU tensor) at element offset GUARD + ``offset`` of a fresh allocation filled with ``fill`` (NaN for
    gradients: one read past the span poisons the sum; SENT for what is written: one store past it shows) -> (whole buffer, the span
    as a view).  Allocations are 256-byte aligned, so the span's 16-byte alignment is ``offset`` % 4."""
    n = values.numel()
    buf = torch.full((GUARD + offset + n + GUARD,), fill, dtype=torch.float32)
    buf[GUARD + offset:GUARD + offset + n] = values
    buf = buf.to(device)
    assert buf.data_ptr() % 256 == 0
    return buf, buf[GUARD + offset:GUARD + offset + n]


def guards_intact(buf, offset, n, fill):
    """nothing outside the span of ``guarded`` was written"""
    out = torch.cat([buf[:GUARD + offset], buf[GUARD + offset + n:]]).cpu()
    return bool(torch.isnan(out).all()) if fill != fill else bool((out == fill).all())

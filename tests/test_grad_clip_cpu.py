"""Gradient clipping without a GPU: the reference of tests/grad_clip_cases.py pinned to torch itself (clip_grad_norm_ followed by
torch.optim.AdamW on the CPU), the host-only partial count of the library, and the constructors' argument checks."""
import inspect

import numpy as np
import pytest
import torch

from passt_amd import _lib
from tests import grad_clip_cases as GC

SHAPES = [(7, 5), (4097,), (3,), (64, 33), (1,)]
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)


def _params(seed, scale):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen) * 0.1) for s in SHAPES]
    gs = [torch.randn(s, generator=gen) * scale for s in SHAPES]
    return ps, gs


@pytest.mark.parametrize("scale,max_norm", [(1.0, 1.0), (1e-2, 0.3), (1e-3, 5.0), (3.0, 0.77), (1.0, float("inf"))])
def test_reference_equals_torch_clip_then_adamw(scale, max_norm):
    ps, gs = _params(11, scale)
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    p0 = torch.cat([p.detach().reshape(-1) for p in ps]).clone()
    g0 = torch.cat([g.reshape(-1) for g in gs])
    opt = torch.optim.AdamW(ps, **HYPER)
    m, v = torch.zeros_like(p0), torch.zeros_like(p0)
    for step in (1, 2):
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert norm.dtype == torch.float32
        # the norm: torch's f32 value against the f64 reference (torch's own error: a norm of per-tensor f32 norms)
        assert abs(float(norm) - GC.ref_norm(g0.numpy())) <= 4 * GC.U * GC.ref_norm(g0.numpy())
        # the factor: bit for bit, given the same f32 norm -- seen through the gradients torch scaled in place
        coef = GC.ref_coef(norm.numpy(), max_norm)
        assert (coef < 1.0) == (float(norm) > max_norm)
        clipped = torch.cat([p.grad.reshape(-1) for p in ps])
        assert torch.equal(clipped, g0 * torch.tensor(float(coef), dtype=torch.float32))
        opt.step()
        p0, m, v = GC.ref_clipped_adamw(p0, g0, m, v, coef, HYPER["lr"], *HYPER["betas"], HYPER["eps"], HYPER["weight_decay"], step)
        got = torch.cat([p.detach().reshape(-1) for p in ps])
        assert torch.allclose(got, p0, rtol=2e-6, atol=1e-7)          # the bound of tests/test_optim_cpu.py
        st = [opt.state[p] for p in ps]
        assert torch.allclose(torch.cat([s["exp_avg"].reshape(-1) for s in st]), m, rtol=2e-6, atol=1e-7)
        assert torch.allclose(torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]), v, rtol=2e-6, atol=1e-12)


def test_factor_formula_bit_for_bit_over_many_norms():
    gen = torch.Generator().manual_seed(5)
    norms = torch.cat([torch.rand(4000, generator=gen) * 10.0, torch.rand(4000, generator=gen) * 1e-3, torch.tensor([0.0, 1.0, 1e30])])
    for max_norm in (1.0, 0.3, 1e-3, 7.5, float("inf")):
        want = torch.clamp(max_norm / (norms + 1e-6), max=1.0)
        got = torch.tensor([float(GC.ref_coef(n, max_norm)) for n in norms.numpy()], dtype=torch.float32)
        assert torch.equal(got, want), max_norm
    nan = GC.ref_coef(np.float32("nan"), 1.0)
    assert np.isnan(nan) and torch.isnan(torch.clamp(1.0 / (torch.tensor(float("nan")) + 1e-6), max=1.0))
    assert GC.ref_coef(np.float32(0.0), 1.0) == 1.0


def test_correct_rounding_check():
    assert GC.is_correctly_rounded_sqrt(np.float32(3.0), 9) and GC.is_correctly_rounded_sqrt(np.sqrt(np.float32(2.0)), 2)
    assert not GC.is_correctly_rounded_sqrt(np.nextafter(np.sqrt(np.float32(2.0)), np.float32(2.0)), 2)
    assert GC.is_correctly_rounded_sqrt(np.float32(0.0), 0)


def test_grad_norm_partials_is_a_function_of_n_alone():
    lib = _lib.load()                       # loads without a GPU
    ns = [1, 2, 3, 4, 5, 4095, 4096, 4097, 8192, 8193, 65537, 1000003, 86_000_000, 1 << 33]
    got = [int(lib.pa_grad_norm_partials(n)) for n in ns]
    assert got[0] == 1
    assert got == sorted(got)                                   # monotone
    assert got == [int(lib.pa_grad_norm_partials(n)) for n in ns]        # the same n, the same count
    assert got == [GC.n_partials(n) for n in ns]
    assert lib.pa_grad_norm_partials(0) == 0 and lib.pa_grad_norm_partials(-5) == 0


def test_public_arguments_and_their_checks():
    import passt_amd.optim
    from passt_amd.train import TrainStep
    sig = inspect.signature(TrainStep.__init__).parameters
    assert sig["clip_grad_norm"].default is None and sig["accumulate"].default == 1
    assert hasattr(TrainStep, "flush")
    sig = inspect.signature(passt_amd.optim.AdamW.__init__).parameters
    assert sig["max_grad_norm"].default is None and sig["max_grad_norm"].kind is inspect.Parameter.KEYWORD_ONLY
    w = torch.nn.Parameter(torch.zeros(3))
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            passt_amd.optim.AdamW([w], max_grad_norm=bad)
    opt = passt_amd.optim.AdamW([w], max_grad_norm=2.0)
    assert opt.max_grad_norm == 2.0 and opt.grad_norm is None

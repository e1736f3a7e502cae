"""pa_gemm_tn_batched_plan through ops.wgrad_tn_batched(..., plan=(n_long, long_steps)): long and short token slices of one
tile give the weight gradients and fused bias gradients of the uniform launch.  Smallest shapes at which each path can go wrong:
a ragged last stage (341 tokens = 7 steps of 48 + 5 tokens, always in the short slice), exact steps (432 = 9 x 48), the smallest
plan there is (96 tokens = 2 steps, one long + one short step), a single tile, edge tiles, fused column sums, an accumulating
problem, and the passt_s block's 108 tiles (324 workgroups: short items dispatched behind the first wave, both XCD orders).
Bounds as in test_gpu_kernels.py (test_wgrad_tn_batched_*): 3e-3 against the f64 product of the same bf16 operands, 1e-5 against
the uniform plan (same products, different split-K grouping) and for the bias gradient (f32 sums of exact bf16 values)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import ops  # noqa: E402
from passt_amd._lib import PA_BF16  # noqa: E402

DEV = "cuda"
SINGLE = [(256, 256, False, False)]                                       # (N, K, with db, accumulate)
EDGE = [(264, 776, True, False), (3072, 264, False, True), (256, 256, True, True)]
BLOCK = [(768, 768, False, False), (2304, 768, True, False), (768, 3072, True, True), (3072, 768, False, False)]


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def run(operands, shapes, plan):
    probs = []
    for (dY, X), (N, K, with_b, acc) in zip(operands, shapes):
        out = torch.full((N, K), 0.25 if acc else 7.0, device=DEV)
        db = torch.full((N,), 0.25 if acc else -3.0, device=DEV) if with_b else None
        probs.append((dY, X, out, acc, db))
    ops.wgrad_tn_batched(probs, PA_BF16, plan=plan)
    torch.cuda.synchronize()
    return [(p[2], p[4]) for p in probs]


SLICES = [(341, (2, 3)), (341, (1, 5)), (341, (2, 1)), (432, (2, 3)), (432, (1, 5)), (432, (2, 1)), (96, (1, 1))]
CASES = [pytest.param(shapes, tokens, plan, id=f"{name}-t{tokens}-a{plan[0]}-L{plan[1]}")
         for name, shapes in (("single_tile", SINGLE), ("edge_tiles", EDGE)) for tokens, plan in SLICES]
CASES += [pytest.param(BLOCK, 341, plan, id=f"block_108_tiles-t341-a{plan[0]}-L{plan[1]}") for plan in ((2, 3), (1, 5))]


@pytest.mark.parametrize("shapes,tokens,plan", CASES)
def test_long_short_plan_matches_f64_and_the_uniform_plan(shapes, tokens, plan):
    operands = [(rnd(tokens, N, seed=300 + i).to(torch.bfloat16).to(DEV), rnd(tokens, K, seed=310 + i).to(torch.bfloat16).to(DEV))
                for i, (N, K, _, _) in enumerate(shapes)]
    got = run(operands, shapes, plan)
    uniform = run(operands, shapes, (0, 0))
    for (dY, X), (N, K, with_b, acc), (w, b), (wu, bu) in zip(operands, shapes, got, uniform):
        base = 0.25 if acc else 0.0
        e_ref = rel_err(w, dY.double().cpu().T @ X.double().cpu() + base)
        e_uni = rel_err(w, wu)
        print(f"tokens {tokens} plan {plan} N {N} K {K}: vs f64 {e_ref:.2e}, vs uniform {e_uni:.2e}")
        assert e_ref < 3e-3
        assert e_uni < 1e-5
        if with_b:
            e_b = rel_err(b, dY.double().cpu().sum(0) + base)
            print(f"    bias gradient vs f64 {e_b:.2e}")
            assert e_b < 1e-5
    for _ in range(3):                              # four launches in all: the slabs are reduced in a fixed order
        again = run(operands, shapes, plan)
        for (w, b), (w2, b2) in zip(got, again):
            assert torch.equal(w, w2) and (b is None or torch.equal(b, b2))

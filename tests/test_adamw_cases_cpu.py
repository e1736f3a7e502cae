"""The exact model of the AdamW kernels checks itself (no GPU): on the inputs tests/test_gpu_adamw_exact.py uses, the f64 route of the
model's two fused multiply-adds gives the correctly rounded f32 result of the exact a * b + c (rational arithmetic, every live
element, every clip factor), and no intermediate of any case is an f32 subnormal, which the device would be free to flush."""
from fractions import Fraction

import numpy as np
import pytest

from tests import adamw_cases as AC

TINY = np.finfo(np.float32).tiny


@pytest.mark.parametrize("factor", AC.FACTORS)
def test_model_fma_is_the_exact_fma_and_nothing_is_subnormal(factor):
    runs = {which: AC.expected(which, factor) for which in (None, "a", "b")}
    b1, m, gm, b2, v, gv = runs[None]["trace"]["moment_operands"]
    assert m.size == gm.size == v.size == gv.size == 12397
    for a, x, c, got in ((b1, m, gm, runs[None]["trace"]["m"]), (b2, v, gv, runs[None]["trace"]["v"])):
        fa = Fraction(float(a))
        bad = sum(not AC.is_correctly_rounded(r, fa * Fraction(float(xe)) + Fraction(float(ce))) for xe, ce, r in zip(x, c, got))
        assert bad == 0
    for which, run in runs.items():
        # the moments do not see the groups' pairs: one pin of the FMA covers every scale set
        for k in "mv":
            assert np.array_equal(run["trace"][k].view(np.int32), runs[None]["trace"][k].view(np.int32)), (which, k)
        for name, x in run["trace"].items():
            if name != "moment_operands":
                x = np.abs(np.asarray(x))
                assert np.isfinite(x).all() and not ((x > 0) & (x < TINY)).any(), (which, factor, name)


def test_correct_rounding_check():
    one, up = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))
    tie = (Fraction(float(one)) + Fraction(float(up))) / 2
    assert AC.is_correctly_rounded(one, tie) and not AC.is_correctly_rounded(up, tie)          # ties go to the even mantissa
    assert AC.is_correctly_rounded(up, tie + Fraction(1, 2 ** 60)) and not AC.is_correctly_rounded(one, tie + Fraction(1, 2 ** 60))
    # where the f64 route double-rounds the check says so: a * b = 2^-24 - 2^-70, so a * b + c lies 2^-70 below the tie between c and
    # its upper neighbour; the f64 addition lands on the tie and the rounding to f32 then goes up, to the even mantissa
    a, b, c = np.float32(2.0 ** -24 * (1.0 + 2.0 ** -23)), np.float32(1.0 - 2.0 ** -23), np.float32(1.0 + 2.0 ** -23)
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    assert exact == Fraction(float(c)) + Fraction(1, 2 ** 24) - Fraction(1, 2 ** 70)
    assert AC.is_correctly_rounded(c, exact) and AC.fma32(a, b, c) != c and not AC.is_correctly_rounded(AC.fma32(a, b, c), exact)

"""The long/short token-slice plan of the batched weight-gradient launch (ops.pick_batched_plan, pa_gemm_tn_batched_plan), without
a GPU: what the planner returns covers every token step of every tile exactly once with no empty item, the slab count and the
workspace follow the plan, problems with different token counts keep the uniform plan, the model prefers long/short for the
passt_s block and uniform for the ESC-50 one, and the entry point rejects invalid plans before it touches a device."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from passt_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C2_BLOCK = [(27, 632), (9, 632), (36, 632), (36, 632)]      # passt_s block, batch 64: 30 336 tokens = 632 steps of 48
C5_BLOCK = [(27, 89), (9, 89), (36, 89), (36, 89)]          # ESC-50 fine-tune, batch 12: 4 236 tokens = 89 steps
BLOCK_NK = [(768, 768), (768, 2304), (3072, 768), (768, 3072)]    # (N, K) of a block's four gradients: 9, 27, 36, 36 tiles


def xcd_swizzle(bid, nwg):
    """pa_common.h: XCD `bid % 8` owns a contiguous run of the logical order"""
    q, r, xcd = nwg >> 3, nwg & 7, bid & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


def items_of(plan, probs):
    """(problem, tile, slab, first step, steps) of every workgroup of the launch, decoded as the kernels decode blockIdx.x"""
    n_long, L, splits = plan
    tfirst = [0]
    for t, _ in probs:
        tfirst.append(tfirst[-1] + t)
    tiles_all = tfirst[-1]

    def problem_of(t):
        p = 0
        while p + 1 < len(probs) and t >= tfirst[p + 1]:
            p += 1
        return p, t - tfirst[p]

    out = []
    if n_long:                                  # gemm_tn_stagger_plan_kernel
        steps = probs[0][1]
        nlong = tiles_all * n_long
        for b in range(tiles_all * (n_long + 1)):
            if b < nlong:
                g, t = divmod(xcd_swizzle(b, nlong), tiles_all)
            else:
                g, t = n_long, xcd_swizzle(b - nlong, tiles_all)
            p, t = problem_of(t)
            out.append((p, t, g, g * L, L if g < n_long else steps - g * L))
    else:                                       # gemm_tn_stagger_batched_kernel: ceil(steps / S) steps per slice, the last one shorter
        for p, ((tiles, steps), S) in enumerate(zip(probs, splits)):
            per = -(-steps // S)
            for t in range(tiles):
                for g in range(S):
                    out.append((p, t, g, g * per, min(steps, (g + 1) * per) - g * per))
    return out


GRID = [[(tiles, steps)] for tiles in (1, 7, 27, 108, 192, 256, 300) for steps in (1, 2, 3, 5, 9, 45, 89, 200, 632)]
GRID += [C2_BLOCK, C5_BLOCK, [(48, 527), (16, 527), (64, 527), (64, 527)], [(3, 8), (1, 8)], [(108, 9)]]


@pytest.mark.parametrize("probs", GRID, ids=lambda p: "+".join(f"{t}x{s}" for t, s in p))
def test_plan_covers_every_token_step_of_every_tile_once(probs):
    plan = ops._pick_batched_plan(probs)
    n_long, L, splits = plan
    assert len(splits) == len(probs)
    if n_long:
        assert n_long in (1, 2) and L >= 1 and 1 <= probs[0][1] - n_long * L <= L
        assert splits == [n_long + 1] * len(probs)                 # slabs per gradient
    else:
        assert splits == ops._pick_batched_splits(probs)
    items = items_of(plan, probs)
    assert len(items) == sum(t * s for (t, _), s in zip(probs, splits))
    seen = {}
    for p, t, g, begin, n in items:
        assert n >= 1, "empty item"
        assert 0 <= g < splits[p] and 0 <= t < probs[p][0]
        assert (p, t, g) not in seen, "two workgroups write one slab tile"
        seen[(p, t, g)] = (begin, n)
    for p, (tiles, steps) in enumerate(probs):
        for t in range(tiles):
            cover = sorted(seen[(p, t, g)] for g in range(splits[p]))
            assert cover[0][0] == 0 and cover[-1][0] + cover[-1][1] == steps
            assert all(a[0] + a[1] == b[0] for a, b in zip(cover, cover[1:]))


def test_long_and_short_items_are_spread_evenly_over_the_xcds():
    """the two orders are swizzled separately: of the passt_s block's 216 long items every XCD (blockIdx.x % 8) gets 27, all of
    ONE slice, and 13 or 14 of the 108 short ones"""
    items = items_of((2, 272, [3] * 4), C2_BLOCK)
    for x in range(8):
        mine = items[x::8]
        assert len({g for _, _, g, _, _ in mine[:27]}) == 1 and all(n == 272 for *_, n in mine[:27])
        assert len(mine) - 27 in (13, 14) and all(g == 2 and n == 88 for _, _, g, _, n in mine[27:])


def test_workspace_follows_the_slab_count():
    shapes = [(N, K, db) for (N, K), db in zip(BLOCK_NK, (False, True, True, False))]
    n_long, splits = 2, [3, 3, 3, 3]
    want = sum((n_long + 1) * N * K for N, K, _ in shapes) + (n_long + 1) * (768 + 3072)
    assert ops.wgrad_batched_ws_floats(splits, shapes) == want
    uni = ops._pick_batched_splits(C2_BLOCK)
    assert ops.wgrad_batched_ws_floats(uni, shapes) == sum(S * N * (K + db) for S, (N, K, db) in zip(uni, shapes))
    assert 7 * want == 3 * ops.wgrad_batched_ws_floats(uni, shapes)          # 3 slabs instead of 7


def test_different_token_counts_keep_the_uniform_plan():
    for probs in ([(27, 632), (9, 632), (36, 632), (36, 3)], [(9, 32), (27, 32), (36, 32), (36, 3)], [(108, 632), (1, 631)]):
        assert ops._pick_batched_plan(probs) == (0, 0, ops._pick_batched_splits(probs))


def test_model_prefers_long_short_for_the_passt_s_block_and_uniform_for_esc50():
    n_long, L, splits = ops._pick_batched_plan(C2_BLOCK)
    uniform = ops._uniform_cost(C2_BLOCK, ops._pick_batched_splits(C2_BLOCK))
    # two long slices and a short one whose three rounds on the 40 CUs left over end well before the long items do
    assert n_long == 2 and 3 * (632 - 2 * L + 4) * ops._SHORT_ITEM_COST <= L + 4 < 290
    assert ops._long_short_cost(108, 632, n_long, L) < (1 - ops._PLAN_MIN_GAIN) * uniform and abs(uniform - 379.8) < 1e-6
    assert ops._pick_batched_plan(C5_BLOCK) == (0, 0, [2, 2, 2, 2])
    # the memoised front gives the same answers unless the process forces the uniform plan
    if ops._FORCE_UNIFORM:
        assert ops.pick_batched_plan(C2_BLOCK) == (0, 0, ops.pick_batched_splits(C2_BLOCK))
    else:
        assert ops.pick_batched_plan(C2_BLOCK) == (n_long, L, [3, 3, 3, 3])
        assert ops.pick_batched_plan(C2_BLOCK) is ops.pick_batched_plan(list(C2_BLOCK))


@pytest.mark.parametrize("env", [{"PASST_AMD_WGRAD_PLAN": "uniform"}, {"PASST_AMD_WGRAD_SLICES": "4"}])
def test_environment_forces_the_uniform_plan(env):
    """read once at import: a fresh interpreter"""
    code = ("from passt_amd import ops; "
            "print(ops.pick_batched_plan([(27, 632), (9, 632), (36, 632), (36, 632)]))")
    full = {**os.environ, "PASST_AMD_WGRAD_PLAN": "long_short", "PASST_AMD_WGRAD_SLICES": "0", **env}
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=full, check=True, capture_output=True, text=True).stdout
    want = [4] * 4 if "PASST_AMD_WGRAD_SLICES" in env else ops._pick_batched_splits(C2_BLOCK)
    assert out.strip() == repr((0, 0, want))


def _args(tokens, shapes, split_k):
    args = (_lib.GemmArgs * len(shapes))()
    for a, (N, K) in zip(args, shapes):
        a.dtype, a.epilogue = _lib.PA_BF16, _lib.EPI_PARTIAL
        a.M, a.N, a.K = N, K, tokens
        a.lda, a.ldb, a.ldo32 = N, K, K
        a.A = a.B = a.out_f32 = 0x1000           # never dereferenced: every call below is rejected before a launch
        a.split_k = split_k
    return args


def test_entry_point_rejects_invalid_plans_without_a_device():
    lib = _lib.load()
    EINVAL, EUNSUPPORTED = -1, -2
    call = lambda args, n_long, L: lib.pa_gemm_tn_batched_plan(args, len(args), n_long, L, None)
    two = [(256, 256), (768, 264)]
    assert call(_args(341, two, 1), 0, 4) == EINVAL                   # no long slice
    assert call(_args(341, two, 3), 2, 0) == EINVAL                   # no steps in it
    assert call(_args(341, two, 3), 2, -1) == EINVAL
    assert call(_args(341, two, 3), 2, 4) == EINVAL                   # 2 x 4 = all 8 steps: the short slice would be empty
    assert call(_args(341, two, 2), 1, 8) == EINVAL
    assert call(_args(341, two, 2), 1, 9) == EINVAL
    assert call(_args(96, two, 3), 2, 1) == EINVAL                    # 2 steps
    assert call(_args(48, two, 2), 1, 1) == EINVAL                    # 1 step: nothing to split
    assert call(_args(341, two, 7), 2, 3) == EINVAL                   # split_k is the slab count, n_long + 1
    assert call(_args(341, two, 3), 1 << 30, 1 << 30) == EINVAL       # the product does not wrap
    mixed = _args(341, two, 3)
    mixed[1].K = 342
    assert call(mixed, 2, 3) == EUNSUPPORTED                          # token counts differ
    assert lib.pa_gemm_tn_batched_plan(None, 1, 2, 3, None) == EINVAL
    assert lib.pa_gemm_tn_batched_plan(_args(341, two, 3), 5, 2, 3, None) == EINVAL

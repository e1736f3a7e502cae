"""``net(x, rollout=..., rollout_from=...)`` without a GPU: the parser and the errors, the argument checks of pa_attention_rollout and
its workspace query (they return before any device access), the launch sequence (tests/test_sequence_cpu.py's recorder, against
tests/golden/rollout_traces.json) and the fixture tests/golden/rollout.npz.

Every test here but the "default traces" one fails on the parent commit: a missing function, a missing symbol, a missing file or a
TypeError on ``rollout=``."""
import contextlib
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from oracle import ref_import
from passt_amd import _lib, ops
from passt_amd import passt as P
from tests import test_sequence_cpu as S
from tests.golden import make_attn_golden as AG
from tests.golden import make_rollout_golden as RG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACES = os.path.join(ROOT, "tests", "golden", "rollout_traces.json")
X_SHAPE = (2, 1, 128, 250)


def _net(depth=2, train=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, depth=depth, num_heads=2, distilled=True,
                              s_patchout_t=6)
    return net.train(train)


# ----------------------------------------------------------------------------------------------
# the parser and the errors
# ----------------------------------------------------------------------------------------------
def test_parse_rollout():
    assert P.parse_rollout(None, 0, 12) is None
    assert P.parse_rollout("attn", 0, 12) == ("attn", 0) and P.parse_rollout("cam", -1, 12) == ("cam", 11)
    assert P.parse_rollout("attn", np.int64(3), 12) == ("attn", 3) and P.parse_rollout("cam", -12, 12) == ("cam", 0)


BAD = [dict(rollout="Attn"), dict(rollout="grad"), dict(rollout=True), dict(rollout=1), dict(rollout=("attn",)), dict(rollout=b"cam"),
       dict(rollout="attn", rollout_from=2), dict(rollout="cam", rollout_from=-3), dict(rollout="attn", rollout_from=1.0),
       dict(rollout="attn", rollout_from="1"), dict(rollout="cam", rollout_from=None), dict(rollout="attn", rollout_from=True),
       dict(rollout="attn", rollout_from=(0,)),
       dict(rollout_from=1), dict(rollout_from=-1)]                 # without rollout=


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
@pytest.mark.parametrize("lengths", [None, [250, 100]])
def test_bad_rollout_raises_before_any_draw(bad, lengths):
    net = _net(train=lengths is None)
    net.varlen_grad = True
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="rollout"):
        net(torch.zeros(X_SHAPE), **bad) if lengths is None else net(torch.zeros(X_SHAPE), lengths=lengths, **bad)
    assert torch.equal(torch.get_rng_state(), state)                # no Patchout draw was consumed, and no device was asked for


def _no_graph_calls():
    def no_grad(net, x):
        with torch.no_grad():
            net(x, rollout="cam")

    def frozen(net, x):
        net.requires_grad_(False)(x, rollout="cam", rollout_from=-1)

    def ragged_without_switch(net, x):
        net.eval()(x, lengths=[250, 100], rollout="cam")

    return [no_grad, frozen, ragged_without_switch]


@pytest.mark.parametrize("call", _no_graph_calls(), ids=lambda f: f.__name__)
def test_a_cam_call_that_records_no_graph_raises_before_any_draw(call):
    net = _net(train=True)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="come out of a backward"):
        call(net, torch.zeros(X_SHAPE))
    assert torch.equal(torch.get_rng_state(), state)


def test_ensemble_rejects_rollout():
    ens = passt_amd.passt.EnsembelerModel([_net(), _net()])
    for kw in (dict(rollout="attn"), dict(rollout="cam"), dict(rollout_from=1)):
        with pytest.raises(ValueError, match="rollout"):
            ens(torch.zeros(X_SHAPE), **kw)


# ----------------------------------------------------------------------------------------------
# the C entries' argument checks
# ----------------------------------------------------------------------------------------------
def test_pa_attention_rollout_checks_its_arguments_before_any_device_access():
    lib = _lib.load()
    assert lib.pa_abi_version() == 6                                 # an addition: the ABI version stays
    host = (C.c_float * 256)()                                       # non-NULL pointers the entry must never dereference
    p, p2 = C.addressof(host), C.addressof(host) + 2 * 33 * 4        # r_out right behind r_in's nr * total_tok floats
    EINVAL, EUNSUPPORTED = -1, -2

    def call(qkv=p, ldqkv=384, lse=p, d_o=p, ldo=128, compact=0, r_in=p, r_out=p2, ws=p, cu=None, total=33, B=1, H=2, N=33, nq=33, nr=2,
             mode=1, slices=0, dtype=_lib.PA_BF16, flags=1):
        return lib.pa_attention_rollout(qkv, ldqkv, lse, d_o, ldo, compact, r_in, r_out, ws, cu, total, B, H, N, nq, nr, mode, slices, 0.5,
                                        0.5, 1.0, 0.125, dtype, flags, None)

    for kw in (dict(qkv=None), dict(lse=None), dict(r_in=None), dict(r_out=None), dict(d_o=None),        # null pointers (CAM needs d_o)
               dict(r_out=p), dict(r_out=p + 4), dict(r_out=p2 - 4), dict(r_in=p2 + 8),      # r_out == r_in, or sharing a float with it
               dict(nr=0), dict(nr=-1), dict(nr=5),                  # nr out of range
               dict(nq=0), dict(nq=-2),                              # nq < 1
               dict(nq=34),                                          # fixed layout: more queries than tokens
               dict(dtype=2), dict(dtype=-1),                        # bad dtype
               dict(B=0), dict(H=0), dict(N=0), dict(B=-1), dict(flags=2), dict(flags=-1), dict(mode=2), dict(mode=-1), dict(slices=-1),
               dict(compact=2), dict(compact=-1), dict(ldqkv=383), dict(ldqkv=0), dict(ldo=127), dict(ldo=0),
               dict(total=32),                                       # fixed layout: total_tok is B * N
               dict(cu=p, total=32),                                 # packed layout: fewer tokens than the longest sequence
               dict(mode=0),                                         # ATTN takes no d_o ...
               dict(mode=0, d_o=None, compact=1)):                   # ... and no compact form of one
        assert call(**kw) == EINVAL, kw
    assert call(ldqkv=388) == EUNSUPPORTED                           # bf16 rows that are not 16-byte aligned
    assert call(ldqkv=386, dtype=_lib.PA_F32) == EUNSUPPORTED
    assert call(ldo=132) == EUNSUPPORTED and call(ldo=130, dtype=_lib.PA_F32) == EUNSUPPORTED

    ws = lib.pa_attention_rollout_ws_floats
    for args in ((0, 1, 33, 33, 2, 0), (33, 0, 33, 33, 2, 0), (33, 1, 0, 33, 2, 0), (33, 1, 33, 0, 2, 0), (33, 1, 33, 33, 0, 0),
                 (33, 1, 33, 33, 5, 0), (33, 1, 33, 33, 2, -1), (32, 1, 33, 33, 2, 0)):
        assert ws(*args) == EINVAL, args


def test_workspace_query_follows_the_slice_rule():
    """S = 1 (no workspace) whenever the queries fit one tile -- always so for the prefix-only tail's nq = 2 -- and for slices=1; an
    explicit count is capped at the number of query tiles and spread evenly: S = ceil(tiles / ceil(tiles / slices))."""
    ws = _lib.load().pa_attention_rollout_ws_floats
    assert ws(474, 1, 474, 2, 2, 0) == 0 and ws(64 * 1190, 64, 1190, 2, 2, 0) == 0 and ws(20, 1, 20, 20, 2, 0) == 0
    assert ws(474, 1, 474, 474, 2, 1) == 0
    assert ws(474, 1, 474, 474, 2, 4) == 4 * 2 * 474                 # 15 tiles in slices of 4: 4 slices
    assert ws(474, 1, 474, 474, 2, 7) == 5 * 2 * 474                 # slices of 3: 5 slices
    assert ws(474, 1, 474, 474, 1, 100) == 15 * 474                  # never more slices than tiles
    assert ws(67 * 2, 2, 67, 67, 2, 2) == 2 * 2 * 134


def test_header_declares_the_entries_and_the_binding_lists_them():
    text = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert "int pa_attention_rollout(" in text and "int64_t pa_attention_rollout_ws_floats(" in text and "#define PA_ABI_VERSION 6" in text
    assert "#define PA_ATTN_ROLLOUT_ATTN 0" in text and "#define PA_ATTN_ROLLOUT_CAM 1" in text and "#define PA_ATTN_ROLLOUT_MAX_ROWS 4" in text
    assert (ops.ATTN_ROLLOUT_ATTN, ops.ATTN_ROLLOUT_CAM, ops.ATTN_ROLLOUT_MAX_ROWS) == (0, 1, 4)
    res, args = _lib.SIGNATURES["pa_attention_rollout"]
    assert res is _lib.i32 and len(args) == 25
    assert _lib.SIGNATURES["pa_attention_rollout_ws_floats"][0] is _lib.i64
    mk = open(os.path.join(ROOT, "passt_amd", "csrc", "Makefile")).read()
    assert "attention_rollout.hip" in mk and "build/attention_rollout.o" in mk.split("EXTRA = -mllvm -amdgpu-mfma-vgpr-form")[0]


def test_the_three_map_kernels_take_their_tile_from_one_header():
    """passt_amd/csrc/pa_attn_tile.h holds the only copy of the tile arithmetic: the three translation units include it, none of them
    issues an MFMA or an exponential itself, and editing the header rebuilds every object."""
    csrc = os.path.join(ROOT, "passt_amd", "csrc")
    tile = open(os.path.join(csrc, "pa_attn_tile.h")).read()
    assert "mma32_first<T>(" in tile and "mma32<T>(" in tile and tile.count("__builtin_amdgcn_exp2f(") == 1
    for name in ("attention_probs.hip", "attention_probs_grad.hip", "attention_rollout.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "pa_attn_tile.h"' in text and '#include "pa_mma.h"' not in text, name
        assert "mma32" not in text and "__builtin_amdgcn_exp2f" not in text and "mfma" not in text.replace("amdgpu-mfma-vgpr-form", ""), name
    rules = [ln for ln in open(os.path.join(csrc, "Makefile")).read().splitlines() if ln.startswith("build/") and ".hip" in ln]
    assert len(rules) == 3 and rules[0].startswith("build/%.o: %.hip") and all("pa_attn_tile.h" in ln.split(":", 1)[1] for ln in rules)


def test_packed_start_rows_and_views():
    """The packed buffer: clip b's dense (2, N_b) block at float 2 * cu_tok[b], one-hot at cls / dist."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "upload_small", lambda host, device: torch.from_numpy(np.ascontiguousarray(host)))
        lay = P._PackedLayout(3, 16, 8, None, None, ntok=np.array([8, 3, 5]))
        r = lay.rollout_start("cpu")
    assert r.shape == (2, 16) and r.dtype == torch.float32 and float(r.sum()) == 6.0
    views = P._PackedLayout.rollout_views(r, torch.tensor([0, 8, 11, 16]))
    assert [tuple(v.shape) for v in views] == [(2, 8), (2, 3), (2, 5)]
    for v in views:
        assert v[0, 0] == 1 and v[1, 1] == 1 and float(v.sum()) == 2.0 and v.untyped_storage().data_ptr() == r.untyped_storage().data_ptr()


# ----------------------------------------------------------------------------------------------
# the launch sequence (tests/test_sequence_cpu.py's recorder, with stand-ins for the two new ops)
# ----------------------------------------------------------------------------------------------
def _roll(qkv, lse, r_in, B, H, N, scale, a, b, nq=None, d_o=None, mode=0, g_scale=1.0, do_compact=False, flags=0, slices=0, out=None):
    nq = N if nq is None else nq
    assert r_in.shape == (B, 2, N) and r_in.dtype == torch.float32 and lse.numel() == B * H * nq and flags == ops.ATTN_Q_PRESCALED
    assert (d_o is None) == (mode == 0)
    if d_o is not None:
        assert d_o.shape == ((B * nq if do_compact else B * N), H * 64) and d_o.dtype == qkv.dtype
    return r_in * g_scale                     # the stand-in hands the factor on: the reducer test reads it back


def _roll_varlen(qkv, lse, r_in, cu_tok, B, H, max_N, scale, a, b, nq=None, d_o=None, mode=0, g_scale=1.0, do_compact=False, flags=0,
                 slices=0, out=None):
    assert r_in.shape == (2, qkv.shape[0]) and lse.numel() == (H * qkv.shape[0] if nq is None else B * H * nq)
    assert (d_o is None) == (mode == 0)
    if d_o is not None:
        assert d_o.shape == ((B * nq if do_compact else qkv.shape[0]), H * 64)
    return r_in * g_scale


def _record(run):
    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(S._RESULTS, "attention_rollout", _roll)
        mp.setitem(S._RESULTS, "attention_rollout_varlen", _roll_varlen)
        return S._record_run(run)


def _is_step(e):
    return e[0].startswith("attention_rollout")


def _is_roll(e):
    """A rollout step, or the upload of the packed layout's one-hot start rows (2, M)."""
    return _is_step(e) or (e[0] == "upload_small" and str(e[1][0]).startswith("np.float32[2, "))


def _step(lengths, train, depth=2, backward=True, **kw):
    def go(rec):
        net = S._net(train=train) if depth == 2 else _net(depth, train)
        net.precision = "bf16"
        net.input_grad = net.varlen_grad = True
        x = torch.zeros(S.X_SHAPE, requires_grad=backward)
        with contextlib.nullcontext() if backward else torch.no_grad():
            out = net(x, **({} if lengths is None else dict(lengths=lengths)), **kw)
        at = 2 + ("hidden" in kw) + ("attn" in kw)                  # behind the maps, in front of tok_offsets
        roll = out[at] if "rollout" in kw else None
        if roll is not None:
            views = roll if isinstance(roll, list) else [roll]
            assert (lengths is not None) == isinstance(roll, list) and len(out) == at + 1 + (lengths is not None)
            assert all(v.dtype == torch.float32 and v.shape[-2] == 2 and v.grad_fn is None and not v.requires_grad and v.grad is None
                       for v in views)
            if kw["rollout"] == "cam":                # the forward hands out the one-hot start rows
                assert all(float(v.sum()) == v.numel() / v.shape[-1] and v[..., 0, 0].min() == 1 and v[..., 1, 1].min() == 1 for v in views)
        if backward:
            (out[0].sum() + out[1].sum()).backward()
            if roll is not None:
                if kw["rollout"] == "cam":
                    assert all(v.grad is not None and v.grad.shape == v.shape and v.grad.dtype == torch.float32 for v in views)
                    if lengths is not None:
                        assert len({v.grad.untyped_storage().data_ptr() for v in views}) == 1
                    assert out[0].grad_fn.c is None and out[0].grad_fn.rollout is None      # nothing keeps the activations
                else:
                    assert all(v.grad is None for v in views)
    return go


TRACE_CASES = {
    "fixed_attn_eval_nograd": dict(lengths=None, train=False, backward=False, rollout="attn"),
    "fixed_attn_train": dict(lengths=None, train=True, rollout="attn"),
    "fixed_attn_from1_full_tail": dict(lengths=None, train=True, rollout="attn", rollout_from=1, hidden=(-1,)),
    "packed_attn_eval_nograd": dict(lengths=S.LENGTHS, train=False, backward=False, rollout="attn"),
    "fixed_cam_train": dict(lengths=None, train=True, rollout="cam"),
    "fixed_cam_from_last": dict(lengths=None, train=True, rollout="cam", rollout_from=-1),
    "packed_cam_varlen_grad": dict(lengths=S.LENGTHS, train=False, rollout="cam"),
    "depth3_attn_from1": dict(lengths=None, train=False, depth=3, backward=False, rollout="attn", rollout_from=1),
}


def _plain(case):
    return {k: v for k, v in case.items() if k not in ("rollout", "rollout_from")}


@pytest.mark.parametrize("name", list(TRACE_CASES))
def test_rollout_adds_its_launches_and_nothing_else(name):
    """With ``rollout`` the trace is that of the same call without it plus the rollout steps: "attn" exactly depth - k steps behind the
    last block (after the head), none in the backward and no attention_probs launch; "cam" none in the forward and one right behind
    the attention backward of every block >= k, no attention_probs_grad launch.  The trace is the committed one."""
    case = TRACE_CASES[name]
    depth, k = case.get("depth", 2), case.get("rollout_from", 0) % case.get("depth", 2)
    plain, got = _record(_step(**_plain(case))), _record(_step(**case))
    with open(TRACES) as f:
        assert got == json.load(f)["traces"][name]
    assert [e for e in got if not _is_roll(e)] == plain
    assert not any(e[0].startswith("attention_probs") for e in got)
    steps = [i for i, e in enumerate(got) if _is_step(e)]
    assert len(steps) == depth - k
    packed = case["lengths"] is not None
    full_tail = "hidden" in case
    for e in (got[i] for i in steps):
        assert e[0] == ("attention_rollout_varlen" if packed else "attention_rollout") and e[3] == "main"
    if case["rollout"] == "attn":
        head = [i for i, e in enumerate(got) if e[0] == "linear_f32_fwd"][0]
        first = head + 1 + packed                                            # (packed: the start rows are uploaded first)
        assert steps == list(range(first, first + depth - k))                # behind the last block, back to back
        for j, i in enumerate(steps):                                        # the last block first; a = b = 0.5; its own nq
            assert got[i][1][-2:] == [0.5, 0.5] and got[i][2]["nq"] == (2 if j == 0 and not full_tail else None)
            assert "mode" not in got[i][2] and "d_o" not in got[i][2]
    else:
        bwd = [i for i, e in enumerate(got) if e[0].startswith("attention_bwd")]
        assert len(bwd) == depth and steps == [i + 1 for i in bwd[:depth - k]]      # the backward walks the blocks downwards
        for j, i in enumerate(steps):
            e = got[i]
            assert e[1][-2:] == [1.0, 1.0] and e[2]["nq"] == (2 if j == 0 else None)
            assert e[2]["mode"] == ops.ATTN_ROLLOUT_CAM and e[2]["g_scale"] == 1.0 and e[2]["do_compact"] == (j == 0)


def test_without_rollout_the_trace_is_the_recorded_one():
    for name in ("fixed_train_bf16", "packed_hidden_attn_grad", "fixed_attn_prefix_mean", "fixed_eval_forward"):
        S.test_launch_sequence_is_the_recorded_one(name)


def test_rollout_rides_along_with_attn_and_attn_grad():
    """All three keywords in one call: the maps, their gradients and both kinds of rollout launch are all there."""
    def go(rec):
        net = S._net(train=True)
        out = net(torch.zeros(S.X_SHAPE), hidden=(0,), attn=(0, -1), attn_rows="prefix", attn_heads="mean", attn_grad="cam", rollout="cam")
        assert len(out) == 5 and out[4].shape[:2] == (2, 2) and out[4].shape[-1] == out[3][0].shape[-1]
        (out[0].sum() + out[2][0].sum()).backward()
        assert out[4].grad is not None and all(m.grad is not None for m in out[3])

    with pytest.MonkeyPatch.context() as mp:
        from tests import test_attn_grad_cpu as TG
        mp.setitem(S._RESULTS, "attention_probs_grad", TG._pgrad)
        got = _record(go)
    assert sum(_is_step(e) for e in got) == 2 and sum(e[0] == "attention_probs_grad" for e in got) == 2
    assert sum(e[0] == "attention_probs" for e in got) == 2


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
@pytest.mark.parametrize("world", [2, 3])
def test_under_an_attached_reducer_the_kernel_gets_the_world_size(lengths, world):
    """An attached reducer makes the node divide dlogits by the world size; prod(I + C_l) is not linear in that factor, so every step is
    handed g_scale = world and nothing is multiplied afterwards.  The stand-in multiplies the rows by g_scale: two steps leave
    world^2 at the one-hot positions."""
    class Reducer:
        def __init__(self, total):
            self.world, self.total, self.flat, self.waited, self.blocks = world, total, None, 0, []

        def on_block_done(self, i):
            self.blocks.append(i)

        def wait(self):
            self.waited += 1

    def go(rec):
        net = S._net(train=lengths is None)
        net.varlen_grad = True
        red = net._ddp = Reducer(net._graph_params()[1])
        out = net(torch.zeros(S.X_SHAPE), **({} if lengths is None else dict(lengths=lengths)), rollout="cam")
        (out[0].sum() + out[1].sum()).backward()
        assert red.waited == 1 and red.flat is not None
        for v in (out[2] if isinstance(out[2], list) else [out[2]]):
            assert float(v.grad.max()) == float(world) ** 2 and float(v.grad.sum()) == float(v.sum()) * world ** 2

    got = _record(go)
    assert [e[2]["g_scale"] for e in got if _is_step(e)] == [float(world)] * 2


# ----------------------------------------------------------------------------------------------
# the fixture
# ----------------------------------------------------------------------------------------------
def _expected():
    out = {}
    for name, case in AG.CASES.items():
        for k in RG.first_blocks(name):
            for kind in ("attn", "cam"):
                out[f"{name}.{kind}.from{k}"] = (case["B"], 290 if not case["training"] else None, case["cfg"]["depth"] - k)
    for i, n in enumerate(AG.RAGGED["lengths"]):
        for kind in ("attn", "cam"):
            out[f"ragged.{i}.{kind}.from0"] = (1, 2 + 12 * ((n - 16) // 10 + 1), AG.RAGGED["cfg"]["depth"])
    return out


def test_fixture_keys_shapes_and_content(golden_dir):
    path = os.path.join(golden_dir, "rollout.npz")
    assert os.path.getsize(path) < 256 * 1024
    gold = dict(np.load(path))
    want = _expected()
    assert RG.first_blocks("three_blocks") == (0, 1) and "three_blocks.cam.from1" in want
    assert set(gold) == set(want) | {k + ".shape" for k in want}
    for k, (B, ntok, nfac) in want.items():
        r = gold[k]
        assert r.dtype == np.float64 and r.ndim == 3 and r.shape[:2] == (B, 2) and tuple(gold[k + ".shape"]) == r.shape
        assert ntok is None or r.shape[2] == ntok
        assert r.min() >= 0
        if ".attn." in k:
            assert np.abs(r.sum(-1) - 1).max() < 1e-12               # the renormalised recipe: every row sums to 1
            assert (r[:, 0, 0] > 0.5 ** nfac).all() and (r[:, 1, 1] > 0.5 ** nfac).all()      # 0.5 per factor stays on the token itself
        else:
            assert (r[:, 0, 0] >= 1).all() and (r[:, 1, 1] >= 1).all()           # I + ...: the start rows stay underneath
    # fewer factors leave more on the diagonal
    assert (gold["three_blocks.attn.from1"][:, 0, 0] > gold["three_blocks.attn.from0"][:, 0, 0]).all()


def test_generator_holds_no_reference_text():
    src = open(os.path.join(ROOT, "tests", "golden", "make_rollout_golden.py")).read()
    assert "ref_import" in src and "GG.run_reference" in src and "softmax(dim" not in src and "class " not in src
    assert RG.CASES is AG.CASES and RG.RAGGED is AG.RAGGED


def test_recipes_are_row_chains():
    """The fixture's recipes on random matrices: their cls / dist rows are the chain of row-vector x matrix products, last block first."""
    rng = np.random.default_rng(5)
    maps = [rng.random((2, 9, 9)) for _ in range(3)]
    maps = [m / m.sum(-1, keepdims=True) for m in maps]
    for first in (0, 1):
        r = np.zeros((2, 2, 9))
        r[:, 0, 0] = r[:, 1, 1] = 1
        c = r.copy()
        for m in reversed(maps[first:]):
            r = 0.5 * r + 0.5 * r @ m
            c = c + c @ m
        assert np.abs(RG.recipe_attn(maps, first) - r).max() < 1e-14 and np.abs(RG.recipe_cam(maps, first) - c).max() < 1e-13


@pytest.mark.skipif(not ref_import.reference_available(), reason="needs the reference checkout")
def test_fixture_regenerates_bit_identically(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setattr(RG, "HERE", str(tmp_path))
    state = torch.get_rng_state()
    RG.main()
    torch.set_rng_state(state)
    a, b = np.load(os.path.join(golden_dir, "rollout.npz")), np.load(os.path.join(str(tmp_path), "rollout.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and float(np.abs(a[k].astype(np.float64) - b[k]).max()) == 0.0, k


if __name__ == "__main__":
    import subprocess
    import sys
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python -m tests.test_rollout_cpu --write")
    commit = subprocess.run(["git", "log", "-1", "--format=%h %s"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    traces = {name: _record(_step(**case)) for name, case in TRACE_CASES.items()}
    with open(TRACES, "w") as f:
        json.dump(dict(note=f"Launch traces of net(x, rollout=...) recorded by `python -m tests.test_rollout_cpu --write` on top of commit "
                            f"{commit}, with tests/test_sequence_cpu.py's recorder.", traces=traces), f, separators=(",", ":"))
        f.write("\n")
    print("wrote", list(traces))

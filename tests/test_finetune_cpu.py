"""Partial fine-tuning without a GPU: the trainable plan (passt.trainable_plan), what a partly frozen network launches -- in the
recorder of tests/test_sequence_cpu.py -- the parameter groups of TrainStep (train.group_scales) and the ABI of the two new
optimizer entries.

The freeze cases on the depth-2 model (stages -1 patch, 0, 1 blocks, 2 final norm + head):
  head_only     norm.* + head.*                      stop = 2
  block1_head   blocks.1.* + norm.* + head.*         stop = 1
  block0_head   blocks.0.* + norm.* + head.*         stop = 0, block 1 runs its activation gradients only
  norm_only     every parameter with dim() <= 1      stop = -1, no weight-gradient GEMM anywhere"""
import re
import warnings

import pytest
import torch

import passt_amd
from passt_amd import _lib
from passt_amd import passt as P
from passt_amd import train as T
from tests import test_sequence_cpu as S

FREEZE = {
    "head_only": lambda n, p: n.startswith(("norm.", "head.")),
    "block1_head": lambda n, p: n.startswith(("blocks.1.", "norm.", "head.")),
    "block0_head": lambda n, p: n.startswith(("blocks.0.", "norm.", "head.")),
    "norm_only": lambda n, p: p.dim() <= 1,
}
STOP = {"head_only": 2, "block1_head": 1, "block0_head": 0, "norm_only": -1, "all": -1}
WGRAD = ("wgrad_tn", "wgrad_tn_batched")
# not launches of the sequence: host bookkeeping, the workspace query, and the first-use staging of a transposed weight copy (every
# case builds its own model, so where those fall depends on which input-gradient GEMM comes first)
HOST = ("side.fork", "side.join", "block_done", "returned", "fwd_end", "transpose", "gemm_colsum_ws")


def _frozen_net(case, precision="bf16", train=True):
    net = S._net(train)
    net.precision = precision
    if case != "all":
        for n, p in net.named_parameters():
            p.requires_grad_(bool(FREEZE[case](n, p)))
    return net


def _run(case, precision="bf16", plan_kw=None, legacy=False):
    """(forward trace, backward trace, block_done indices, which ctx["saved"] entries are None) of one forward + backward through the
    public kernel-sequence functions under the case's plan (``legacy``: save=True and every gradient buffer, as before plans)."""
    state = {}

    def run(rec):
        net = _frozen_net(case, precision)
        plan = P.trainable_plan(net, **(plan_kw or {}))
        logits, feat, ctx = P.passt_forward(net, torch.zeros(S.X_SHAPE), save=True if legacy else plan)
        state["saved_none"] = [s is None for s in ctx["saved"]]
        state["plan"] = plan
        rec.log("fwd_end")
        grads = {n: torch.zeros_like(p) for n, p in net.named_parameters() if (n in plan.wanted if not legacy else not n.startswith("head_dist."))}
        P.passt_backward(net, ctx, torch.ones_like(logits), torch.ones_like(feat), grads,
                         on_block_done=lambda i: rec.log("block_done", (i,)), want_dx=bool((plan_kw or {}).get("want_dx")))
    trace = S._record_run(run)
    cut = [e[0] for e in trace].index("fwd_end")
    fwd, bwd = trace[:cut], trace[cut + 1:]
    return fwd, bwd, [e[1][0] for e in bwd if e[0] == "block_done"], state


def _names(trace):
    return [e[0] for e in trace if e[0] not in HOST]


@pytest.fixture(scope="module")
def full():
    return _run("all")


def test_all_trainable_plan_launches_what_the_call_without_a_plan_launches(full):
    legacy = _run("all", legacy=True)
    assert full[0] == legacy[0] and full[1] == legacy[1] and full[2] == [2, 1, 0, -1]
    assert full[3]["saved_none"] == [False, False]


@pytest.mark.parametrize("case", list(FREEZE))
def test_forward_of_a_partly_frozen_net_is_the_all_trainable_forward(case, full):
    fwd, _, _, state = _run(case)
    stop = STOP[case]
    assert state["plan"].stop == stop
    assert state["saved_none"] == [i < stop for i in range(2)]
    assert [e[0] for e in fwd] == [e[0] for e in full[0]]
    block_lns = 0
    for got, want in zip(fwd, full[0]):
        if got[0] == "layernorm_fwd" and got[1][4] == P.PA_BF16:      # the blocks' LayerNorms (two per block, in block order)
            assert got[1][:5] == want[1][:5] and got[2:] == want[2:]
            assert got[1][5] is (block_lns // 2 >= stop), (case, block_lns)
            block_lns += 1
        else:
            assert got == want
    assert block_lns == 4


def test_head_only_backward_is_the_head_stage(full):
    _, bwd, done, _ = _run("head_only")
    names = _names(bwd)
    assert names == ["linear_f32_bwd", "head_pre_bwd"] + ["colsum_f32"] * 4
    assert done == [2]
    for banned in ("gemm_nt", "dgelu_gemm", "attention_bwd", "layernorm_bwd", "wgrad_tn", "patch_bwd"):
        assert not any(n.startswith(banned) for n in names), banned
    assert len(_names(full[1])) > 20


def test_block1_and_head_backward_ends_with_block_1s_weight_gradients():
    _, bwd, done, _ = _run("block1_head")
    names = _names(bwd)
    assert names[-1] == "wgrad_tn_batched" and names.count("wgrad_tn_batched") == 1
    assert names.count("attention_bwd") == 1 and names.count("dgelu_gemm") == 1
    assert not any(n.startswith("patch_") for n in names)
    assert done == [2, 1]
    problems = [e for e in bwd if e[0] == "wgrad_tn_batched"][0][1][0]
    assert len(problems) == 4


def _block_segments(names):
    """the backward's op names cut at every dgelu_gemm's block start (the launch in front of it belongs to the block: the fc2 weight
    gradient is only queued): [head stage, last block, ..., block 0 (+ patch stage)]"""
    cuts = [i for i, n in enumerate(names) if n == "dgelu_gemm"]
    return [names[a:b] for a, b in zip([0] + cuts, cuts + [len(names)])]


def test_block0_and_head_with_block_1_frozen(full):
    _, bwd, done, _ = _run("block0_head")
    names = _names(bwd)
    assert done == [2, 0]
    head, b1, b0 = _block_segments(names)
    # block 1: what the fully frozen backward (the loss-network mode) launches for it, and nothing else

    def run(rec):
        net = S._net(True).requires_grad_(False)
        net.precision = "bf16"
        logits, feat, ctx = P.passt_forward(net, torch.zeros(S.X_SHAPE), save=True)
        rec.log("fwd_end")
        P.passt_backward(net, ctx, torch.ones_like(logits), torch.ones_like(feat), None, want_dx=True)
    tr = S._record_run(run)
    frozen = _names(tr[[e[0] for e in tr].index("fwd_end") + 1:])
    f_head, f_b1, _ = _block_segments(frozen)
    # the head stage of this case reduces its parameters (colsum_f32); behind them both convert the head's gradient for the last block
    assert b1[:-1] == f_b1 and not any(n in WGRAD or n == "colsum" for n in b1[:-1])
    # block 0 is complete: the all-trainable block 0 -- plus its fc2.bias, which the frozen block above no longer reduces for it --
    # and the backward ends with its weight gradients (no patch stage)
    _, _, full_b0 = _block_segments(_names(full[1]))
    assert b1[-1] == "colsum" and b0 == full_b0[:full_b0.index("wgrad_tn_batched") + 1]
    assert names[-1] == "wgrad_tn_batched" and names.count("wgrad_tn_batched") == 1
    assert len([e for e in bwd if e[0] == "wgrad_tn_batched"][0][1][0]) == 4
    # block 1's LayerNorm backward launches hand out no parameter gradient, block 0's do
    ln = [e for e in bwd if e[0] == "layernorm_bwd"]
    assert len(ln) == 4 and all(e[1][6] is None and e[1][7] is None for e in ln[:2]) and all(e[1][6] is not None for e in ln[2:])


def test_norm_only_has_no_weight_gradient_problem(full):
    _, bwd, done, _ = _run("norm_only")
    names = _names(bwd)
    assert not any(n in WGRAD for n in names)
    assert done == [2, 1, 0, -1]
    # every activation-gradient launch of the all-trainable backward is there, in order
    assert [n for n in names if n not in ("colsum", "colsum_f32")] == [n for n in _names(full[1]) if n not in WGRAD + ("colsum", "colsum_f32")]
    # no reduction waits for a finishing launch that never comes
    for e in bwd:
        if e[0] in ("layernorm_bwd", "dgelu_gemm"):
            assert e[2].get("defer") is None


def test_norm_only_fp32_keeps_the_activation_chain():
    _, bwd, done, _ = _run("norm_only", precision="fp32")
    full32 = _run("all", precision="fp32")
    names = _names(bwd)
    assert not any(n in WGRAD for n in names) and done == [2, 1, 0, -1]
    assert [n for n in names if n != "colsum"] == [n for n in _names(full32[1]) if n not in WGRAD + ("colsum",)]


def test_stop_falls_when_the_backward_has_work_further_down(full):
    # the input's gradient: the whole activation chain and the patch stage, weight gradients only where something is trainable
    _, bwd, done, state = _run("head_only", plan_kw=dict(want_dx=True))
    names = _names(bwd)
    assert state["plan"].stop == -1 and state["saved_none"] == [False, False]
    assert names.count("attention_bwd") == 2 and "patch_input_bwd" in names and not any(n in WGRAD for n in names)
    assert done == [2]
    # a map gradient / rollout step at block 0 (attn_grad=, rollout="cam"): the chain down to block 0's attention backward
    _, bwd, done, state = _run("block1_head", plan_kw=dict(low_block=0))
    names = _names(bwd)
    assert state["plan"].stop == 0 and names.count("attention_bwd") == 2 and names[-1] == "attention_bwd"
    assert names.count("wgrad_tn_batched") == 1 and done == [2, 1] and not any(n.startswith("patch_") for n in names)


def test_autograd_node_of_a_partly_frozen_net():
    got = {}

    def run(rec):
        net = _frozen_net("block1_head")
        logits, feat = net(torch.zeros(S.X_SHAPE))
        rec.log("fwd_end")
        (logits.sum() + feat.sum()).backward()
        got["grads"] = {n for n, p in net.named_parameters() if p.grad is not None}
        got["want"] = {n for n, p in net.named_parameters() if p.requires_grad and not n.startswith("head_dist.")}
    tr = S._record_run(run)
    names = _names(tr[[e[0] for e in tr].index("fwd_end") + 1:])
    assert got["grads"] == got["want"] and len(got["want"]) == 12 + 6
    assert names.count("attention_bwd") == 1 and names[-1] == "wgrad_tn_batched"

    def run_dx(rec):
        net = _frozen_net("head_only")
        net.input_grad = True
        x = torch.zeros(S.X_SHAPE, requires_grad=True)
        logits, feat = net(x)
        rec.log("fwd_end")
        (logits.sum() + feat.sum()).backward()
        got["dx"] = x.grad
    tr = S._record_run(run_dx)
    names = _names(tr[[e[0] for e in tr].index("fwd_end") + 1:])
    assert got["dx"] is not None and names.count("attention_bwd") == 2 and "patch_input_bwd" in names


# ---- the plan itself ---------------------------------------------------------------------------------------------------------------
def _deep(depth):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return passt_amd.PaSST(img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, depth=depth, num_heads=2, distilled=True)


PLAN_TABLE = [
    # trainable name prefixes, want_dx, low_block -> stop as an offset: ("d", k) = depth - k, or an absolute stage
    (("norm.", "head."), False, None, ("d", 0)),
    (("head.1.bias",), False, None, ("d", 0)),
    (("blocks.1.", "head."), False, None, 1),
    (("blocks.1.norm2.bias",), False, None, 1),
    (("blocks.0.mlp.fc1.weight", "head."), False, None, 0),
    (("cls_token",), False, None, -1),
    (("patch_embed.proj.bias", "head."), False, None, -1),
    (("norm.", "head."), True, None, -1),
    (("norm.", "head."), False, 0, 0),
    (("blocks.1.",), False, 0, 0),
    (("blocks.0.",), False, 1, 0),
    ((), False, None, ("d", 0)),
    ((), True, None, -1),
    (("head_dist.",), False, None, ("d", 0)),
]


@pytest.mark.parametrize("depth", [2, 12])
def test_plan_table(depth):
    net = _deep(depth)
    for prefixes, want_dx, low, stop in PLAN_TABLE:
        for n, p in net.named_parameters():
            p.requires_grad_(n.startswith(prefixes) if prefixes else False)
        plan = P.trainable_plan(net, want_dx=want_dx, low_block=low)
        want = {n for n, p in net.named_parameters() if p.requires_grad and not n.startswith("head_dist.")}
        assert plan.stop == (depth - stop[1] if isinstance(stop, tuple) else stop), (prefixes, want_dx, low)
        assert plan.wanted == want
        assert plan.live == {P.param_stage(n, depth) for n in want}
        named = net._graph_params()[0]
        assert [named[i][0] for i in plan.idx] == [n for n, _ in named if n in want]
        assert plan.total == sum(p.numel() for n, p in named if n in want)
        # the scratch outputs: the unwanted small parameters of the stages that run their reductions anyway
        assert {n for n, _ in plan.dump} == {n for n, _ in named if n not in want and P.param_stage(n, depth) in plan.live
                                             and not n.endswith(P._WGRAD_MATRICES)}
    assert P.param_stage("time_new_pos_embed", depth) == -1 and P.param_stage("patch_embed.proj.weight", depth) == -1
    assert P.param_stage(f"blocks.{depth - 1}.norm1.weight", depth) == depth - 1 and P.param_stage("norm.bias", depth) == depth
    assert P.param_stage("head.0.weight", depth) == depth


@pytest.mark.parametrize("depth", [2, 12])
def test_group_scales(depth):
    net = _deep(depth)
    nd = [(n, p.dim()) for n, p in net.named_parameters() if not n.startswith("head_dist.")]
    assert T.group_scales(nd, depth) is None and T.group_scales(nd, depth, None, ()) is None
    pairs = dict(zip((n for n, _ in nd), T.group_scales(nd, depth, 0.75, "bias_norm", net.no_weight_decay())))
    assert pairs["head.1.weight"] == (1.0, 1.0) and pairs["norm.weight"] == (1.0, 0.0) and pairs["head.1.bias"] == (1.0, 0.0)
    for i in range(depth):
        assert pairs[f"blocks.{i}.attn.qkv.weight"] == (0.75 ** (depth - i), 1.0)
        assert pairs[f"blocks.{i}.attn.qkv.bias"] == (0.75 ** (depth - i), 0.0)
        assert pairs[f"blocks.{i}.norm1.weight"] == (0.75 ** (depth - i), 0.0)
    for n in net.no_weight_decay():
        assert pairs[n] == (0.75 ** (depth + 1), 0.0)
    assert pairs["patch_embed.proj.weight"] == (0.75 ** (depth + 1), 1.0) and pairs["patch_embed.proj.bias"] == (0.75 ** (depth + 1), 0.0)
    no_wd = {n for n, (_, w) in pairs.items() if w == 0.0}
    assert no_wd == {n for n, d in nd if d <= 1} | set(net.no_weight_decay())
    # names only, no layer decay
    pairs = dict(zip((n for n, _ in nd), T.group_scales(nd, depth, None, net.no_weight_decay(), net.no_weight_decay())))
    assert {n for n, (l, w) in pairs.items() if w == 0.0} == set(net.no_weight_decay()) and {l for l, _ in pairs.values()} == {1.0}
    # a head-only list: the model's names that are not trainable are no error, a name that is nowhere is
    head = [(n, d) for n, d in nd if n.startswith("head.")]
    assert T.group_scales(head, depth, None, net.no_weight_decay(), net.no_weight_decay()) is None
    with pytest.raises(ValueError):
        T.group_scales(head, depth, None, {"no.such.parameter"}, net.no_weight_decay())
    with pytest.raises(ValueError):
        T.group_scales(head, depth, None, "bias", net.no_weight_decay())


def test_train_step_refuses_an_empty_trainable_set_and_groups_without_adamw():
    net = S._net(True).requires_grad_(False)
    with pytest.raises(ValueError, match="requires a gradient"):
        T.TrainStep(net, None)
    net.head_dist.requires_grad_(True)                  # never trained: still nothing to update
    with pytest.raises(ValueError, match="requires a gradient"):
        T.TrainStep(net, None)
    net = _frozen_net("head_only")
    with pytest.raises(ValueError, match="AdamW"):
        T.TrainStep(net, None, optimizer="sgd", no_weight_decay="bias_norm")
    assert all(p.grad is None for p in net.parameters())         # refused before anything was rebound


# ---- ABI of the new entries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, nargs", [("pa_adamw_stage_groups", 17), ("pa_adamw_groups", 16)])
def test_abi_of_the_group_entries(name, nargs):
    import os
    res, args = _lib.SIGNATURES[name]
    assert len(args) == nargs
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "passt_amd.h")).read()
    proto = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert proto is not None and len(proto.group(1).split(",")) == nargs
    lib = _lib.load()
    fn = getattr(lib, name)
    assert len(fn.argtypes) == nargs
    # the descriptor the table shares with pa_adamw_stage is untouched
    assert [f[0] for f in _lib.AdamwStageDesc._fields_] == ["offset", "dst", "dst_t", "rows", "cols", "tile_begin", "reserved"]

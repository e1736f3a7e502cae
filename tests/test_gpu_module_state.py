"""The ground between the kernels and the caller, under real torch usage: (A) the staged weight copies (passt_amd.passt._Staged)
after every route by which weights change behind a plain module, (B) the same through the training drivers -- train, validate,
train again; parameters written from outside between steps --, and (C) the one autograd node under the call patterns torch allows:
two forwards and one backward, a forward between a recorded forward and its backward, another stream, autocast, autograd.grad.

Everything is decided bit for bit by the two checks of tests/module_state_cases.py -- every copy marked current equals the cast of
its parameter; a deepcopy with an empty cache, run under the same seeds, returns the same bits -- or by comparing two runs of the same
launches.  No reference, no tolerance.  Geometry: the SMALL network with model_small_train's Patchout, B=3, T=250.
"""
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from passt_amd import optim as pa_optim  # noqa: E402
from passt_amd._lib import PA_BF16  # noqa: E402
from passt_amd.passt import _Staged  # noqa: E402
from passt_amd.schedule import SWA  # noqa: E402
from passt_amd.train import TrainStep  # noqa: E402
from tests import module_state_cases as MS  # noqa: E402
from tests.module_state_cases import (assert_copies_current, assert_trees_equal, assert_twin_equal, batch, build_small, eval_call,  # noqa: E402
                                      loss_of, train_call)

DEV = "cuda"
DEPTH = 2
LENS_EVAL = [250, 137, 60]          # ragged validation batch: frames per clip
LENS_TRAIN = [250, 180, 130]        # ragged training batch: every clip keeps patches under model_small_train's Patchout
FROZEN = lambda n: n.startswith(("blocks.1.", "norm.", "head."))        # noqa: E731  tests/test_gpu_finetune.py's block1_head


def quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def seed_all(s):
    torch.manual_seed(s)
    np.random.seed(s)


def warm(net, seed=11):
    """one train-mode forward and backward: every copy of the precision exists and is current, every gradient exists"""
    x, y = batch(seed)
    seed_all(seed)
    quiet(train_call(x, y), net)


def check_module(net, num_classes=None):
    """the checks of part A: the copies, the cold twin forward and backward in train mode (input gradient included), the cold twin
    forward in eval mode"""
    xt, yt = batch(21, num_classes=num_classes)
    xv, _ = batch(22)
    net.train()
    net.input_grad = True
    assert_copies_current(net)                              # whatever still claims to be current after the route
    assert_twin_equal(net, train_call(xt, yt, want_dx=True), seed=21, what="train")
    assert assert_copies_current(net) >= 4 * DEPTH
    net.eval()
    assert_twin_equal(net, eval_call(xv), seed=22, what="eval")
    assert assert_copies_current(net) >= 4 * DEPTH
    net.train()


# ---- A. routes on a plain module --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("route", MS.ROUTES, ids=MS.ROUTE_IDS)
def test_route_on_plain_module(route, precision):
    net = build_small(precision).train()
    warm(net)
    if route.name == "adamw_fused" and not MS.fused_accepted(DEV):
        with pytest.raises((RuntimeError, ValueError)):
            route.mutate(net, torch.Generator().manual_seed(5))
        return
    p = MS.one_weight(net)
    before, ver, ptr = p.detach().clone(), p._version, p.data_ptr()
    route.mutate(net, torch.Generator().manual_seed(5))
    assert not torch.equal(p.detach(), before)
    assert (p._version != ver) == route.bumps and (p.data_ptr() != ptr) == route.moves       # the CPU facts hold on the device
    if route.needs_mark:
        net.mark_params_updated()                           # the contract route: the checks run after the call
    check_module(net)


@pytest.mark.parametrize("route", ["data_mul", "data_copy"])
def test_data_write_without_mark_is_what_the_checker_catches(route):
    """the contract route without its call: the copies stay marked current and wrong, and both checkers say so"""
    r = MS.ROUTES[MS.ROUTE_IDS.index(route)]
    net = build_small("bf16").train()
    warm(net)
    r.mutate(net, torch.Generator().manual_seed(5))
    with pytest.raises(AssertionError, match="marked current but differs"):
        assert_copies_current(net)
    net.eval()
    with pytest.raises(AssertionError, match="differs"):
        assert_twin_equal(net, eval_call(batch(22)[0]))


def test_negative_control_blind_cache(monkeypatch):
    """The checkers can fail: with a cache key that never changes, a bf16 train step, an update from outside and a forward give what
    the stale copies give, and the twin comparison raises."""
    monkeypatch.setattr(_Staged, "_version", lambda self, p: 0)
    net = build_small("bf16").train()
    warm(net)
    MS.ROUTES[MS.ROUTE_IDS.index("no_grad_mul")].mutate(net, None)
    net.eval()
    with pytest.raises(AssertionError, match="differs"):
        assert_twin_equal(net, eval_call(batch(22)[0]))
    with pytest.raises(AssertionError, match="marked current but differs"):
        assert_copies_current(net)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_route_module_surgery(precision):
    net = build_small(precision).train()
    warm(net)
    torch.manual_seed(1)
    net.blocks[0].mlp.fc1 = nn.Linear(128, 512).to(DEV)      # same shape, new parameters
    check_module(net)
    net.head[1] = nn.Linear(128, 11).to(DEV)                 # another class count: the output shape follows
    x, _ = batch(23)
    with torch.no_grad():
        assert quiet(net, x)[0].shape == (3, 11)
    check_module(net, num_classes=11)


def test_route_precision_switch():
    """bf16 -> fp32 -> bf16 with an optimizer step between the switches: the copies of the dtype that sat out are stale, not lost"""
    net = build_small("bf16").train()
    warm(net)
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    for precision in ("fp32", "bf16", "fp32", "bf16"):
        opt.step()                                          # on the gradients of the last backward
        net.precision = precision
        check_module(net)
    dts = {k[1] for k in net._staged.cache}
    assert len(dts) == 2


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_route_freeze_then_unfreeze(precision):
    net = build_small(precision).train()
    warm(net)
    x, y = batch(24)
    net.blocks[0].requires_grad_(False)
    seed_all(24)
    quiet(train_call(x, y), net)
    assert net.blocks[0].mlp.fc1.weight.grad is None
    torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-2).step()
    check_module(net)
    net.blocks[0].requires_grad_(True)
    seed_all(25)
    quiet(train_call(x, y), net)
    torch.optim.AdamW(net.parameters(), lr=1e-2).step()
    check_module(net)


# ---- B. training drivers ----------------------------------------------------------------------------------------------------------------
MODES = {
    #  name            (precision, TrainStep keywords, network keywords, marks copies by hand)
    "plain":           ("bf16", {}, {}, True),
    "plain_fp32":      ("fp32", {}, {}, True),
    "no_fused_stage":  ("bf16", {}, {}, False),
    "layer_decay":     ("bf16", dict(layer_decay=0.75), {}, True),
    "clip":            ("bf16", dict(clip_grad_norm=0.5), {}, True),
    "accumulate":      ("bf16", dict(accumulate=2), {}, True),
    "frozen":          ("bf16", {}, {}, True),
    "graph":           ("bf16", dict(graph=True), {}, False),
    "ragged":          ("bf16", {}, {}, True),
    "sgd":             ("bf16", dict(optimizer="sgd"), {}, False),
    "drop_path":       ("bf16", {}, dict(drop_path_rate=0.2), True),
}


def make_driver(mode, seed=12):
    precision, ts_kw, net_kw, by_hand = MODES[mode]
    net = build_small(precision, seed=seed, **net_kw).train()
    if mode == "frozen":
        for n, p in net.named_parameters():
            p.requires_grad_(bool(FROZEN(n)))
    if mode == "ragged":
        net.varlen_train = True
    ts = TrainStep(net, None, lr=1e-2, weight_decay=1e-2, **ts_kw)
    assert ts.fused_stage == (mode not in ("no_fused_stage", "sgd"))
    return net, ts


def do_steps(mode, ts, first, count):
    """steps first .. first + count - 1 of the mode's fixed sequence: batch and seeds are a function of the step number alone"""
    for i in range(first, first + count):
        x, y = batch(200 + i % 2)
        seed_all(300 + i)
        quiet(ts.step, x, y, lengths=LENS_TRAIN if mode == "ragged" else None)


def validate(net):
    """what a validation pass asks of the module, against cold twins"""
    xv, _ = batch(22)
    was = net.training
    net.eval()
    assert_twin_equal(net, eval_call(xv), what="validation")
    assert_twin_equal(net, eval_call(xv, lengths=LENS_EVAL), what="ragged validation")
    assert_twin_equal(net, eval_call(xv, attn=(0,)), what="attn")
    net.train(was)


def state_of(ts):
    return dict(p=ts.flat_p.clone(), m=None if ts.m is None else ts.m.clone(), v=None if ts.v is None else ts.v.clone())


@pytest.mark.parametrize("mode", list(MODES))
def test_train_validate_train(mode, monkeypatch):
    """Train, validate, train again: validation sees the weights the optimizer wrote, and does not move the trajectory."""
    if mode == "no_fused_stage":
        monkeypatch.setenv("PASST_AMD_NO_FUSED_STAGE", "1")
    else:
        monkeypatch.delenv("PASST_AMD_NO_FUSED_STAGE", raising=False)
    # graph: three eager warm-up steps and two replays; accumulate: the validation falls between a folding micro-step and its update
    n1 = {"graph": 5, "accumulate": 3}.get(mode, 2)
    n2 = {"accumulate": 3}.get(mode, 2)
    net, ts = make_driver(mode)
    do_steps(mode, ts, 0, n1)
    if mode == "graph":
        assert ts._g is not None and "graph" in ts._g
    n = assert_copies_current(net)
    if MODES[mode][3]:
        assert n >= 4 * DEPTH
    validate(net)
    assert net.training
    do_steps(mode, ts, n1, n2)
    got = state_of(ts)
    n = assert_copies_current(net)
    if MODES[mode][3]:
        assert n >= 4 * DEPTH
    ref_net, ref_ts = make_driver(mode)
    do_steps(mode, ref_ts, 0, n1 + n2)
    assert ts.t == ref_ts.t
    assert_trees_equal(got, state_of(ref_ts), "interrupted vs uninterrupted run: ")
    assert_trees_equal(dict(net.state_dict()), dict(ref_net.state_dict()), "state_dict: ")
    validate(net)                                           # ... and still holds at the end
    ts.close()
    ref_ts.close()


def test_load_state_dict_between_steps():
    net, ts = make_driver("plain")
    do_steps("plain", ts, 0, 2)
    ptr = net.blocks[0].mlp.fc1.weight.data_ptr()
    MS.ROUTES[MS.ROUTE_IDS.index("load_state_dict")].mutate(net, torch.Generator().manual_seed(5))
    assert net.blocks[0].mlp.fc1.weight.data_ptr() == ptr    # written in place into the flat views
    loaded = ts.flat_p.clone()
    validate(net)
    do_steps("plain", ts, 2, 1)
    assert assert_copies_current(net) >= 4 * DEPTH
    validate(net)
    # the step read the loaded values: a run that is told by hand gives the same bits
    net2, ts2 = make_driver("plain")
    do_steps("plain", ts2, 0, 2)
    ts2.flat_p.copy_(loaded)
    net2.mark_params_updated()
    do_steps("plain", ts2, 2, 1)
    assert_trees_equal(state_of(ts), state_of(ts2), "load_state_dict vs marked restore: ")
    ts.close()
    ts2.close()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_restoring_flat_p_replays_the_same_steps(precision):
    """The only way to restore a TrainStep: write flat_p / m / v, put t back, call net.mark_params_updated().  The steps that followed
    the snapshot then give the same bits again."""
    mode = "plain" if precision == "bf16" else "plain_fp32"
    net, ts = make_driver(mode)
    do_steps(mode, ts, 0, 1)
    saved, t = state_of(ts), ts.t
    do_steps(mode, ts, 1, 2)
    first = state_of(ts)
    assert not torch.equal(first["p"], saved["p"])
    ts.flat_p.copy_(saved["p"])
    ts.m.copy_(saved["m"])
    ts.v.copy_(saved["v"])
    ts.t = t
    net.mark_params_updated()
    assert assert_copies_current(net) == 0                  # every copy is stale now
    do_steps(mode, ts, 1, 2)
    assert_trees_equal(state_of(ts), first, "replayed steps: ")
    validate(net)
    ts.close()


def test_swa_copy_to_the_module_itself():
    net, ts = make_driver("plain")
    swa = SWA(ts)
    for i in range(2):
        do_steps("plain", ts, i, 1)
        swa.update()
    saved = ts.flat_p.clone()
    assert swa.copy_to(net) is net
    assert torch.equal(ts.flat_p, swa.avg) and not torch.equal(saved, swa.avg)
    validate(net)                                           # the averaged weights are what validation runs on
    ts.flat_p.copy_(saved)
    net.mark_params_updated()
    do_steps("plain", ts, 2, 1)
    assert assert_copies_current(net) >= 4 * DEPTH
    ref_net, ref_ts = make_driver("plain")
    do_steps("plain", ref_ts, 0, 3)
    assert_trees_equal(state_of(ts), state_of(ref_ts), "SWA validation in between: ")
    validate(net)
    ts.close()
    ref_ts.close()


def test_flush_after_a_write_to_a_frozen_weight():
    """accumulate=2 on a partly frozen network: a frozen weight written between a folding micro-step and flush() has a new version
    when the update marks the frozen copies current -- only those that WERE current may be marked."""
    net = build_small("bf16").train()
    for n, p in net.named_parameters():
        p.requires_grad_(bool(FROZEN(n)))
    ts = TrainStep(net, None, lr=1e-2, weight_decay=1e-2, accumulate=2)
    do_steps("frozen", ts, 0, 1)
    assert ts._micro == 1 and ts.t == 0
    w = net.blocks[0].mlp.fc1.weight
    key = (id(w), PA_BF16, False)
    st = net._staged
    assert key in st.cache and st.cache[key][0] == st._version(w)        # the forward staged the frozen weight
    with torch.no_grad():
        w.copy_(w.detach() * 1.5)
    ts.flush()
    assert ts._micro == 0 and ts.t == 1
    validate(net)
    assert_copies_current(net)
    # the frozen weights nobody wrote keep their copies current: no restaging in the steady state
    w2 = net.blocks[0].attn.proj.weight
    do_steps("frozen", ts, 1, 2)
    assert st.cache[(id(w2), PA_BF16, False)][0] == st._version(w2)
    assert assert_copies_current(net) >= 4 * DEPTH
    ts.close()


def test_frozen_write_while_the_other_precision_runs():
    """The same rule from another side: a frozen weight written while the network trains in fp32 leaves its bf16 copy stale through
    the fp32 steps (they refresh f32 copies only), and the update at their end must not mark it current."""
    net = build_small("bf16").train()
    for n, p in net.named_parameters():
        p.requires_grad_(bool(FROZEN(n)))
    ts = TrainStep(net, None, lr=1e-2, weight_decay=1e-2)
    do_steps("frozen", ts, 0, 1)
    w = net.blocks[0].mlp.fc1.weight
    assert (id(w), PA_BF16, False) in net._staged.cache
    net.precision = "fp32"
    with torch.no_grad():
        w.copy_(w.detach() * 1.5)
    do_steps("frozen", ts, 1, 2)
    assert_copies_current(net)
    validate(net)
    net.precision = "bf16"
    assert_copies_current(net)
    validate(net)
    do_steps("frozen", ts, 3, 1)
    assert assert_copies_current(net) >= 4 * DEPTH
    validate(net)
    ts.close()


def _optim_steps(net, opt, first, count):
    for i in range(first, first + count):
        x, y = batch(200 + i % 2)
        seed_all(300 + i)
        opt.zero_grad()
        logits, feat = quiet(net, x)
        loss_of(logits, feat, y).backward()
        opt.step()


def test_bound_optim_adamw_train_validate_train():
    runs = []
    for interrupted in (True, False):
        net = build_small("bf16").train()
        opt = pa_optim.AdamW(net.parameters(), lr=1e-2, weight_decay=1e-2)
        _optim_steps(net, opt, 0, 3)
        assert net._flat is not None and opt._bound
        assert assert_copies_current(net) >= 4 * DEPTH
        if interrupted:
            validate(net)
        _optim_steps(net, opt, 3, 2)
        assert net._flat is not None
        assert assert_copies_current(net) >= 4 * DEPTH
        if interrupted:
            validate(net)
        fl = opt._flat[0]
        runs.append(dict(sd=dict(net.state_dict()), m=fl["m"].clone(), v=fl["v"].clone()))
    assert_trees_equal(runs[0], runs[1], "bound optim.AdamW, validation in between: ")


def test_bound_optim_adamw_flat_buffer_write_needs_the_mark():
    """the contract route on the bound optimizer's flat buffer: restore it, mark, and the next forward reads the restored values"""
    net = build_small("bf16").train()
    opt = pa_optim.AdamW(net.parameters(), lr=1e-2, weight_decay=1e-2)
    _optim_steps(net, opt, 0, 2)
    fl = opt._flat[0]
    saved = fl["flat_p"].clone()
    _optim_steps(net, opt, 2, 1)
    fl["flat_p"].copy_(saved)
    with pytest.raises(AssertionError, match="marked current but differs"):
        assert_copies_current(net)
    net.mark_params_updated()
    validate(net)


# ---- C. the autograd node ---------------------------------------------------------------------------------------------------------------
def _grads(net):
    return {n: None if p.grad is None else p.grad.clone() for n, p in net.named_parameters()}


def _clear(net, opt):
    if opt is not None:
        opt.zero_grad()
    else:
        for p in net.parameters():
            p.grad = None


@pytest.mark.parametrize("bound", [False, True], ids=["unbound", "bound"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_two_forwards_one_backward(precision, bound):
    """l1 + l2 over two batches through one net, one backward: g1 + g2 of two separate passes on the same draws (f32 addition is
    commutative, so the order the two nodes run in does not show).  Bound to optim.AdamW the first node to run overwrites the flat
    buffer (the ``fresh`` branch) and the second adds."""
    net = build_small(precision).train()
    opt = None
    if bound:
        opt = pa_optim.AdamW(net.parameters(), lr=1e-2)
        _optim_steps(net, opt, 0, 1)
        assert net._flat is not None
    (x1, y1), (x2, y2) = batch(31), batch(32)
    _clear(net, opt)
    seed_all(31)
    lo1, fe1 = quiet(net, x1)
    rng = torch.get_rng_state()                              # the second forward's Patchout draws start here
    lo2, fe2 = quiet(net, x2)
    (loss_of(lo1, fe1, y1) + loss_of(lo2, fe2, y2)).backward()
    both = _grads(net)
    _clear(net, opt)
    seed_all(31)
    a1, b1 = quiet(net, x1)
    loss_of(a1, b1, y1).backward()
    g1 = _grads(net)
    _clear(net, opt)
    torch.set_rng_state(rng)
    a2, b2 = quiet(net, x2)
    loss_of(a2, b2, y2).backward()
    g2 = _grads(net)
    assert_trees_equal([lo1, fe1, lo2, fe2], [a1, b1, a2, b2], "forwards: ")
    want = {n: None if g1[n] is None else g1[n] + g2[n] for n in g1}
    assert sum(g is not None for g in want.values()) > 20 and float(want["blocks.0.mlp.fc1.weight"].abs().max()) > 0
    assert_trees_equal(both, want, "two forwards, one backward: ")
    assert (net._flat is not None) == bound


@pytest.mark.parametrize("intruder", ["eval_no_grad", "recorded_dropped"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_forward_between_forward_and_backward(precision, intruder):
    """a forward of another batch of another shape between a recorded forward and its backward: the shared workspaces of
    model._scratch (part, colsum_ws, grad_dump, side) belong to whoever runs, the saved activations to the node"""
    net = build_small(precision).train()
    x, y = batch(33)
    xo, _ = batch(34, B=2, T=200)
    seed_all(33)
    want = quiet(train_call(x, y), net)
    _clear(net, None)
    seed_all(33)
    logits, feat = quiet(net, x)
    if intruder == "eval_no_grad":
        net.eval()
        with torch.no_grad():
            other = quiet(net, xo)
        net.train()
        assert other[0].shape == (2, 37) and other[0].grad_fn is None
    else:
        other = quiet(net, xo)                              # records a graph that is dropped unused
        assert other[0].grad_fn is not None
        del other
    loss_of(logits, feat, y).backward()
    got = dict(logits=logits.detach(), feat=feat.detach(), dx=None, grads=_grads(net))
    assert_trees_equal(got, want, f"{intruder}: ")


@pytest.mark.parametrize("overlap", [False, True], ids=["serial_wgrad", "overlap_wgrad"])
def test_non_default_stream(overlap):
    net = build_small("bf16").train()
    net.overlap_wgrad = overlap
    net.input_grad = True
    x, y = batch(35)
    call = train_call(x, y, want_dx=True)
    seed_all(35)
    want = quiet(call, net)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    seed_all(35)
    with torch.cuda.stream(s):
        got = quiet(call, net)
    s.synchronize()
    torch.cuda.synchronize()
    assert_trees_equal(got, want, "stream: ")
    assert assert_copies_current(net) >= 4 * DEPTH


def test_autocast_is_invisible_to_the_node():
    net = build_small("bf16").train()
    net.input_grad = True
    x, y = batch(36)
    call = train_call(x, y, want_dx=True)
    seed_all(36)
    want = quiet(call, net)
    seed_all(36)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = quiet(call, net)
    assert_trees_equal(got, want, "autocast, precision='bf16': ")
    # precision=None follows autocast: the bf16 kernels, f32 outputs
    net.precision = None
    seed_all(36)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = quiet(call, net)
    assert got["logits"].dtype == torch.float32 and got["dx"].dtype == torch.float32
    assert_trees_equal(got, want, "autocast, precision=None: ")
    # ... and the f32 kernels under an explicit precision, autocast or not
    net.precision = "fp32"
    seed_all(36)
    want32 = quiet(call, net)
    seed_all(36)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = quiet(call, net)
    assert_trees_equal(got, want32, "autocast, precision='fp32': ")
    assert not torch.equal(want32["logits"], want["logits"])


def test_bf16_input_is_converted():
    """_checked_input: an x that arrives in bf16 is converted to f32 (x.contiguous().float()), with or without a graph; x.grad comes
    back in x's own dtype"""
    net = build_small("bf16").eval()
    x, y = batch(37)
    xb = x.bfloat16()
    with torch.no_grad():
        assert_trees_equal(list(quiet(net, xb)), list(quiet(net, xb.float())), "bf16 x, no graph: ")
    net.train()
    seed_all(37)
    a = quiet(net, xb)
    seed_all(37)
    b = quiet(net, xb.float())
    assert a[0].grad_fn is not None and a[0].dtype == torch.float32
    assert_trees_equal([t.detach() for t in a], [t.detach() for t in b], "bf16 x, recorded: ")
    net.input_grad = True
    xg = xb.clone().requires_grad_(True)
    xf = xb.float().requires_grad_(True)
    seed_all(37)
    loss_of(*quiet(net, xg), y).backward()
    seed_all(37)
    loss_of(*quiet(net, xf), y).backward()
    assert xg.grad.dtype == torch.bfloat16 and torch.equal(xg.grad, xf.grad.bfloat16())


def test_autograd_grad_on_a_subset_of_the_inputs():
    """torch.autograd.grad(loss, [x]) and torch.autograd.grad(loss, the parameters of whole stages) against the matching entries of a
    full backward.  What the node computes follows from which of its inputs REQUIRE a gradient (ctx.needs_input_grad), not from which
    ones torch.autograd.grad asks for: the launches are the full backward's, torch drops the rest, nothing lands in ``p.grad``.  The
    subset is block 1, the final norm and the head (whole stages)."""
    net = build_small("bf16").train()
    net.input_grad = True
    x, y = batch(38)
    seed_all(38)
    want = quiet(train_call(x, y, want_dx=True), net)
    _clear(net, None)
    xx = x.clone().requires_grad_(True)
    seed_all(38)
    logits, feat = quiet(net, xx)
    (dx,) = torch.autograd.grad(loss_of(logits, feat, y), [xx])
    assert all(p.grad is None for p in net.parameters())
    assert_trees_equal([logits.detach(), feat.detach(), dx], [want["logits"], want["feat"], want["dx"]], "autograd.grad(loss, [x]): ")
    named = [(n, p) for n, p in net.named_parameters() if FROZEN(n)]
    assert len(named) > 10
    seed_all(38)
    logits, feat = quiet(net, x)
    gs = torch.autograd.grad(loss_of(logits, feat, y), [p for _, p in named])
    assert all(p.grad is None for p in net.parameters())
    assert_trees_equal({n: g for (n, _), g in zip(named, gs)}, {n: want["grads"][n] for n, _ in named}, "autograd.grad(loss, subset): ")

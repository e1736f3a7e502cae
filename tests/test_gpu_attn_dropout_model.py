"""Attention dropout through the model on the HIP path: against the real reference's fixture (tests/golden/attn_dropout.npz: the
reference's own forward and backward with the rule's masks in place of its ``attn_drop`` draws), and the invariants of the interface
(prefix tail = full tail, eval / p = 0, replay, captured graph).

Bounds: those tests/test_gpu_drop_path.py::test_model_vs_reference_fixture applies to its fixture -- 1e-3 in fp32 and BF16_LOGITS /
BF16_GRADS of tests/test_gpu_model.py in bf16.  Every measured value is printed and recorded before it is asserted.

Every test fails on the parent commit at the missing ``attn_drop_seed`` argument or at the missing dropout entries."""
import gc
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from passt_amd import passt as P  # noqa: E402
from tests.golden import make_attn_dropout_golden as AG  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_hidden_golden as HG  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, BF16_LOGITS, DEV, rel  # noqa: E402
from tests.test_gpu_model import record as record_model  # noqa: E402

LIM = {"fp32": (1e-3, 1e-3), "bf16": (BF16_LOGITS, BF16_GRADS)}      # (outputs, gradients): test_model_vs_reference_fixture's


@pytest.fixture(autouse=True)
def _collect_models():
    """The models of these tests end in reference cycles (autograd nodes, tracebacks of the refusals): collect them here, so that no
    later test sees a live PaSST disappear under its hands (passt._LIVE is a weak set)."""
    yield
    gc.collect()


def record(name, **kw):
    record_model(name, **kw)
    print(name, {k: float(v) for k, v in kw.items()})


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def build(case, precision, rates=AG.RATES):
    cfg = case["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.PaSST(u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"], s_patchout_f=cfg["s_patchout_f"],
                            img_size=cfg["img_size"], patch_size=cfg["patch"], stride=cfg["stride"], num_classes=cfg["num_classes"],
                            embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"], distilled=True)
    sd = detgen.passt_state_dict(cfg, case["seed"])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    if rates is not None:
        for blk, p in zip(m.blocks, rates):
            blk.attn.attn_drop.p = p                                   # the reference user's line
    m.precision = precision
    return m.to(DEV)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "attn_dropout.npz")))


def _step(m, case, route, seed=AG.SEED, hidden=None):
    """(logits, features, dx, {parameter: gradient}) of one train-mode step of the fixture's loss under ``seed``: ``route`` "autograd" =
    net(x); loss.backward(), "direct" = passt_forward / passt_backward.  ``hidden``: asked for as well (the last block: the full tail)."""
    x, a, b = HG.inputs(case)
    torch.manual_seed(case["torch_seed"])              # the Patchout draws are the fixture's
    kw = {} if seed is None else dict(attn_drop_seed=seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if route == "autograd":
            m.input_grad = True
            m.zero_grad()
            xg = _dev(x).requires_grad_(True)
            out = m(xg, **kw) if hidden is None else m(xg, hidden=hidden, **kw)
            ((out[0] * _dev(a)).sum() + (out[1] * _dev(b)).sum()).backward()
            grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
            return out[0].detach(), out[1].detach(), xg.grad, grads
        assert hidden is None
        logits, feat, ctx = P.passt_forward(m, _dev(x), True, **kw)
        grads = {n: torch.full_like(p, float("nan")) for n, p in m.named_parameters() if not n.startswith("head_dist.")}
        dx = P.passt_backward(m, ctx, _dev(a), _dev(b), grads, want_dx=True)
        return logits, feat, dx, grads


def _metrics(case, name, gold, logits, feat, dx, grads):
    met = dict(logits=rel(logits.cpu(), gold[name + ".logits"]), features=rel(feat.cpu(), gold[name + ".features"]),
               dx=rel(G.pin_sample(dx.cpu().numpy(), AG.SAMPLE), gold[name + ".dx"]))
    for k in AG.PARAM_GRADS:
        met["grad." + k] = rel(G.pin_sample(grads[k].cpu().numpy(), AG.SAMPLE), gold[f"{name}.grad.{k}"])
    return met


def _assert(met, precision):
    lim_out, lim_g = LIM[precision]
    for k, v in met.items():
        assert v < (lim_g if k.startswith(("dx", "grad.")) else lim_out), (k, v, met)


@pytest.mark.parametrize("name", list(AG.CASES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("route", ["autograd", "direct"])
def test_model_vs_reference_fixture(gold, name, precision, route):
    case = AG.CASES[name]
    m = build(case, precision).train()
    assert P.attn_drop_rates(m) == [0, 64, 128]
    logits, feat, dx, grads = _step(m, case, route)
    assert dx.shape == (case["B"], 1, case["cfg"]["img_size"][0], case["T"])
    met = _metrics(case, name, gold, logits, feat, dx, grads)
    record(f"attn_dropout.model.{name}[{precision},{route}]", **met)
    _assert(met, precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_prefix_tail_equals_full_tail(gold, precision):
    """hidden=(last,) makes the last block run on all rows: the mask of the cls / dist rows is the same, so the outputs and gradients
    agree with the prefix-only tail's within the fixture's bounds (and with the fixture)."""
    name = "patchout"
    case = AG.CASES[name]
    m = build(case, precision).train()
    base = _step(m, case, "autograd")
    full = _step(m, case, "autograd", hidden=(AG.DEPTH - 1,))
    met = dict(logits=rel(full[0].cpu(), base[0].cpu()), features=rel(full[1].cpu(), base[1].cpu()), dx=rel(full[2].cpu(), base[2].cpu()))
    for k in AG.PARAM_GRADS:
        met["grad." + k] = rel(full[3][k].cpu(), base[3][k].cpu())
    record(f"attn_dropout.model.full_tail_vs_prefix[{precision}]", **met)
    _assert(met, precision)
    _assert(_metrics(case, name, gold, *full), precision)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_eval_and_zero_rates_equal_a_model_never_touched(precision):
    case = AG.CASES["patchout"]
    x = _dev(HG.inputs(case)[0])

    def run(m, train, **kw):
        torch.manual_seed(case["torch_seed"])
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = m.train(train)(x, **kw)
        return out, torch.cuda.get_rng_state()
    plain_e, st_e = run(build(case, precision, None), False)
    plain_t, st_t = run(build(case, precision, None), True)
    got_e, gst_e = run(build(case, precision), False, attn_drop_seed=(1, 2))             # ignored in eval mode
    got_t, gst_t = run(build(case, precision, (0.0, 0.0, 0.0)), True)
    for a, b in ((plain_e, got_e), (plain_t, got_t)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(st_e, gst_e) and torch.equal(st_t, gst_t)                          # nothing drawn
    # an active model draws once on the device and differs
    act, ast = run(build(case, precision), True)
    assert not torch.equal(act[0], plain_t[0]) and not torch.equal(ast, st_t)


def test_same_seed_replays_and_another_seed_differs():
    case = AG.CASES["plain"]
    m = build(case, "bf16").train()
    a = _step(m, case, "autograd")
    b = _step(m, case, "autograd", seed=torch.tensor([AG.SEED[0] - 2 ** 32 if AG.SEED[0] >= 2 ** 31 else AG.SEED[0],
                                                      AG.SEED[1] - 2 ** 32 if AG.SEED[1] >= 2 ** 31 else AG.SEED[1]], dtype=torch.int32))
    c = _step(m, case, "autograd", seed=(AG.SEED[0] ^ 1, AG.SEED[1]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in AG.PARAM_GRADS:
        assert torch.equal(a[3][k], b[3][k]), k
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2])
    # a drawn seed: the device generator's, and a replay with it is bit-identical
    torch.manual_seed(321)
    want = P.attn_drop_draw(torch.device(DEV))
    x = _dev(HG.inputs(case)[0])
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(321)
        drawn = m(x)
        fed = m(x, attn_drop_seed=want)
    assert torch.equal(drawn[0], fed[0]) and torch.equal(drawn[1], fed[1])


def test_train_step_graph_equals_eager_with_attention_dropout():
    """TrainStep(graph=True) with attn_drop.p = 0.1 on every block: the step's seed is drawn ahead of the replay into a buffer of fixed
    address; 3 warm-up steps and 2 replayed ones leave the parameters and moments of the eager TrainStep, bit for bit."""
    from passt_amd.train import TrainStep
    case = dict(G.CASES["model_small_train"], seed=962)
    x, y = G.model_inputs(case)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    outs = []
    for graph in (False, True):
        net = build(case, "bf16", (0.1,) * case["cfg"]["depth"]).train()
        ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=True, graph=graph)
        losses = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for step in range(5):
                torch.manual_seed(90 + step)
                np.random.seed(90 + step)
                losses.append(ts.step(xg, yg).clone())
        torch.cuda.synchronize()
        assert ts.t == 5 and (not graph or ("graph" in ts._g and ts._g["ad"] is not None))
        outs.append((torch.cat([l.reshape(1) for l in losses]).cpu(), ts.flat_p.clone(), ts.m.clone(), ts.v.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # and the steps differ from a run without dropout (the entries really ran)
    net = build(case, "bf16", None).train()
    ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=True, graph=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(90)
        np.random.seed(90)
        first = ts.step(xg, yg).clone()
    assert not torch.equal(first.cpu().reshape(1), outs[0][0][:1])

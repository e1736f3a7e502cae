"""Stochastic depth (drop_path_rate > 0) without a GPU: the constructor and the module tree, the draws against the live reference and
against the masks the reference's own run left in tests/golden/drop_path.npz, the host expansion to rows, and -- in the recorder
harness of tests/test_sequence_cpu.py -- which launches of the kernel sequence get a row factor.

Every test fails on the parent commit: ``PaSST(..., drop_path_rate=0.5)`` raises NotImplementedError there."""
import copy
import os
import pickle
import warnings

import numpy as np
import pytest
import torch
from torch import nn

import passt_amd
from oracle import ref_import
from passt_amd import ops
from passt_amd import passt as P
from tests import test_sequence_cpu as S
from tests.golden import make_drop_path_golden as DG

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drop_path.npz")
SMALL = dict(img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, num_heads=2, distilled=True)


def _net(depth=3, rate=0.5, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return passt_amd.PaSST(depth=depth, drop_path_rate=rate, **dict(SMALL, **kw))


def test_constructor_places_drop_path_where_linspace_puts_it():
    net = _net(depth=5, rate=0.2)
    want = [r.item() for r in torch.linspace(0, 0.2, 5)]
    for blk, p in zip(net.blocks, want):
        if p > 0:
            assert isinstance(blk.drop_path, P.DropPath) and blk.drop_path.drop_prob == p
            assert not blk.drop_path.state_dict() and not list(blk.drop_path.parameters())
        else:
            assert isinstance(blk.drop_path, nn.Identity)
    assert [type(b.drop_path) for b in _net(depth=3, rate=0.0).blocks] == [nn.Identity] * 3
    # the state_dict is that of a model without stochastic depth; copies and pickles keep the rates
    assert list(net.state_dict()) == list(_net(depth=5, rate=0.0).state_dict())
    rates = lambda m: [getattr(b.drop_path, "drop_prob", 0.0) for b in m.blocks]  # noqa: E731
    want0 = [p if p > 0 else 0.0 for p in want]
    for twin in (copy.deepcopy(net), pickle.loads(pickle.dumps(net))):
        assert rates(twin) == want0
    assert rates(P.lighten_model(copy.deepcopy(net), cut_depth=2)) == [want0[0], want0[3], want0[4]]
    for bad in (dict(drop_rate=0.1), dict(attn_drop_rate=0.1)):
        with pytest.raises(NotImplementedError):
            _net(**bad)


def test_drop_path_module_forward_is_the_reference_arithmetic():
    m = P.DropPath(0.25).train()
    x = torch.ones(64, 3, 5)
    torch.manual_seed(5)
    y = m(x)
    torch.manual_seed(5)
    u = torch.rand((64, 1, 1))
    assert torch.equal(y, x.div(0.75) * (0.75 + u).floor())
    assert m.eval()(x) is x and P.DropPath(0.0).train()(x) is x


@pytest.mark.skipif(not ref_import.reference_available(), reason="reference checkout not available")
@pytest.mark.parametrize("seed", [0, 17])
def test_draws_equal_the_live_reference_modules(seed):
    """After the same seed, drop_path_draws gives per call what the reference's DropPath modules return for an all-ones input, called
    in block order (attention branch, MLP branch), and leaves the generator where they leave it."""
    B, depth, rate = 7, 4, 0.3
    net = _net(depth=depth, rate=rate).train()
    ref_passt, _ = ref_import.load_reference()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = ref_import.run_silently(ref_passt.PaSST, img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, depth=depth,
                                      num_heads=2, distilled=True, drop_path_rate=rate).train()
    torch.manual_seed(seed)
    want = torch.ones(depth, 2, B)
    for i, blk in enumerate(ref.blocks):
        if not isinstance(blk.drop_path, nn.Identity):
            for j in range(2):
                want[i, j] = blk.drop_path(torch.ones(B, 3, 4))[:, 0, 0]
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    got = P.drop_path_draws(net, B, "cpu")
    assert got.dtype == torch.float32 and got.shape == (depth, 2, B)
    assert torch.equal(got, want) and torch.equal(torch.get_rng_state(), state)
    assert set(got[0].flatten().tolist()) == {1.0}                     # block 0: linspace starts at 0
    # eval mode: nothing is drawn
    torch.manual_seed(seed)
    state = torch.get_rng_state()
    assert torch.equal(P.drop_path_draws(net.eval(), B, "cpu"), torch.ones(depth, 2, B)) and torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("name", list(DG.CASES))
def test_draws_equal_the_masks_of_the_reference_run(name):
    """The fixture's masks came out of the reference's forward, where the Patchout draws and the mask draws share the CPU generator:
    the host part of this forward (patchout_draws, then drop_path_draws) must leave the same masks."""
    gold = np.load(GOLDEN)
    case = DG.CASES[name]
    cfg = case["cfg"]
    net = _net(depth=cfg["depth"], rate=DG.RATE, u_patchout=cfg["u_patchout"], s_patchout_t=cfg["s_patchout_t"],
               s_patchout_f=cfg["s_patchout_f"]).train()
    torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P.patchout_draws(net, (case["B"], 1, cfg["img_size"][0], case["T"]))
    d = P.drop_path_draws(net, case["B"], "cpu")
    masks = torch.from_numpy(gold[name + ".masks"])
    assert torch.equal((d > 0).float(), masks)
    assert DG.masks_are_telling(gold[name + ".masks"], [1, 2])
    # fed back as flags they give the same factors, and entries of the block without a DropPath are ignored
    junk = masks.clone()
    junk[0] = 0
    assert torch.equal(P.drop_path_scales(net, junk, case["B"], "cpu"), d)
    with pytest.raises(ValueError):
        P.drop_path_scales(net, masks[:, :, :-1], case["B"], "cpu")


def test_rows_expansion():
    net = _net().train()
    B, ntok = 4, 7
    scales = torch.arange(3 * 2 * B, dtype=torch.float32).view(3, 2, B)
    rows = P._DropRows(scales, P.drop_path_rates(net), ntok)
    assert rows.full.shape == (3, 2, B * ntok) and rows.tail.shape == (2, 2 * B)
    for i in (1, 2):
        for j in range(2):
            r = rows.rows(i, j)
            assert r.is_contiguous() and torch.equal(r.view(B, ntok), scales[i, j].view(B, 1).expand(B, ntok))
    for j in range(2):
        assert torch.equal(rows.rows(2, j, compact=True).view(B, 2), scales[2, j].view(B, 1).expand(B, 2))
    assert rows.rows(0, 0) is None and rows.rows(0, 1) is None and rows.rows(-1, 1) is None
    # no active module: no rows at all
    lay = P._FixedLayout(net, B, ntok)
    assert P._drop_rows(net.eval(), lay, scales) is None and P._drop_rows(_net(rate=0.0).train(), lay, scales) is None


def _with_rowscale(fn):
    return lambda *a, rowscale=None, **k: fn(*a, **k)


def _trace(net, precision, lengths=None):
    """The launches of one forward + backward through the public kernel-sequence functions, in test_sequence_cpu's recorder; the
    stand-ins of the four ops that can take a factor accept the keyword."""
    def case(rec, mp):
        for name in ("linear_resid", "layernorm_bwd", "layernorm_bwd2", "convert"):
            mp.setattr(ops, name, rec.op(name, _with_rowscale(S._RESULTS[name])))
        net.precision = precision
        S._direct(rec, net, S._fixed_fwd, P.passt_backward)
    return S._record(case)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_which_launches_get_a_factor(precision):
    net = _net(s_patchout_t=6, s_patchout_f=3).train()
    trace = _trace(net, precision)
    B = S.X_SHAPE[0]
    scaled = [(e[0], e[2]["rowscale"]) for e in trace if "rowscale" in e[2]]
    M = next(e[1][0] for e in trace if e[0] == "layernorm_fwd")         # "f32[M, D]" of the first LayerNorm
    M = int(M[M.index("[") + 1:M.index(",")])
    full, tail = f"f32[{M}]", f"f32[{2 * B}]"
    assert scaled == [
        ("linear_resid", full), ("linear_resid", full),                  # block 1: proj, fc2
        ("linear_resid", tail), ("linear_resid", tail),                  # block 2, the prefix-only tail: proj, fc2 on compact rows
        ("convert", tail),                                               # the head's gradient enters block 2's MLP branch
        ("layernorm_bwd", tail),                                         # block 2 norm2: proj of block 2
        ("layernorm_bwd", full),                                         # block 2 norm1: fc2 of block 1
        ("layernorm_bwd", full),                                         # block 1 norm2: proj of block 1
    ], scaled                                                            # block 1 norm1 feeds fc2 of block 0, block 0's norms nothing: no factor
    ln = [e for e in trace if e[0] == "layernorm_bwd"]
    assert len(ln) == 6 and ["rowscale" in e[2] for e in ln] == [True, True, True, False, False, False]
    # rate 0 and eval: the keyword is never passed
    for quiet in (_net(rate=0.0, s_patchout_t=6, s_patchout_f=3).train(), net.eval()):
        assert not [e for e in _trace(quiet, precision) if "rowscale" in e[2]]


def test_eval_and_rate_zero_launch_what_they_always_launched():
    """A model built with a rate runs, in eval mode, the launch sequence of a model without one (same ops, same arguments)."""
    def run(net):
        def case(rec, mp):
            net.precision = "bf16"
            with torch.no_grad():
                rec.log("returned", net(torch.zeros(S.X_SHAPE)))
        return S._record(case)
    assert run(_net(rate=0.5).eval()) == run(_net(rate=0.0).eval())


def test_ragged_training_with_drop_path_raises():
    net = _net().train()
    net.varlen_train = True
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        net(torch.zeros(S.X_SHAPE), lengths=S.LENGTHS)
    state = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="drop_path_rate"):
        P.passt_forward_varlen(net, torch.zeros(S.X_SHAPE), S.LENGTHS)
    assert torch.equal(torch.get_rng_state(), state)                     # nothing drawn

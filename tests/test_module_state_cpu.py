"""CPU half of the module-state tests: (1) what torch does to a parameter's version counter and storage on every route of
tests/module_state_cases.py -- the facts the staged-copy cache key ``(p._version, p.data_ptr(), epoch)`` rests on --, and (2) the
bookkeeping of passt_amd.passt._Staged itself with torch stand-ins for the four kernels it launches."""
import copy

import pytest
import torch
import torch.nn as nn

from passt_amd import ops, passt
from passt_amd._lib import PA_BF16, PA_F32
from passt_amd.passt import _Staged
from tests import module_state_cases as MS

TD = {PA_F32: torch.float32, PA_BF16: torch.bfloat16}


def _linear_with_grads():
    torch.manual_seed(3)
    lin = nn.Linear(6, 4)
    lin(torch.randn(5, 6)).square().sum().backward()
    return lin


# ---- 1. version facts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", MS.ROUTES, ids=MS.ROUTE_IDS)
def test_route_version_facts(route):
    """Every route changes the values; it bumps ``_version`` or not, moves the storage or not, as the table says.  A route that does
    neither must be one the table sends through mark_params_updated() -- or torch's fused optimizer, which the step hook covers."""
    if route.name == "adamw_fused" and not MS.fused_accepted("cpu"):
        with pytest.raises((RuntimeError, ValueError)):
            torch.optim.AdamW(_linear_with_grads().parameters(), fused=True)
        return
    lin = _linear_with_grads()
    p = MS.one_weight(lin)
    before, ver, ptr = p.detach().clone(), p._version, p.data_ptr()
    route.mutate(lin, torch.Generator().manual_seed(5))
    assert MS.one_weight(lin) is p
    assert not torch.equal(p.detach(), before), "the route changed nothing"
    assert (p._version != ver) == route.bumps, (route.name, p._version - ver)
    assert (p.data_ptr() != ptr) == route.moves, route.name
    seen = route.bumps or route.moves
    assert seen or route.needs_mark or route.name == "adamw_fused"
    assert not (seen and route.needs_mark)


def test_fused_step_hook_marks_the_models_it_touches():
    """The one route torch hides from the version counters without the caller writing ``.data``: after a fused optimizer's step
    every live PaSST that holds a copy of one of its parameters has a new epoch; other models and other optimizers do not."""
    class Net:                                               # what the hook reads of a model
        def __init__(self):
            self._staged, self.marks = _Staged(), 0

        def mark_params_updated(self):
            self.marks += 1

    a, b, idle = Net(), Net(), Net()
    pa, pb = nn.Parameter(torch.zeros(2, 2)), nn.Parameter(torch.zeros(2, 2))
    a._staged.cache[(id(pa), PA_BF16, False)] = [None, None, pa]
    b._staged.cache[(id(pb), PA_BF16, False)] = [None, None, pb]
    live = list(passt._LIVE)
    try:
        for n in (a, b, idle):
            passt._LIVE.add(n)
        pa.grad = torch.ones(2, 2)
        torch.optim.SGD([pa], lr=0.1).step()                 # bumps the version itself: no mark
        assert (a.marks, b.marks, idle.marks) == (0, 0, 0)
        if MS.fused_accepted("cpu"):
            torch.optim.AdamW([pa], lr=0.1, fused=True).step()
            assert (a.marks, b.marks, idle.marks) == (1, 0, 0)
            sch_opt = torch.optim.Adam([pa], lr=0.1, fused=True)
            torch.optim.lr_scheduler.LambdaLR(sch_opt, lambda e: 1.0)        # a scheduler wraps step(): the hook still fires
            sch_opt.step()
            assert (a.marks, b.marks, idle.marks) == (2, 0, 0)
        passt._after_fused_step(type("Opt", (), dict(param_groups=[dict(params=[pa, pb], fused=True)]))(), (), {})
        assert b.marks == 1 and idle.marks == 0
        passt._after_fused_step(type("Opt", (), dict(param_groups=[dict(params=[pa, pb], fused=None)]))(), (), {})
        assert b.marks == 1
    finally:
        for n in (a, b, idle):
            passt._LIVE.discard(n)
    assert list(passt._LIVE) == live


# ---- 2. _Staged with stand-in kernels ---------------------------------------------------------------------------------------------------
class StandIns:
    """ops.convert / transpose / make_stage_table / stage_weights / make_adamw_stage_table in torch on the CPU, counting launches"""

    def __init__(self, monkeypatch):
        self.calls = dict(convert=0, transpose=0, stage_weights=0, make_stage_table=0, make_adamw_stage_table=0)
        for name in self.calls:
            monkeypatch.setattr(ops, name, getattr(self, name))

    def convert(self, x, dtype, rowscale=None):
        self.calls["convert"] += 1
        return x.to(TD[dtype]).clone()

    def transpose(self, x, dtype, ldo=None, out=None):
        self.calls["transpose"] += 1
        return x.t().contiguous().to(TD[dtype])

    def make_stage_table(self, entries, device):
        self.calls["make_stage_table"] += 1
        return list(entries), len(entries), 0

    def stage_weights(self, table, n, tiles, dtype):
        self.calls["stage_weights"] += 1
        assert n == len(table)
        for src, dst, dst_t in table:
            if dst is not None:
                dst.copy_(src.to(dst.dtype))
            if dst_t is not None:
                dst_t.copy_(src.t().to(dst_t.dtype))

    def make_adamw_stage_table(self, entries, device):
        self.calls["make_adamw_stage_table"] += 1
        return list(entries), len(entries), 0


class Holder:
    """what assert_copies_current reads of a model"""

    def __init__(self, st, params):
        self._staged, self._params = st, params

    def named_parameters(self):
        return list(self._params.items())


@pytest.fixture
def staged(monkeypatch):
    k = StandIns(monkeypatch)
    torch.manual_seed(0)
    ps = {"a": nn.Parameter(torch.randn(4, 6)), "b": nn.Parameter(torch.randn(3, 2, 5)), "c": nn.Parameter(torch.randn(8, 4))}
    st = _Staged()
    for p in ps.values():
        st.get(p, PA_BF16, False)
        st.get(p, PA_BF16, True)
    return st, ps, k, Holder(st, ps)


def test_staged_first_use_makes_one_copy_each(staged):
    st, ps, k, net = staged
    assert (k.calls["convert"], k.calls["transpose"], k.calls["stage_weights"]) == (3, 3, 0)
    assert len(st.cache) == 6 and st.gen == 6
    assert st.get(ps["b"], PA_BF16, True).shape == (10, 3)                  # [rows][rest] transposed
    assert MS.assert_copies_current(net) == 6
    # f32, not transposed: the parameter itself, nothing cached
    w = st.get(ps["a"], PA_F32, False)
    assert w.data_ptr() == ps["a"].data_ptr() and len(st.cache) == 6


def test_staged_unchanged_key_returns_the_same_tensor(staged):
    st, ps, k, net = staged
    before = dict(k.calls)
    for p in ps.values():
        assert st.get(p, PA_BF16, False) is st.cache[(id(p), PA_BF16, False)][1]
        assert st.get(p, PA_BF16, True) is st.get(p, PA_BF16, True)
    assert k.calls == before and st.gen == 6


def test_staged_version_bump_triggers_one_batched_refresh(staged):
    st, ps, k, net = staged
    outs = {key: ent[1] for key, ent in st.cache.items()}
    with torch.no_grad():
        for p in ps.values():                                # an optimizer step: every parameter written in place
            p.add_(1.0)
    assert MS.assert_copies_current(net) == 0                # all stale, none claims to be current
    got = st.get(ps["a"], PA_BF16, False)
    assert k.calls["stage_weights"] == 1 and k.calls["make_stage_table"] == 1
    assert got is outs[(id(ps["a"]), PA_BF16, False)]       # refreshed in place
    assert MS.assert_copies_current(net) == 6                # ... and with it every other copy of the dtype
    for p in ps.values():
        st.get(p, PA_BF16, True)
    assert k.calls["stage_weights"] == 1 and (k.calls["convert"], k.calls["transpose"]) == (3, 3) and st.gen == 6
    with torch.no_grad():
        ps["c"].mul_(2.0)                                    # one parameter alone: again one batched launch, same table
    st.get(ps["c"], PA_BF16, True)
    assert k.calls["stage_weights"] == 2 and k.calls["make_stage_table"] == 1
    assert MS.assert_copies_current(net) == 6


def test_staged_refresh_is_per_dtype(staged):
    st, ps, k, net = staged
    t32 = st.get(ps["a"], PA_F32, True)
    assert t32.dtype == torch.float32 and st.gen == 7
    with torch.no_grad():
        ps["a"].add_(1.0)
    st.get(ps["a"], PA_BF16, False)                          # refreshes the bf16 copies only
    assert MS.assert_copies_current(net) == 6
    assert st.cache[(id(ps["a"]), PA_F32, True)][0] != st._version(ps["a"])
    assert st.get(ps["a"], PA_F32, True) is t32 and MS.assert_copies_current(net) == 7


def test_staged_new_storage_makes_a_new_copy_and_bumps_gen(staged):
    st, ps, k, net = staged
    old = st.get(ps["a"], PA_BF16, False)
    ver = ps["a"]._version
    ps["a"].data = ps["a"].detach() * 3.0
    assert ps["a"]._version == ver                           # only the storage tells
    new = st.get(ps["a"], PA_BF16, False)
    assert new is not old and st.gen == 7 and k.calls["convert"] == 4 and k.calls["stage_weights"] == 0
    assert torch.equal(new, (ps["a"].detach()).to(torch.bfloat16))
    assert PA_BF16 not in st.tables                          # the batched table names the old tensors: dropped
    # the transposed copy of the same parameter is still marked with the old storage: stale, re-made on use
    assert MS.assert_copies_current(net) == 5
    st.get(ps["a"], PA_BF16, True)
    assert MS.assert_copies_current(net) == 6 and st.gen == 8


def test_staged_data_write_is_invisible_until_marked(staged):
    """``p.data.mul_()`` changes neither version nor storage: the copy stays marked current AND WRONG -- what assert_copies_current
    exists to catch -- until mark_params_updated's epoch bump."""
    st, ps, k, net = staged
    ps["a"].data.mul_(2.0)
    assert st.get(ps["a"], PA_BF16, False) is st.cache[(id(ps["a"]), PA_BF16, False)][1] and k.calls["stage_weights"] == 0
    with pytest.raises(AssertionError, match="marked current but differs"):
        MS.assert_copies_current(net)
    st.epoch += 1                                            # PaSST.mark_params_updated
    assert MS.assert_copies_current(net) == 0                # every copy stale
    st.get(ps["a"], PA_BF16, False)
    assert k.calls["stage_weights"] == 1 and MS.assert_copies_current(net) == 6


def test_staged_mark_fresh_leaves_other_keys_stale(staged):
    st, ps, k, net = staged
    st.epoch += 1
    keys = [(id(ps["a"]), PA_BF16, False), (id(ps["a"]), PA_BF16, True), (id(ps["a"]), PA_F32, True)]      # the last one: unknown, ignored
    st.mark_fresh(keys)
    current = {key for key, ent in st.cache.items() if ent[0] == st._version(ent[2])}
    assert current == set(keys[:2])
    assert MS.assert_copies_current(net) == 2


def test_staged_adamw_table_follows_gen(staged):
    st, ps, k, net = staged
    params = [(ps["a"], 0), (ps["b"], 24), (ps["c"], 54)]
    t1 = st.adamw_table("span", params, PA_BF16)
    assert k.calls["make_adamw_stage_table"] == 1 and len(t1[3]) == 6
    assert st.adamw_table("span", params, PA_BF16)[0] is t1[0] and k.calls["make_adamw_stage_table"] == 1
    # entries: (offset, rows, cols, copy, transposed copy) in buffer order
    assert [(e[0], e[1], e[2]) for e in t1[0]] == [(0, 4, 6), (24, 3, 10), (54, 8, 4)]
    assert all(e[3] is st.cache[(id(p), PA_BF16, False)][1] and e[4] is st.cache[(id(p), PA_BF16, True)][1]
               for e, (p, _) in zip(t1[0], params))
    ps["a"].data = ps["a"].detach().clone()                  # new storage -> new copy -> gen moves -> the table is rebuilt
    new = st.get(ps["a"], PA_BF16, False)
    t2 = st.adamw_table("span", params, PA_BF16)
    assert k.calls["make_adamw_stage_table"] == 2 and t2[0][0][3] is new
    # another dtype: no copies known, every parameter one plain run
    t3 = st.adamw_table("span", params, PA_F32)
    assert t3[3] == [] and [(e[1], e[3], e[4]) for e in t3[0]] == [(1, None, None)] * 3


def test_deepcopy_of_a_model_has_an_empty_cache():
    """what the cold twin rests on: runtime state is not copied, values, mode, precision and requires_grad are"""
    import warnings
    import passt_amd
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 100), stride=10, num_classes=5, embed_dim=64, depth=1, num_heads=1, distilled=True)
    net.precision = "bf16"
    net.eval()
    net.blocks[0].requires_grad_(False)
    p = net.blocks[0].mlp.fc1.weight
    net._staged.cache[(id(p), PA_BF16, False)] = [net._staged._version(p), p.detach().to(torch.bfloat16), p]
    net.mark_params_updated()
    twin = MS.cold_twin(net)
    assert twin._staged is not net._staged and twin._staged.epoch == 0 and net._staged.epoch == 1
    assert not twin.training and twin.precision == "bf16" and not twin.blocks[0].mlp.fc1.weight.requires_grad
    assert copy.deepcopy(twin)._staged.cache == {}

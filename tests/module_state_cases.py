"""What the module-state tests share (tests/test_module_state_cpu.py, tests/test_gpu_module_state.py): the routes by which a caller
changes weights behind a passt_amd.PaSST, as data, and the two checks that decide bit for bit whether the staged weight copies
(passt_amd.passt._Staged) followed.  Importable without a GPU.

A copy counts as current while ``(p._version, p.data_ptr(), epoch)`` is what it was when the copy was written.  A route is therefore
seen by the cache when torch bumps the version counter or gives the parameter another storage; the routes that do neither
(``needs_mark``) are the contract of ``net.mark_params_updated()``.  ``bumps`` / ``moves`` are what torch is expected to do to the
parameter ``one_weight(module)``; tests/test_module_state_cpu.py pins them on a CPU nn.Linear, so a torch upgrade that changes what
the cache key rests on fails there first.

No reference and no tolerance: ``assert_copies_current`` compares every copy marked current with the cast (transposed cast) of its
parameter, and ``assert_twin_equal`` runs the same call on the module and on a deepcopy of it -- same values, empty cache -- under
the same seeds and compares everything with torch.equal.
"""
import collections
import copy
import warnings

import numpy as np
import torch
import torch.nn as nn

Route = collections.namedtuple("Route", "name mutate needs_mark bumps moves")


def one_weight(module):
    """the single weight the one-parameter routes write: a GEMM weight with both kinds of copies"""
    return module.blocks[0].mlp.fc1.weight if hasattr(module, "blocks") else module.weight


def _with_grad(module):
    ps = [p for p in module.parameters() if p.grad is not None]
    assert ps, "the optimizer routes follow a backward"
    return ps


def _like(p, rng, scale=0.05):
    """deterministic values on p's device, drawn on the CPU"""
    return (torch.randn(p.shape, generator=rng) * scale).to(p.device)


def _sgd(m, rng):
    torch.optim.SGD(_with_grad(m), lr=0.05).step()


def _adamw_foreach(m, rng):
    torch.optim.AdamW(_with_grad(m), lr=1e-2, weight_decay=1e-2, foreach=True).step()


def _adamw_fused(m, rng):
    torch.optim.AdamW(_with_grad(m), lr=1e-2, weight_decay=1e-2, fused=True).step()


def _load_state_dict(m, rng):
    m.load_state_dict({k: v + _like(v, rng) if v.is_floating_point() else v for k, v in m.state_dict().items()})


def _no_grad_mul(m, rng):
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.03125)


def _no_grad_copy(m, rng):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.detach() + _like(p, rng))


def _detach_add(m, rng):
    for p in m.parameters():
        p.detach().add_(_like(p, rng))


def _init_one(m, rng):
    torch.manual_seed(int(torch.randint(1 << 30, (1,), generator=rng)))
    nn.init.trunc_normal_(one_weight(m), std=0.05)


def _data_assign(m, rng):
    for p in m.parameters():
        p.data = p.detach() + _like(p, rng)


def _data_mul(m, rng):
    for p in m.parameters():
        p.data.mul_(1.03125)


def _data_copy(m, rng):
    for p in m.parameters():
        p.data.copy_(p.detach() + _like(p, rng))


ROUTES = [
    #     name              mutate          needs_mark  bumps  moves
    Route("sgd",            _sgd,            False,     True,  False),
    Route("adamw_foreach",  _adamw_foreach,  False,     True,  False),
    # torch._fused_adamw_ writes the parameters without touching their version counters: seen through the optimizer step hook
    # passt_amd.passt installs, not through the cache key
    Route("adamw_fused",    _adamw_fused,    False,     False, False),
    Route("load_state_dict", _load_state_dict, False,   True,  False),
    Route("no_grad_mul",    _no_grad_mul,    False,     True,  False),
    Route("no_grad_copy",   _no_grad_copy,   False,     True,  False),
    Route("detach_add",     _detach_add,     False,     True,  False),
    Route("init_trunc_normal", _init_one,    False,     True,  False),
    Route("data_assign",    _data_assign,    False,     False, True),
    Route("data_mul",       _data_mul,       True,      False, False),
    Route("data_copy",      _data_copy,      True,      False, False),
]
ROUTE_IDS = [r.name for r in ROUTES]


def fused_accepted(device):
    """does this torch take AdamW(fused=True) for parameters on ``device``?"""
    try:
        torch.optim.AdamW([torch.zeros(2, device=device, requires_grad=True)], fused=True)
        return True
    except (RuntimeError, ValueError):
        return False


# ---- the two checkers -----------------------------------------------------------------------------------------------------------------
def assert_copies_current(net):
    """Every staged copy that is marked current equals the cast (transposed cast) of its parameter, bit for bit.  Returns how many
    entries that were: callers assert a count, so that an empty or all-stale cache cannot pass."""
    st = net._staged
    names = {id(p): n for n, p in net.named_parameters()}
    n = 0
    for (pid, dt, transposed), (ver, out, p) in st.cache.items():
        if ver != st._version(p):
            continue
        w = p.detach().reshape(p.shape[0], -1)
        want = (w.t().contiguous() if transposed else w).to(out.dtype)
        assert torch.equal(out, want), f"staged copy of {names.get(pid, '<a replaced parameter>')} (transposed={transposed}, " \
            f"{out.dtype}) is marked current but differs from its parameter: max |diff| " \
            f"{float((out.float() - want.float()).abs().max()):.3e}"
        n += 1
    return n


def cold_twin(net):
    """A deepcopy: same values, same mode and precision, nothing staged."""
    twin = copy.deepcopy(net)
    assert twin.training == net.training and twin.precision == net.precision
    a, b = net.state_dict(), twin.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].data_ptr() != b[k].data_ptr(), k
    assert [p.requires_grad for p in net.parameters()] == [p.requires_grad for p in twin.parameters()]
    assert not twin._staged.cache
    return twin


def _flatten(tree, prefix=""):
    if torch.is_tensor(tree) or tree is None:
        yield prefix, tree
    elif isinstance(tree, dict):
        for k, v in tree.items():
            yield from _flatten(v, f"{prefix}.{k}")
    else:
        for i, v in enumerate(tree):
            yield from _flatten(v, f"{prefix}[{i}]")


def assert_trees_equal(got, want, what=""):
    """two nests of tensors (dicts / lists / None): same structure, same shapes, torch.equal leaves"""
    g, w = list(_flatten(got)), list(_flatten(want))
    assert [k for k, _ in g] == [k for k, _ in w], (what, [k for k, _ in g], [k for k, _ in w])
    for (k, a), (_, b) in zip(g, w):
        assert (a is None) == (b is None), (what, k)
        if a is None:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        assert torch.equal(a, b), f"{what}{k}: differs, max |diff| {float((a.double() - b.double()).abs().max()):.3e} " \
                                  f"of max |value| {float(b.double().abs().max()):.3e}"


def assert_twin_equal(net, call, seed=0, twin=None, what=""):
    """``call(module)`` -> a nest of tensors, run on ``net`` and on a cold twin of it under the same torch / numpy seeds: bit-equal.
    Returns the twin (warm now) for further calls."""
    twin = cold_twin(net) if twin is None else twin
    outs = []
    for m in (net, twin):
        torch.manual_seed(seed)
        np.random.seed(seed)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            outs.append(call(m))
    assert_trees_equal(outs[0], outs[1], what)
    return twin


# ---- the model and its calls ----------------------------------------------------------------------------------------------------------
def small_case(seed=12, **over):
    from tests.golden import make_golden as G
    return dict(G.CASES["model_small_train"], seed=seed, **over)


def build_small(precision, seed=12, device="cuda", **cfg):
    """The SMALL network of tests/golden/make_golden.py with model_small_train's Patchout (structured and unstructured), deterministic
    weights; ``cfg``: further constructor arguments (drop_path_rate)."""
    import passt_amd
    from oracle import detgen
    c = small_case(seed)["cfg"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = passt_amd.PaSST(u_patchout=c["u_patchout"], s_patchout_t=c["s_patchout_t"], s_patchout_f=c["s_patchout_f"],
                            img_size=c["img_size"], patch_size=c["patch"], stride=c["stride"], num_classes=c["num_classes"],
                            embed_dim=c["embed_dim"], depth=c["depth"], num_heads=c["num_heads"], distilled=True, **cfg)
    sd = detgen.passt_state_dict(c, seed)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
    m.precision = precision
    return m.to(device)


def batch(seed, B=3, T=250, device="cuda", num_classes=None):
    """model_small_train's odd batch (B=3, T=250) on another seed, or another shape"""
    from oracle import detgen
    from tests.golden import make_golden as G
    x, y = G.model_inputs(small_case(seed, B=B, T=T))
    if num_classes is not None:
        y = (detgen.uniform(seed, "y", (B, num_classes), 0.0, 1.0) < 0.1).astype(np.float32)
    return torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)


def loss_of(logits, feat, y):
    """BCE on the logits plus a term on the features, so that both output gradients are live"""
    return torch.nn.functional.binary_cross_entropy_with_logits(logits, y, reduction="none").mean() + 0.1 * feat.square().mean()


def train_call(x, y, want_dx=False):
    """forward, loss, backward from cleared gradients -> logits, features, every parameter gradient, the input gradient"""
    def call(m):
        for p in m.parameters():
            p.grad = None
        xx = x.clone().requires_grad_(want_dx)
        logits, feat = m(xx)
        loss_of(logits, feat, y).backward()
        return dict(logits=logits.detach(), feat=feat.detach(), dx=xx.grad,
                    grads={n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()})
    return call


def eval_call(x, **kw):
    """a no_grad forward (``kw``: lengths=, attn=, ...) -> everything it returns"""
    def call(m):
        with torch.no_grad():
            return list(m(x, **kw))
    return call

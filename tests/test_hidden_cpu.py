"""``net(x, hidden=...)`` without a GPU: argument validation, the launch sequence (tests/test_sequence_cpu.py's recorder), the ABI.

Every test here fails on the parent commit with a TypeError on the ``hidden=`` keyword (the ABI test: on the missing symbols)."""
import os
import re
import warnings

import pytest
import torch

import passt_amd
from passt_amd import _lib
from passt_amd import passt as P
from tests import test_sequence_cpu as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(depth=2, train=False, frozen=False, precision="bf16", **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, depth=depth, num_heads=2, distilled=True, **kw)
    net.train(train).requires_grad_(not frozen)
    net.precision, net.input_grad, net.varlen_grad = precision, True, True
    return net


_record = S._record_run         # trace of ``run(rec)`` with every op replaced by the recorder's stand-in


def _names(trace):
    return [e[0] for e in trace]


# ----------------------------------------------------------------------------------------------
# validation
# ----------------------------------------------------------------------------------------------
BAD = [3, "norm", (), [], (0, 0), (1, -1), ("norm", "norm"), (2,), (-3,), (True,), (0.5,), ("last",), (None,), {0}]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
def test_bad_hidden_raises_before_any_launch_or_draw(bad, lengths):
    def run(rec):
        net = _net(train=lengths is None, s_patchout_t=6, s_patchout_f=3)
        state = torch.get_rng_state()
        with pytest.raises(ValueError, match="hidden"):
            net(torch.zeros(S.X_SHAPE), hidden=bad) if lengths is None else net(torch.zeros(S.X_SHAPE), lengths=lengths, hidden=bad)
        assert torch.equal(torch.get_rng_state(), state)            # no Patchout draw was consumed
    assert _record(run) == []                                       # nothing was launched


def test_parse_hidden_resolves_negative_indices_in_order():
    assert P.parse_hidden((3, 7, -1, "norm"), 12) == (3, 7, 11, "norm")
    assert P.parse_hidden(["norm", -12], 12) == ("norm", 0)


def test_ensemble_rejects_hidden():
    ens = passt_amd.passt.EnsembelerModel([_net(), _net()])
    with pytest.raises(ValueError, match="hidden"):
        ens(torch.zeros(S.X_SHAPE), hidden=(0,))


def test_forward_is_still_one_opaque_call_for_the_compiler():
    assert getattr(passt_amd.PaSST.forward, "_torchdynamo_disable", False)
    import inspect
    p = inspect.signature(passt_amd.PaSST.forward).parameters
    assert p["hidden"].default is None and "hidden" in (passt_amd.PaSST.forward.__doc__ or "")


# ----------------------------------------------------------------------------------------------
# forward sequence
# ----------------------------------------------------------------------------------------------
def _fwd(net, hidden, lengths=None, out=None):
    def run(rec):
        with torch.no_grad():
            kw = {} if hidden is None else dict(hidden=hidden)
            res = net(torch.zeros(S.X_SHAPE), **kw) if lengths is None else net(torch.zeros(S.X_SHAPE), lengths=lengths, **kw)
        if out is not None:
            out.append(res)
    return run


@pytest.mark.parametrize("lengths,train", [(None, False), (None, True), (S.LENGTHS, False)])       # no training on ragged batches
def test_intermediate_layers_launch_exactly_the_default_forward(lengths, train):
    kw = dict(s_patchout_t=6, s_patchout_f=3) if train else {}
    res = []
    base = _record(_fwd(_net(3, train, **kw), None, lengths))
    got = _record(_fwd(_net(3, train, **kw), (1, 0), lengths, res))
    assert len(base) > 20 and got == base                  # same ops, same arguments, same order (and the same Patchout draws)
    out = res[0]
    if lengths is None:
        logits, feat, hs = out
        assert isinstance(hs, list) and len(hs) == 2 and all(h.dim() == 3 and h.shape[0] == S.X_SHAPE[0] and h.shape[2] == 128 for h in hs)
    else:
        logits, feat, hs, tok = out
        assert tok.dtype == torch.int64 and tok.device.type == "cpu" and tok.shape == (len(lengths) + 1,) and tok[0] == 0
        assert all(h.shape == (int(tok[-1]), 128) for h in hs)
        g = P.varlen_geometry(lengths, 16, 10, 12, 25)
        assert tok.tolist() == g["cu_tok"].tolist()


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
@pytest.mark.parametrize("hidden", [(-1,), ("norm",), (0, "norm", 1)])
def test_last_block_request_runs_the_full_tail(lengths, hidden):
    base = _record(_fwd(_net(), None, lengths))
    got = _record(_fwd(_net(), hidden, lengths))
    attn = "attention_fwd" if lengths is None else "attention_fwd_varlen"
    b_attn, g_attn = [e for e in base if e[0] == attn], [e for e in got if e[0] == attn]
    assert [e[2].get("nq") for e in b_attn] == [None, 2] and [e[2].get("nq") for e in g_attn] == [None, None]
    bn, gn = _names(base), _names(got)
    assert bn.count("gather_rows") == gn.count("gather_rows") == 1
    # prefix tail: the residual rows are gathered right behind the 2-query attention; full tail: the head gathers its rows at the end
    assert bn[bn.index("gather_rows") - 1] == attn and gn[gn.index("gather_rows") + 1] in ("layernorm_fwd", "head_pre_fwd")
    extra_ln = 1 if "norm" in hidden else 0
    assert gn.count("layernorm_fwd") == bn.count("layernorm_fwd") + extra_ln
    if extra_ln:
        e = got[gn.index("head_pre_fwd") - 1]
        assert e[0] == "layernorm_fwd" and e[1][4] == _lib.PA_F32          # the final norm of every row, in f32
    # everything else is launched as before, in the same order
    rest = [n for n in gn if n != "gather_rows"]
    if extra_ln:
        rest.pop(len(rest) - 1 - rest[::-1].index("layernorm_fwd"))
    assert rest == [n for n in bn if n != "gather_rows"]


# ----------------------------------------------------------------------------------------------
# backward sequence
# ----------------------------------------------------------------------------------------------
def _step(net, hidden, use, lengths=None, pooled=True):
    """forward + backward of a loss on logits / features (``pooled``) and on the token outputs whose position is in ``use``"""
    def run(rec):
        x = torch.zeros(S.X_SHAPE, requires_grad=True)
        kw = {} if hidden is None else dict(hidden=hidden)
        out = net(x, **kw) if lengths is None else net(x, lengths=lengths, **kw)
        loss = out[0].sum() + out[1].sum() if pooled else 0
        for j in use:
            loss = loss + out[2][j].sum()
        loss.backward()
        rec.log("returned", (x.grad, [n for n, p in net.named_parameters() if p.grad is not None]))
    return run


LN_BWD = ("layernorm_bwd", "layernorm_bwd2")


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
@pytest.mark.parametrize("frozen", [False, True])
def test_two_addend_layernorm_only_where_a_gradient_arrived(lengths, frozen):
    base = _record(_step(_net(3, frozen=frozen), None, (), lengths))
    # requested, not used by the loss: the backward is the default one, launch for launch
    assert _record(_step(_net(3, frozen=frozen), (1, 0), (), lengths)) == base
    # LayerNorm backwards run norm2, norm1 of block 2, then block 1, then block 0: block k's output gradient is formed by norm1 of k + 1
    def ln(trace):
        return [e[0] for e in trace if e[0] in LN_BWD]
    assert ln(base) == ["layernorm_bwd"] * 6
    only1 = _record(_step(_net(3, frozen=frozen), (1, 0), (0,), lengths))
    assert ln(only1) == ["layernorm_bwd", "layernorm_bwd2"] + ["layernorm_bwd"] * 4
    both = _record(_step(_net(3, frozen=frozen), (1, 0), (0, 1), lengths))
    assert ln(both) == ["layernorm_bwd", "layernorm_bwd2", "layernorm_bwd", "layernorm_bwd2", "layernorm_bwd", "layernorm_bwd"]
    # nothing else changes: the other launches are the default backward's, with the same arguments
    for got in (only1, both):
        assert len(got) == len(base)
        for g, b in zip(got, base):
            if g[0] == "layernorm_bwd2":
                assert b[0] == "layernorm_bwd" and g[1][:6] == b[1][:6] and g[1][7:] == b[1][6:] and g[2] == b[2]
            else:
                assert g == b
    # a loss on token outputs only still runs (logits and features arrive as None)
    alone = _record(_step(_net(3, frozen=frozen), (1, 0), (0,), lengths, pooled=False))
    assert ln(alone) == ln(only1)
    if frozen:
        assert not any(n.startswith("wgrad") or n.startswith("colsum") for n in _names(both))


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
@pytest.mark.parametrize("frozen", [False, True])
def test_full_tail_backward_injects_in_one_kernel(lengths, frozen):
    base = _record(_step(_net(frozen=frozen), None, (), lengths))
    assert "scatter_rows_into_zeros" in _names(base) and "tail_inject" not in _names(base)
    for use, adds in (((), (None, None)), ((0,), ("f32", None)), ((1,), (None, "f32")), ((0, 1), ("f32", "f32"))):
        got = _record(_step(_net(frozen=frozen), (-1, "norm"), use, lengths))
        names = _names(got)
        assert "scatter_rows_into_zeros" not in names and names.count("tail_inject") == 1 and "layernorm_bwd2" not in names
        e = got[names.index("tail_inject")]
        assert [None if a is None else a[:3] for a in e[1][3:5]] == list(adds)
        attn = [x for x in got if x[0] in ("attention_bwd", "attention_bwd_varlen")]
        assert all(x[2].get("nq") is None for x in attn) and len(attn) == 2
        n_ln = [x for x in got if x[0] == "layernorm_bwd"]
        assert len(n_ln) == 4 + (1 in use)
        if 1 in use:                                       # the final norm over all rows, in front of the head's report and the tail kernel
            first = n_ln[0]
            assert names.index("layernorm_bwd") < names.index("tail_inject") and first[1][0].startswith("f32")
            if frozen:
                assert first[2].get("defer") is not None and not first[2].get("accumulate")
            else:
                assert first[2].get("accumulate") is True      # on top of what the head's own rows gave norm.weight / norm.bias
        if frozen:
            assert not any(n.startswith("wgrad") or n.startswith("colsum") for n in names)


# ----------------------------------------------------------------------------------------------
# ABI
# ----------------------------------------------------------------------------------------------
NEW = ("pa_layernorm_bwd2", "pa_layernorm_bwd2_partial", "pa_tail_inject")


def test_new_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "passt_amd.h")) as f:
        src = f.read()
    assert re.search(r"#define PA_ABI_VERSION 6\b", src)
    for n in NEW:
        assert re.search(r"\bint " + n + r"\s*\(", src), n
        assert n in _lib.SIGNATURES
    # the old entries keep their signatures
    assert len(_lib.SIGNATURES["pa_layernorm_bwd"][1]) == 17 and len(_lib.SIGNATURES["pa_layernorm_bwd_partial"][1]) == 13
    assert len(_lib.SIGNATURES["pa_layernorm_bwd2"][1]) == 18 and len(_lib.SIGNATURES["pa_layernorm_bwd2_partial"][1]) == 14
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.pa_abi_version() == 6
    for n in NEW:
        assert getattr(lib, n) is not None
    # host-side argument checks answer without a GPU
    assert lib.pa_tail_inject(None, None, 0, None, None, None, None, 0, 4, 8, None) != 0          # no output
    assert lib.pa_layernorm_bwd2_partial(None, 0, None, None, None, None, None, None, None, None, None, 4, 8, None) != 0

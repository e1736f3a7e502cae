"""``net(x, attn=..., attn_grad=...)`` without a GPU: the parser and the errors, the argument checks of pa_attention_probs_grad (they
return before any device access), the launch sequence (tests/test_sequence_cpu.py's recorder) and the fixture
tests/golden/attn_grad.npz.

Every test here but the two "default traces" ones fails on the parent commit: a missing function, a missing symbol, a missing file or a
TypeError on ``attn_grad=``."""
import ctypes as C
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
from tests.golden import make_attn_grad_golden as GG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
def test_parse_attn_grad():
    assert P.parse_attn_grad(None, None) is None and P.parse_attn_grad(None, (0,)) is None
    assert P.parse_attn_grad(True, (0,)) == "grad" and P.parse_attn_grad("grad", (0,), "each") == "grad"
    assert P.parse_attn_grad("cam", (0,), "each") == "cam" and P.parse_attn_grad("cam", (0,), "mean") == "cam"


BAD = [dict(attn_grad="gradient", attn=(0,)), dict(attn_grad=1, attn=(0,)), dict(attn_grad="Grad", attn=(0,)), dict(attn_grad=("cam",), attn=(0,)),
       dict(attn_grad="grad"), dict(attn_grad="cam"), dict(attn_grad=True),                              # without attn=
       dict(attn_grad="grad", attn=(0,), attn_heads="mean"), dict(attn_grad=True, attn=(0,), attn_heads="mean")]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
@pytest.mark.parametrize("lengths", [None, [250, 100]])
def test_bad_attn_grad_raises_before_any_draw(bad, lengths):
    net = _net(train=lengths is None)
    net.varlen_grad = True
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="attn_grad"):
        net(torch.zeros(X_SHAPE), **bad) if lengths is None else net(torch.zeros(X_SHAPE), lengths=lengths, **bad)
    assert torch.equal(torch.get_rng_state(), state)                # no Patchout draw was consumed, and no device was asked for


def _no_graph_calls():
    def no_grad(net, x):
        with torch.no_grad():
            net(x, attn=(0,), attn_grad="cam")

    def frozen(net, x):
        net.requires_grad_(False)(x, attn=(0,), attn_grad="grad")

    def ragged_without_switch(net, x):
        net.eval()(x, lengths=[250, 100], attn=(0,), attn_grad="grad")

    return [no_grad, frozen, ragged_without_switch]


@pytest.mark.parametrize("call", _no_graph_calls(), ids=lambda f: f.__name__)
def test_a_call_that_records_no_graph_raises_before_any_draw(call):
    net = _net(train=True)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="come out of a backward"):
        call(net, torch.zeros(X_SHAPE))
    assert torch.equal(torch.get_rng_state(), state)


def test_ensemble_rejects_attn_grad():
    ens = passt_amd.passt.EnsembelerModel([_net(), _net()])
    with pytest.raises(ValueError, match="attn_grad"):
        ens(torch.zeros(X_SHAPE), attn=(0,), attn_grad="cam")
    with pytest.raises(ValueError, match="attn_grad"):
        ens(torch.zeros(X_SHAPE), attn_grad="cam")


# ----------------------------------------------------------------------------------------------
# the C entry's argument checks
# ----------------------------------------------------------------------------------------------
def test_pa_attention_probs_grad_checks_its_arguments_before_any_device_access():
    lib = _lib.load()
    assert lib.pa_abi_version() == 6                                 # an addition: the ABI version stays
    host = (C.c_float * 16)()                                        # a non-NULL pointer the entry must never dereference
    p = C.addressof(host)
    EINVAL, EUNSUPPORTED = -1, -2

    def call(qkv=p, ldqkv=384, lse=p, d_o=p, ldo=128, compact=0, out=p, cu=None, off=None, B=1, H=2, N=33, nq=33, mean=0, mode=1,
             dtype=_lib.PA_BF16, flags=1):
        return lib.pa_attention_probs_grad(qkv, ldqkv, lse, d_o, ldo, compact, out, cu, off, B, H, N, nq, mean, mode, 0.125, dtype, flags, None)

    for kw in (dict(qkv=None), dict(out=None), dict(B=0), dict(H=0), dict(N=0), dict(nq=0), dict(B=-1), dict(nq=-2),
               dict(nq=34),                 # fixed layout: more queries than tokens
               dict(flags=2), dict(flags=-1), dict(mean=2), dict(mean=-1), dict(dtype=2), dict(dtype=-1),
               dict(ldqkv=383), dict(ldqkv=0),      # a row shorter than [q | k | v] x H x 64
               dict(cu=p),                  # packed layout without its offsets
               dict(off=p),                 # offsets without the packed layout
               # the entry's own
               dict(d_o=None), dict(mode=2), dict(mode=-1), dict(mode=0, mean=1), dict(lse=None), dict(lse=None, mean=1),
               dict(ldo=127), dict(ldo=0), dict(compact=2), dict(compact=-1)):
        assert call(**kw) == EINVAL, kw
    assert call(ldqkv=388) == EUNSUPPORTED                           # bf16 rows that are not 16-byte aligned
    assert call(ldqkv=386, dtype=_lib.PA_F32) == EUNSUPPORTED
    assert call(ldo=132) == EUNSUPPORTED and call(ldo=130, dtype=_lib.PA_F32) == EUNSUPPORTED


def test_header_declares_the_entry_and_the_binding_lists_it():
    text = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert "int pa_attention_probs_grad(" in text and "#define PA_ABI_VERSION 6" in text
    assert "#define PA_ATTN_PGRAD_GRAD 0" in text and "#define PA_ATTN_PGRAD_CAM 1" in text
    assert (ops.ATTN_PGRAD_GRAD, ops.ATTN_PGRAD_CAM) == (0, 1)
    res, args = _lib.SIGNATURES["pa_attention_probs_grad"]
    assert res is _lib.i32 and len(args) == 19
    assert hasattr(_lib.load(), "pa_attention_probs_grad")
    assert "attention_probs_grad.hip" in open(os.path.join(ROOT, "passt_amd", "csrc", "Makefile")).read()


# ----------------------------------------------------------------------------------------------
# the launch sequence (tests/test_sequence_cpu.py's recorder, with stand-ins for the two new ops)
# ----------------------------------------------------------------------------------------------
def _pgrad(qkv, lse, d_o, B, H, N, scale, nq=None, head_mean=False, mode=0, do_compact=False, flags=0, out=None):
    nq = N if nq is None else nq
    assert d_o.shape == ((B * nq if do_compact else B * N), H * 64) and d_o.dtype == qkv.dtype and flags == ops.ATTN_Q_PRESCALED
    assert (lse is None) if mode == 0 else (lse.numel() == B * H * nq and lse.dtype == torch.float32)
    return torch.zeros(B, 1 if head_mean else H, nq, N)


def _pgrad_varlen(qkv, lse, d_o, cu_tok, out_off, total_out, B, H, max_N, scale, nq=None, head_mean=False, mode=0, do_compact=False, flags=0,
                  out=None):
    assert d_o.shape == ((B * nq if do_compact else qkv.shape[0]), H * 64) and out_off.dtype == torch.int64 and out_off.numel() == B
    assert (lse is None) if mode == 0 else lse.numel() == (H * qkv.shape[0] if nq is None else B * H * nq)
    return torch.zeros(total_out)


def _record(run):
    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(S._RESULTS, "attention_probs_grad", _pgrad)
        mp.setitem(S._RESULTS, "attention_probs_grad_varlen", _pgrad_varlen)
        return S._record_run(run)


def _is_grad_launch(e):
    return e[0].startswith("attention_probs_grad")


KWS = [dict(attn=(0,), attn_grad="grad"), dict(attn=(-1, 0), attn_rows="prefix", attn_grad=True), dict(attn=(-1,), attn_grad="cam"),
       dict(attn=(1, 0), attn_rows="prefix", attn_heads="mean", attn_grad="cam"), dict(attn=(0,), attn_heads="mean", attn_grad="cam")]


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
@pytest.mark.parametrize("kw", KWS, ids=[repr(k) for k in KWS])
def test_gradients_add_one_launch_behind_each_attention_backward_and_nothing_else(lengths, kw):
    """Forward + backward through the autograd node: with ``attn_grad`` the trace is that of the call with ``attn=`` alone plus one
    map-gradient launch right behind the attention backward of every requested block, on the main stream; .grad is None before
    the backward and has the map's shape and f32 after it."""
    plain_kw = {k: v for k, v in kw.items() if k != "attn_grad"}

    def run(kws):
        def go(rec):
            net = S._net(train=lengths is None)
            net.input_grad = net.varlen_grad = True
            x = torch.zeros(S.X_SHAPE, requires_grad=True)
            out = net(x, **({} if lengths is None else dict(lengths=lengths)), **kws)
            maps = [t for m in out[2] for t in (m if isinstance(m, list) else [m])]
            assert all(t.grad is None and t.grad_fn is None and not t.requires_grad for t in maps)
            (out[0].sum() + out[1].sum()).backward()
            if "attn_grad" in kws:
                assert all(t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == torch.float32 for t in maps)
                if lengths is not None:                             # every clip's gradient is a view of one flat buffer per map
                    for m in out[2]:
                        assert len({t.grad.untyped_storage().data_ptr() for t in m}) == 1
            else:
                assert all(t.grad is None for t in maps)
        return go
    plain, got = _record(run(plain_kw)), _record(run(kw))
    prefix, cam = kw.get("attn_rows") == "prefix", kw["attn_grad"] == "cam"
    # "cam" on prefix rows below a prefix-only tail cuts the lse to those rows with torch ops: no launch of the library
    assert [e for e in got if not _is_grad_launch(e)] == plain
    launches = [i for i, e in enumerate(got) if _is_grad_launch(e)]
    assert len(launches) == len(kw["attn"])
    blocks = sorted((a % 2 for a in kw["attn"]), reverse=True)      # the backward walks the blocks downwards
    bwd = [i for i, e in enumerate(got) if e[0].startswith("attention_bwd")]
    assert len(bwd) == 2
    for i, blk in zip(launches, blocks):
        e = got[i]
        assert e[0] == ("attention_probs_grad" if lengths is None else "attention_probs_grad_varlen") and e[3] == "main"
        assert i - 1 == bwd[1 - blk]                                 # right behind that block's attention backward
        full_tail = blk == 1 and not prefix
        assert e[2]["nq"] == (2 if prefix else None) and e[2]["mode"] == int(cam) and e[2]["head_mean"] == (kw.get("attn_heads") == "mean")
        assert e[2]["do_compact"] == (blk == 1 and not full_tail)    # only the prefix-only tail hands over a compact d_att


@pytest.mark.parametrize("name", ["fixed_attn_prefix_mean", "packed_hidden_attn_grad", "fixed_train_bf16"])
def test_without_attn_grad_the_traces_are_the_recorded_ones(name):
    S.test_launch_sequence_is_the_recorded_one(name)


def test_the_backward_drops_the_request_and_the_saved_activations():
    def go(rec):
        net = S._net(train=True)
        out = net(torch.zeros(S.X_SHAPE), attn=(0,), attn_grad="cam")
        out[0].sum().backward()
        g = out[2][0].grad
        assert g is not None and out[0].grad_fn.c is None and out[0].grad_fn.attn_grad is None      # nothing keeps the activations
    _record(go)


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
@pytest.mark.parametrize("world", [2, 3])
def test_under_an_attached_reducer_the_map_gradients_are_this_ranks_own(lengths, world):
    """An attached reducer makes the node divide dlogits / dfeat by the world size (the mean over ranks); like x.grad the maps'
    gradients are local quantities and are multiplied back.  With a map-gradient stand-in that returns the scale of the d_att it was
    handed (ones here: the recorder's kernels do not compute), every element of every .grad -- every clip of a packed map too -- must
    come out as ``world``: scaled exactly once."""
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
        out = net(torch.zeros(S.X_SHAPE), **({} if lengths is None else dict(lengths=lengths)), attn=(0, -1), attn_rows="prefix",
                  attn_grad="cam")
        (out[0].sum() + out[1].sum()).backward()
        assert red.waited == 1 and red.flat is not None and red.blocks
        maps = [t for m in out[2] for t in (m if isinstance(m, list) else [m])]
        assert len(maps) == (2 if lengths is None else 2 * len(lengths))
        for t in maps:
            assert t.grad.shape == t.shape and bool((t.grad == float(world)).all())

    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(S._RESULTS, "attention_probs_grad", lambda *a, **k: torch.ones_like(_pgrad(*a, **k)))
        mp.setitem(S._RESULTS, "attention_probs_grad_varlen", lambda *a, **k: torch.ones_like(_pgrad_varlen(*a, **k)))
        S._record_run(go)


def test_attn_grad_false_is_no_request():
    def go(rec):
        net = S._net(train=False)
        with torch.no_grad():
            assert len(net(torch.zeros(S.X_SHAPE), attn_grad=False)) == 2 and len(net(torch.zeros(S.X_SHAPE), attn=(0,), attn_grad=False)) == 3
            ens = passt_amd.passt.EnsembelerModel([net])
            assert len(ens(torch.zeros(S.X_SHAPE), attn_grad=False)) == 2
    _record(go)


# ----------------------------------------------------------------------------------------------
# the fixture
# ----------------------------------------------------------------------------------------------
def _expected():
    """{fixture key: shape} of every recorded tensor"""
    out = {}

    def add(prefix, B, H, ntok, blocks):
        for blk in blocks:
            for kind, variants in (("grad", GG.GRAD_VARIANTS), ("cam", tuple(AG.VARIANTS))):
                for v in variants:
                    rows, heads = AG.VARIANTS[v]
                    out[f"{prefix}.{kind}.b{blk}.{v}"] = (B, H, rows, heads, ntok)

    for name, case in AG.CASES.items():
        cfg = case["cfg"]
        add(name, case["B"], cfg["num_heads"], 290 if not case["training"] else None, [a % cfg["depth"] for a in case["attn"]])
    for i, n in enumerate(AG.RAGGED["lengths"]):
        cfg = AG.RAGGED["cfg"]
        add(f"ragged.{i}", 1, cfg["num_heads"], 2 + 12 * ((n - 16) // 10 + 1), [a % cfg["depth"] for a in AG.RAGGED["attn"]])
    return out


def test_fixture_keys_shapes_and_content(golden_dir):
    path = os.path.join(golden_dir, "attn_grad.npz")
    assert os.path.getsize(path) <= 1.25 * os.path.getsize(os.path.join(golden_dir, "attn.npz"))          # attn.npz's scale
    gold = dict(np.load(path))
    maps = dict(np.load(os.path.join(golden_dir, "attn.npz")))
    want_keys = set()
    for k, (B, H, rows, heads, ntok) in _expected().items():
        want_keys |= {k, k + ".stats", k + ".shape"}
        shape = tuple(int(s) for s in gold[k + ".shape"])
        N = shape[-1]
        assert ntok is None or N == ntok, (k, shape)
        nq = 2 if rows == "prefix" else N
        assert shape == ((B, nq, N) if heads == "mean" else (B, H, nq, N)), (k, shape)
        # same geometry as the map of the same name
        assert shape == tuple(int(s) for s in maps[k.replace(".grad.", ".attn.").replace(".cam.", ".attn.") + ".shape"])
        assert gold[k].dtype == np.float32 and gold[k].size == min(int(np.prod(shape)), GG.SAMPLE)
        l2, amax = gold[k + ".stats"]
        assert l2 > 0 and amax > 0 and np.abs(gold[k]).max() <= amax
        if ".cam." in k:
            assert gold[k].min() >= 0
    assert set(gold) == want_keys
    # a gradient has both signs; the last block's has non-zero rows only where the head reads: the cls / dist queries
    assert gold["eval.grad.b0.all.each"].min() < 0 < gold["eval.grad.b0.all.each"].max()
    assert np.isclose(gold["eval.grad.b1.all.each.stats"], gold["eval.grad.b1.prefix.each.stats"], rtol=1e-6).all()
    assert gold["eval.grad.b0.all.each.stats"][0] > 1.001 * gold["eval.grad.b0.prefix.each.stats"][0]          # block 0's is dense


def test_generator_holds_no_reference_text():
    src = open(os.path.join(ROOT, "tests", "golden", "make_attn_grad_golden.py")).read()
    assert "ref_import" in src and "retain_grad()" in src and "softmax(dim" not in src and "class " not in src
    assert GG.CASES is AG.CASES and GG.RAGGED is AG.RAGGED and GG.SAMPLE == AG.SAMPLE


@pytest.mark.skipif(not ref_import.reference_available(), reason="needs the reference checkout")
def test_fixture_regenerates_bit_identically(golden_dir, tmp_path, monkeypatch):
    monkeypatch.setattr(GG, "HERE", str(tmp_path))
    state = torch.get_rng_state()
    GG.main()
    torch.set_rng_state(state)
    a, b = np.load(os.path.join(golden_dir, "attn_grad.npz")), np.load(os.path.join(str(tmp_path), "attn_grad.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k

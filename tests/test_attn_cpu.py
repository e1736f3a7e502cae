"""``net(x, attn=...)`` without a GPU: the parser, the packed-output offsets, the argument checks of pa_attention_probs (they return
before any device access), and the fixture tests/golden/attn.npz.

Every test here fails on the parent commit: a missing function, a missing symbol, a missing file or a TypeError on ``attn=``."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from passt_amd import _lib, ops
from passt_amd import passt as P
from tests.golden import make_attn_golden as AG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_SHAPE = (2, 1, 128, 250)


def _net(depth=2, train=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, depth=depth, num_heads=2, distilled=True,
                              s_patchout_t=6)
    return net.train(train)


# ----------------------------------------------------------------------------------------------
# the parser
# ----------------------------------------------------------------------------------------------
def test_parse_attn_resolves_negative_indices_in_order():
    assert P.parse_attn((3, 7, -1), 12) == ((3, 7, 11), False, False)
    assert P.parse_attn([-12, 5], 12, "prefix", "mean") == ((0, 5), True, True)
    assert P.parse_attn(range(3), 3, attn_heads="mean") == ((0, 1, 2), False, True)
    assert P.parse_attn((np.int64(1),), 2, attn_rows="prefix") == ((1,), True, False)


BAD = [3, "0", (), [], (0, 0), (1, -1), (2,), (-3,), (True,), (0.5,), ("norm",), (None,), {0}]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
@pytest.mark.parametrize("lengths", [None, [250, 100]])
def test_bad_attn_raises_before_any_draw(bad, lengths):
    net = _net(train=lengths is None)
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="attn"):
        net(torch.zeros(X_SHAPE), attn=bad) if lengths is None else net(torch.zeros(X_SHAPE), lengths=lengths, attn=bad)
    assert torch.equal(torch.get_rng_state(), state)                # no Patchout draw was consumed, and no device was asked for


@pytest.mark.parametrize("kw", [dict(attn_rows="cls"), dict(attn_rows=None), dict(attn_heads="sum"), dict(attn_heads=1),
                                dict(attn_rows="Prefix", attn_heads="mean")])
@pytest.mark.parametrize("attn", [None, (0,)])
def test_bad_modes_raise(kw, attn):
    with pytest.raises(ValueError, match="attn_rows|attn_heads"):
        _net()(torch.zeros(X_SHAPE), attn=attn, **kw)


def test_ensemble_rejects_attn():
    ens = passt_amd.passt.EnsembelerModel([_net(), _net()])
    with pytest.raises(ValueError, match="attn"):
        ens(torch.zeros(X_SHAPE), attn=(0,))


# ----------------------------------------------------------------------------------------------
# the packed layout's offsets
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ntok", [[130, 20, 67, 3], [1190], [1, 1, 5], [26, 518, 1190]])
@pytest.mark.parametrize("H_out", [1, 2, 12])
@pytest.mark.parametrize("nq", [None, 2, 64, 5000])
def test_offsets_helper_against_numpy(ntok, H_out, nq):
    off, total = ops.attention_probs_offsets(ntok, H_out, nq)
    assert off.dtype == np.int64 and off.shape == (len(ntok),)
    sizes = [H_out * (n if nq is None else min(nq, n)) * n for n in ntok]            # [H_out][min(nq, N_b)][N_b], dense
    assert total == sum(sizes) and off.tolist() == [sum(sizes[:i]) for i in range(len(ntok))]


def test_offsets_helper_does_not_wrap_at_2_to_31():
    off, total = ops.attention_probs_offsets([40000, 40000], 12)
    assert off.tolist() == [0, 12 * 40000 * 40000] and total == 2 * 12 * 40000 * 40000


@pytest.mark.parametrize("bad", [dict(ntok=[]), dict(ntok=[5, 0]), dict(ntok=[5], H_out=0), dict(ntok=[5], nq=0)])
def test_offsets_helper_rejects(bad):
    with pytest.raises(ValueError):
        ops.attention_probs_offsets(bad["ntok"], bad.get("H_out", 2), bad.get("nq"))


def test_packed_views_cut_the_flat_buffer():
    tok = torch.tensor([0, 5, 8, 20])
    for prefix in (False, True):
        for mean in (False, True):
            off, total = ops.attention_probs_offsets([5, 3, 12], 1 if mean else 2, 2 if prefix else None)
            flat = torch.arange(total, dtype=torch.float32)
            views = P._PackedLayout.attn_views(flat, tok, 2, prefix, mean)
            for v, o, n in zip(views, off.tolist(), [5, 3, 12]):
                nq = 2 if prefix else n
                assert tuple(v.shape) == ((nq, n) if mean else (2, nq, n))
                assert v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and float(v.reshape(-1)[0]) == o
            assert sum(v.numel() for v in views) == total


# ----------------------------------------------------------------------------------------------
# the C entry's argument checks
# ----------------------------------------------------------------------------------------------
def test_pa_attention_probs_checks_its_arguments_before_any_device_access():
    lib = _lib.load()
    assert lib.pa_abi_version() == 6                                 # an addition: the ABI version stays
    host = (C.c_float * 16)()                                        # a non-NULL pointer the entry must never dereference
    p = C.addressof(host)
    EINVAL, EUNSUPPORTED = -1, -2

    def call(qkv=p, ldqkv=384, lse=p, out=p, cu=None, off=None, B=1, H=2, N=33, nq=33, mean=0, dtype=_lib.PA_BF16, flags=1):
        return lib.pa_attention_probs(qkv, ldqkv, lse, out, cu, off, B, H, N, nq, mean, 0.125, dtype, flags, None)

    for kw in (dict(qkv=None), dict(lse=None), dict(out=None), dict(B=0), dict(H=0), dict(N=0), dict(nq=0), dict(B=-1), dict(nq=-2),
               dict(nq=34),                 # fixed layout: more queries than tokens
               dict(flags=2), dict(flags=-1), dict(mean=2), dict(mean=-1), dict(dtype=2), dict(dtype=-1),
               dict(ldqkv=383), dict(ldqkv=0),      # a row shorter than [q | k | v] x H x 64
               dict(cu=p),                  # packed layout without its offsets
               dict(off=p)):                # offsets without the packed layout
        assert call(**kw) == EINVAL, kw
    assert call(ldqkv=388) == EUNSUPPORTED                           # bf16 rows that are not 16-byte aligned
    assert call(ldqkv=386, dtype=_lib.PA_F32) == EUNSUPPORTED


def test_header_declares_the_entry_and_the_binding_lists_it():
    text = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert "int pa_attention_probs(" in text and "#define PA_ABI_VERSION 6" in text
    res, args = _lib.SIGNATURES["pa_attention_probs"]
    assert res is _lib.i32 and len(args) == 15


# ----------------------------------------------------------------------------------------------
# the fixture
# ----------------------------------------------------------------------------------------------
def _expected_maps():
    """{fixture key prefix: (B, H, Ntok)} of every recorded map"""
    out = {}
    for name, case in AG.CASES.items():
        cfg = case["cfg"]
        ntok = 290 if not case["training"] else None                 # eval at 250 frames: 2 + 12 x 24 patches
        for a in case["attn"]:
            out[f"{name}.attn.b{a % cfg['depth']}"] = (case["B"], cfg["num_heads"], ntok)
    for i, n in enumerate(AG.RAGGED["lengths"]):
        for a in AG.RAGGED["attn"]:
            out[f"ragged.{i}.attn.b{a % AG.RAGGED['cfg']['depth']}"] = (1, AG.RAGGED["cfg"]["num_heads"], 2 + 12 * ((n - 16) // 10 + 1))
    return out


def test_fixture_keys_shapes_and_row_sums(golden_dir):
    path = os.path.join(golden_dir, "attn.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(golden_dir, "hidden.npz"))
    gold = dict(np.load(path))
    want_keys = set()
    for name in list(AG.CASES) + [f"ragged.{i}" for i in range(len(AG.RAGGED["lengths"]))]:
        want_keys |= {name + ".logits", name + ".features"}
    for pre, (B, H, ntok) in _expected_maps().items():
        for v, (rows, heads) in AG.VARIANTS.items():
            k = f"{pre}.{v}"
            want_keys |= {k, k + ".stats", k + ".l1", k + ".shape"}
            shape = tuple(int(s) for s in gold[k + ".shape"])
            N = shape[-1]
            assert ntok is None or N == ntok, (k, shape)
            nq = 2 if rows == "prefix" else N
            assert shape == ((B, nq, N) if heads == "mean" else (B, H, nq, N)), (k, shape)
            n = int(np.prod(shape))
            assert gold[k].dtype == np.float32 and gold[k].size == min(n, AG.SAMPLE)
            # a softmax row sums to 1: the map's L1 total is its number of rows (f32 rows: 1e-6 each)
            n_rows = n // N
            assert abs(float(gold[k + ".l1"]) - n_rows) < 2e-6 * n_rows, (k, float(gold[k + ".l1"]), n_rows)
            l2, amax = gold[k + ".stats"]
            assert 0 < amax <= 1.0 + 1e-6 and gold[k].min() >= 0 and gold[k].max() <= amax
            assert n_rows / N - 1e-3 <= l2 ** 2 <= n_rows + 1e-3            # between uniform rows and one-hot rows
    assert set(gold) == want_keys
    # the training case kept Patchout's tokens: fewer than the full grid
    assert int(gold["patchout_train.attn.b0.all.each.shape"][-1]) < 290


def test_generator_holds_no_reference_text_and_variants_cover_the_interface():
    src = open(os.path.join(ROOT, "tests", "golden", "make_attn_golden.py")).read()
    assert "ref_import" in src and "softmax(dim" not in src and "class " not in src
    assert sorted(AG.VARIANTS.values()) == sorted((r, h) for r in ("all", "prefix") for h in ("each", "mean"))


# ----------------------------------------------------------------------------------------------
# the launch sequence (tests/test_sequence_cpu.py's recorder)
# ----------------------------------------------------------------------------------------------
from tests import test_sequence_cpu as S  # noqa: E402


_record = S._record_run


def _without_maps(trace):
    """the trace without the map launches and what only they need (the packed offsets' upload)"""
    return [e for e in trace if not e[0].startswith("attention_probs") and not (e[0] == "upload_small" and e[1][0].startswith("np.int64"))]


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
@pytest.mark.parametrize("kw", [dict(attn=(0,)), dict(attn=(-1, 0), attn_rows="prefix"), dict(attn=(1,), attn_rows="prefix", attn_heads="mean"),
                                dict(attn=(0,), attn_heads="mean")])
def test_maps_add_their_launch_behind_the_attention_and_nothing_else(lengths, kw):
    """Forward + backward through the autograd node (train mode with Patchout on the fixed path, eval on the packed one): with maps
    asked for -- not all rows of the last block -- the trace is the plain call's plus one map launch right behind each block's
    attention; the maps carry no grad_fn and come back in the documented place."""
    def run(with_maps):
        def go(rec):
            net = S._net(train=lengths is None)
            net.input_grad = net.varlen_grad = True
            x = torch.zeros(S.X_SHAPE, requires_grad=True)
            args = {} if lengths is None else dict(lengths=lengths)
            out = net(x, **args, **(kw if with_maps else {}))
            if with_maps:
                assert len(out) == (3 if lengths is None else 4) and len(out[2]) == len(kw["attn"])
                prefix, mean = kw.get("attn_rows") == "prefix", kw.get("attn_heads") == "mean"
                for m in out[2]:
                    if lengths is None:
                        assert m.grad_fn is None and m.dim() == (3 if mean else 4) and m.shape[-2] == (2 if prefix else m.shape[-1])
                    else:
                        ntok = (out[3][1:] - out[3][:-1]).tolist()
                        assert [tuple(t.shape[-2:]) for t in m] == [(2 if prefix else n, n) for n in ntok]
                        assert all(t.grad_fn is None and t.dim() == (2 if mean else 3) for t in m)
            (out[0].sum() + out[1].sum()).backward()
            assert x.grad is not None
        return go
    plain, maps = _record(run(False)), _record(run(True))
    assert _without_maps(maps) == plain
    names = [e[0] for e in maps]
    launches = [i for i, n in enumerate(names) if n.startswith("attention_probs")]
    assert len(launches) == len(kw["attn"])
    for i in launches:
        assert names[i] == ("attention_probs" if lengths is None else "attention_probs_varlen")
        assert any(n.startswith("attention_fwd") for n in names[max(0, i - 4):i]) and maps[i][3] == "main"


@pytest.mark.parametrize("lengths", [None, S.LENGTHS])
def test_all_rows_of_the_last_block_run_the_full_tail_like_hidden(lengths):
    """attn=(-1,) with every row: the same launches as hidden=(-1,) plus the map's."""
    def run(kw):
        def go(rec):
            net = S._net(train=False)
            args = {} if lengths is None else dict(lengths=lengths)
            with torch.no_grad():
                out = net(torch.zeros(S.X_SHAPE), **args, **kw)
            assert len(out) == (3 if lengths is None else 4)
        return go
    assert _without_maps(_record(run(dict(attn=(-1,))))) == _without_maps(_record(run(dict(hidden=(-1,)))))


def test_hidden_and_attn_together_return_in_the_documented_order():
    def go(rec):
        net = S._net(train=False)
        with torch.no_grad():
            lo, fe, hs, maps = net(torch.zeros(S.X_SHAPE), hidden=(0, "norm"), attn=(1, 0), attn_heads="mean")
            assert len(hs) == 2 and hs[0].shape == (2, 290, 128) and [tuple(m.shape) for m in maps] == [(2, 290, 290)] * 2
            lo, fe, hs, maps, tok = net(torch.zeros(S.X_SHAPE), lengths=S.LENGTHS, hidden=(0,), attn=(0,), attn_rows="prefix")
            assert hs[0].dim() == 2 and isinstance(maps[0], list) and maps[0][0].shape[-2] == 2 and tok.dtype == torch.int64
    _record(go)

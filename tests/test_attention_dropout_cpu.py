"""Attention dropout without a device: the mask rule (known answers of Philox4x32-10, the host entry pa_attention_dropout_mask against
the numpy restatement of tests/attention_dropout_cases.py), the suite's own conditions (kept fraction of the masks the GPU tests use),
the checkers against plain torch with the specified arithmetic and against eight fault models, the argument checks of the two device
entries, and the Python level (rates, refusals, what a forward launches and draws) in the recorder harness of tests/test_sequence_cpu.py.

Every test fails on the parent commit at a missing symbol (pa_attention_*dropout*), attribute (attn_drop_rates, attn_drop_mask) or
argument (attn_drop_seed)."""
import ctypes
import gc
import math
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from passt_amd import _lib, ops
from passt_amd import passt as P
from tests import attention_cases as A
from tests import attention_dropout_cases as DR
from tests import test_sequence_cpu as S
from tests.attention_cases import AC, PA_BF16, PA_F32, PRE
from tests.attention_dropout_cases import DC, TorchDropAttention

EDGE = (1, 3, 4, 5, 31, 33, 65, 513)


@pytest.fixture(autouse=True)
def _collect_models():
    """The models of these tests end in reference cycles (autograd nodes, tracebacks of the refusals): collect them here, so that no
    later test sees a live PaSST disappear under its hands (passt._LIVE is a weak set)."""
    yield
    gc.collect()


# ---- the rule ------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, want in DR.KNOWN_ANSWERS:
        assert tuple(int(x) for x in DR.philox4x32_10(*ctr, *key)) == want


@pytest.mark.parametrize("N", EDGE)
def test_host_mask_equals_the_restatement(N):
    """shapes that cross every patch (4 x 4) and tile (32 / 64 / 128) edge; BH = 1 is the first head of BH = 7"""
    for nq in (q for q in EDGE if q <= N):
        for site in (0, 3):
            by = DR.rule_bytes(DR.SEED, site, 7, nq, N)
            for t in (1, 26, 128, 255):
                want = torch.from_numpy(by >= t)
                for BH in (1, 7):
                    got = ops.attn_drop_mask(DR.SEED, site, 1, BH, nq, N, t / 256.0)
                    assert got.dtype == torch.bool and tuple(got.shape) == (1, BH, nq, N)
                    assert torch.equal(got[0], want[:BH]), (N, nq, site, t, BH)


def test_host_mask_refusals_and_rate_quantisation():
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 64)()
    assert lib.pa_attention_dropout_mask(1, 2, 0, 1, 4, 4, 128, buf) == 0
    for args in ((1, 2, 0, 0, 4, 4, 128, buf), (1, 2, 0, 1, 5, 4, 128, buf), (1, 2, 0, 1, 0, 4, 128, buf), (1, 2, 0, 1, 4, 4, 0, buf),
                 (1, 2, 0, 1, 4, 4, 256, buf), (1, 2, 0, 1, 4, 4, 128, None)):
        assert lib.pa_attention_dropout_mask(*args) == A.PA_EINVAL, args
    assert [ops.attn_drop_t(p) for p in (0.0, 0.001, 0.002, 0.1, 0.25, 0.5, 0.997)] == [0, 0, 1, 26, 64, 128, 255]
    for bad in (0.999, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            ops.attn_drop_t(bad)
    assert bool(ops.attn_drop_mask(DR.SEED, 0, 1, 2, 3, 5, 0.0).all())             # t == 0: nothing is drawn, everything kept
    # a (2,) tensor with int32 storage is read as two uint32 words
    s = torch.tensor([DR.SEED[0] - 2 ** 32 if DR.SEED[0] >= 2 ** 31 else DR.SEED[0], DR.SEED[1] - 2 ** 32 if DR.SEED[1] >= 2 ** 31 else DR.SEED[1]],
                     dtype=torch.int32)
    assert torch.equal(ops.attn_drop_mask(s, 1, 1, 2, 9, 9, 0.5), ops.attn_drop_mask(DR.SEED, 1, 1, 2, 9, 9, 0.5))


def test_masks_differ_with_every_coordinate():
    base = DR.rule_bytes(DR.SEED, 2, 4, 64, 64)
    assert not np.array_equal(base, DR.rule_bytes((DR.SEED[0] ^ 1, DR.SEED[1]), 2, 4, 64, 64))     # seed word 0
    assert not np.array_equal(base, DR.rule_bytes((DR.SEED[0], DR.SEED[1] ^ 1), 2, 4, 64, 64))     # seed word 1
    assert not np.array_equal(base, DR.rule_bytes(DR.SEED, 3, 4, 64, 64))                           # site
    for s in range(3):
        assert not np.array_equal(base[s], base[s + 1])                                             # s
    for i in range(63):
        assert not np.array_equal(base[:, i], base[:, i + 1])                                       # q (inside a patch and across)
        assert not np.array_equal(base[:, :, i], base[:, :, i + 1])                                 # k
    # one call covers a 4 x 4 patch: its 16 bytes are the 16 bytes of the four words
    R = DR.philox4x32_10(3, 5, 1, 2, *DR.SEED)
    patch = base[1, 20:24, 12:16]
    for w in range(4):
        for j in range(4):
            assert int(patch[w, j]) == (int(R[w]) >> (8 * j)) & 0xff


def test_kept_fraction_of_the_suites_masks():
    """A condition on the chosen seed: over every mask the GPU tests use, the kept fraction lies within 5 sigma of keep."""
    from tests.test_gpu_attention_dropout import READ_N, READ_T            # constants only: importing launches nothing
    shapes = {(d.site, d.c.B * d.c.H, d.c.nqk, d.c.N, d.t) for N in DR.N_FWD_BWD for d in DR.fwd_bwd_cases(N)}
    shapes |= {((N + t) % 7, BH, N, N, t) for N in READ_N for BH in (1, 6) for t in READ_T}
    shapes |= {(11, 6, 1190, 1190, t) for t in (26, 128)}
    kept, total = {}, {}
    for site, BH, nq, N, t in sorted(shapes):
        m = DR.rule_bytes(DR.SEED, site, BH, nq, N) >= t
        kept[t] = kept.get(t, 0) + int(m.sum())
        total[t] = total.get(t, 0) + m.size
    assert set(kept) == {1, 26, 64, 128, 255}
    for t, n in total.items():
        keep = DR.keep_of(t)
        assert abs(kept[t] / n - keep) <= 5 * math.sqrt(keep * (1 - keep) / n), (t, kept[t] / n, keep, n)


# ---- the checkers: the specified arithmetic passes, the fault models do not --------------------------------------------------------
@pytest.mark.parametrize("N", DR.N_FWD_BWD)
def test_torch_passes_every_case(N):
    worst = {}

    def rec(group, ratio):
        worst[group] = max(worst.get(group, 0.0), ratio)
    for d in DR.fwd_bwd_cases(N):
        DR.check_dropout(TorchDropAttention(), d, rec)
    assert worst and max(worst.values()) <= 1.0


def test_exact_regime_is_where_one_over_keep_is_a_power_of_two():
    assert [t for t in range(1, 256) if DR.exact_regime(t)] == [128, 192, 224, 240, 248, 252, 254, 255]
    assert not DR.exact_regime(64) and DR.keep_of(64) == 0.75
    for t in (128, 192):                   # a second exact threshold: the exact families, bit for bit in bf16
        for fam in ("select", "pair", "uniform"):
            DR.check_dropout(TorchDropAttention(), DC(AC(PA_BF16, 1, 3, 65, fam, PRE), t, site=1))


def _mask(d, b, site=None, **kw):
    c = d.c
    m = torch.from_numpy(DR.rule_bytes(d.seed, d.site if site is None else site, c.B * c.H, c.nqk, c.N, **kw) >= d.t)
    return m[b * c.H:(b + 1) * c.H]


class QueryAndKeyExchanged(TorchDropAttention):
    """the rule evaluated at (k, q)"""
    def mask(self, d, b, phase):
        return _mask(d, b, q_of=lambda q, k: k, k_of=lambda q, k: q)


class NextHead(TorchDropAttention):
    """the mask of head s + 1"""
    def mask(self, d, b, phase):
        return _mask(d, b, s0=1)


class SiteIgnored(TorchDropAttention):
    def mask(self, d, b, phase):
        return _mask(d, b, site=0)


class BytesReversed(TorchDropAttention):
    """byte 3 - (k & 3) of the word"""
    def mask(self, d, b, phase):
        return _mask(d, b, k_of=lambda q, k: (k & ~np.uint64(3)) | (np.uint64(3) - (k & np.uint64(3))))


class TileLocalKey(TorchDropAttention):
    """the key index inside the 64-key tile instead of the sequence's"""
    def mask(self, d, b, phase):
        return _mask(d, b, k_of=lambda q, k: k & np.uint64(63))


class NoRescaleInBackward(TorchDropAttention):
    """1 / keep missing in the backward only"""
    def rkeep_bwd(self, d):
        return torch.tensor(1.0)


class DeltaFromUndroppedO(TorchDropAttention):
    """delta formed from the o of the undropped softmax"""
    def o_for_delta(self, c, o_dense, o_f32, b):
        return A.TorchAttention().fwd_seq(c, A.attn_inputs(c)["qkv"], b)[0].to(A.TD[c.dt]).float()


class ZeroDsOnDropped(TorchDropAttention):
    """dS = 0 on dropped elements instead of -P delta"""
    def ds(self, P, x, ndelta, m):
        return torch.where(m, P * (x + ndelta), torch.zeros_like(P))


_B = PA_BF16
FAULTS = (
    (QueryAndKeyExchanged, (DC(AC(_B, 1, 3, 65, "select"), 128, site=1), DC(AC(PA_F32, 1, 3, 33, "graded", PRE), 26, site=1))),
    (NextHead, (DC(AC(_B, 1, 3, 65, "select", PRE), 128), DC(AC(PA_F32, 2, 3, 33, "uniform"), 26))),
    (SiteIgnored, (DC(AC(_B, 1, 3, 65, "pair"), 128, site=4), DC(AC(PA_F32, 1, 3, 65, "graded", nq=2), 26, site=4))),
    (BytesReversed, (DC(AC(_B, 1, 3, 33, "select"), 128), DC(AC(PA_F32, 1, 1, 64, "uniform", PRE), 26))),
    (TileLocalKey, (DC(AC(_B, 1, 3, 129, "select"), 128), DC(AC(PA_F32, 1, 3, 129, "graded", nq=2), 26))),
    (NoRescaleInBackward, (DC(AC(_B, 1, 3, 65, "select"), 128), DC(AC(PA_F32, 1, 3, 65, "graded", PRE), 26))),
    (DeltaFromUndroppedO, (DC(AC(_B, 1, 3, 65, "select"), 128), DC(AC(PA_F32, 1, 3, 65, "graded"), 26))),
    (ZeroDsOnDropped, (DC(AC(_B, 1, 3, 65, "pair"), 128), DC(AC(PA_F32, 1, 3, 65, "graded", PRE), 26))),
)


@pytest.mark.parametrize("model,cases", FAULTS, ids=lambda x: x.__name__ if isinstance(x, type) else "")
def test_fault_model_is_rejected(model, cases):
    for d in cases:
        DR.check_dropout(TorchDropAttention(), d)              # the case itself is one an honest implementation passes
        with pytest.raises(AssertionError):
            DR.check_dropout(model(), d)


# ---- the C entries refuse without a device ---------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    f = ctypes.c_float(0.125)

    def fwd(qkv=q, ldqkv=192, o=q, ldo=64, lse=q, B=1, H=1, N=4, nq=4, dt=1, flags=0, seed=q, site=0, t=128):
        return lib.pa_attention_fwd_dropout(qkv, ldqkv, o, ldo, lse, B, H, N, nq, f, dt, flags, seed, site, t, None)

    def bwd(qkv=q, ldqkv=192, o=q, d_o=q, ldo=64, lse=q, delta=q, dqkv=q, lddqkv=192, B=1, H=1, N=4, nq=4, dt=1, flags=0, seed=q, site=0, t=128):
        return lib.pa_attention_bwd_dropout(qkv, ldqkv, o, d_o, ldo, lse, delta, dqkv, lddqkv, B, H, N, nq, f, dt, flags, seed, site, t, None)
    common = (dict(seed=None), dict(t=0), dict(t=256), dict(t=-3), dict(qkv=None), dict(o=None), dict(lse=None), dict(B=0), dict(H=0), dict(N=0),
              dict(nq=0), dict(nq=5), dict(dt=7), dict(ldqkv=184), dict(ldo=56))
    for kw in common + (dict(flags=2), dict(flags=16)):                    # a backward-only flag, an unknown bit
        assert fwd(**kw) == A.PA_EINVAL, kw
    for kw in common + (dict(d_o=None), dict(delta=None), dict(dqkv=None), dict(lddqkv=184), dict(flags=16), dict(flags=1 | 32)):
        assert bwd(**kw) == A.PA_EINVAL, kw
    assert fwd(ldqkv=194) == A.PA_EUNSUPPORTED and bwd(lddqkv=194) == A.PA_EUNSUPPORTED       # rows off 16-byte alignment
    # the Python bindings refuse a host seed, a wrong t and a wrong seed shape before they reach the library
    x = torch.zeros(4, 192)
    for seed, t in ((torch.zeros(3, dtype=torch.int32), 128), (torch.zeros(2), 128), ((1, 2), 128)):
        with pytest.raises(_lib.PasstAmdError):
            ops.attention_fwd_dropout(x, 1, 1, 4, 0.125, seed, 0, t)
    for t in (0, 256, 12.5):
        with pytest.raises(ValueError):
            ops.attention_fwd_dropout(x, 1, 1, 4, 0.125, torch.zeros(2, dtype=torch.int32), 0, t)


# ---- Python level ---------------------------------------------------------------------------------------------------------------
SMALL = dict(img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, num_heads=2, distilled=True, s_patchout_t=6, s_patchout_f=3)


def _net(depth=3, rates=(0.0, 0.25, 0.5)):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(depth=depth, **SMALL)
    for blk, p in zip(net.blocks, rates):
        blk.attn.attn_drop.p = p                                       # the reference's way: get_model() has no dropout argument
    return net


def test_attn_drop_rates():
    net = _net().train()
    assert passt_amd.attn_drop_rates(net) == [0, 64, 128] == P.attn_drop_rates(net)
    assert P.attn_drop_rates(net.eval()) == [0, 0, 0]
    net.train()
    net.blocks[1].attn.attn_drop = torch.nn.Identity()                 # a module without p
    net.blocks[2].attn.attn_drop.p = 0.1
    assert P.attn_drop_rates(net) == [0, 0, 26]
    net.blocks[0].attn.attn_drop.p = 0.999
    with pytest.raises(ValueError, match="255/256"):
        P.attn_drop_rates(net)
    # the constructor keeps refusing the rates, and now says where attention dropout is set
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(NotImplementedError, match=r"attn_drop\.p"):
            passt_amd.PaSST(depth=1, attn_drop_rate=0.1, **SMALL)


def test_refusals_come_before_any_draw():
    net = _net().train()
    net.varlen_train = True
    x = torch.zeros(S.X_SHAPE)
    state = torch.get_rng_state()
    with pytest.raises(NotImplementedError, match="attention dropout"):
        net(x, lengths=S.LENGTHS)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        P.passt_forward_varlen(net, x, S.LENGTHS)
    xg = torch.zeros(S.X_SHAPE, requires_grad=True)
    net.input_grad = True
    with pytest.raises(NotImplementedError, match="attn_grad"):
        net(xg, attn=[1], attn_grad="grad")
    with pytest.raises(NotImplementedError, match="rollout"):
        net(xg, rollout="cam", rollout_from=2)
    assert torch.equal(torch.get_rng_state(), state)                   # nothing drawn
    with pytest.raises(ValueError):
        P.attn_drop_seed_tensor((1, 2 ** 32), "cpu")
    assert P.attn_drop_seed_tensor((2 ** 32 - 1, 7), "cpu").tolist() == [-1, 7]


def _drop_ops(rec, mp):
    """stand-ins of the two dropout ops next to the recorder's own"""
    def fwd(qkv, B, H, N, scale, seed, site, t, nq=None, flags=0):
        return S._attention_fwd(qkv, B, H, N, scale, nq=nq, flags=flags)

    def bwd(qkv, o, d_o, lse, B, H, N, scale, seed, site, t, nq=None, flags=0):
        return torch.zeros_like(qkv)
    mp.setattr(ops, "attention_fwd_dropout", rec.op("attention_fwd_dropout", fwd))
    mp.setattr(ops, "attention_bwd_dropout", rec.op("attention_bwd_dropout", bwd))


def _trace(net, seed=None, autograd=False):
    def case(rec, mp):
        _drop_ops(rec, mp)
        net.precision = "bf16"
        kw = {} if seed is None else dict(attn_drop_seed=seed)
        if autograd:
            x = torch.zeros(S.X_SHAPE)
            logits, feat = net(x, **kw)
            (logits.sum() + feat.sum()).backward()
        else:
            S._direct(rec, net, lambda n: P.passt_forward(n, torch.zeros(S.X_SHAPE), save=True, **kw), P.passt_backward)
    return S._record(case)


@pytest.mark.parametrize("autograd", [False, True])
def test_which_blocks_launch_the_dropout_entries(autograd):
    net = _net().train()
    trace = _trace(net, autograd=autograd)
    att = [e for e in trace if e[0].startswith("attention_")]
    # forward: block 0 plain, block 1 (t = 64) and block 2 (the prefix-only tail, t = 128, nq = 2) with site = block index;
    # backward: blocks 2, 1 with the same site and t, then block 0 plain
    assert [e[0] for e in att] == ["attention_fwd", "attention_fwd_dropout", "attention_fwd_dropout", "attention_bwd_dropout",
                                   "attention_bwd_dropout", "attention_bwd"]
    assert [e[1][-2:] for e in att[1:3]] == [[1, 64], [2, 128]] and [e[1][-2:] for e in att[3:5]] == [[2, 128], [1, 64]]
    assert all(e[1][-3] == "i32[2]" for e in att[1:5])
    assert att[2][2].get("nq") == 2 and att[3][2].get("nq") == 2
    # a replayed seed draws nothing more than a model without dropout draws
    quiet = _trace(_net(rates=(0, 0, 0)).train(), autograd=autograd)
    assert _trace(net, seed=(5, 6), autograd=autograd)[-1] == quiet[-1] != trace[-1]


def test_eval_and_rate_zero_launch_and_draw_what_they_always_did():
    def run(net, **kw):
        def case(rec, mp):
            net.precision = "bf16"
            with torch.no_grad():
                rec.log("returned", net(torch.zeros(S.X_SHAPE), **kw))
        return S._record(case)
    def plain():                                                       # a model never touched (a fresh one per run: the first run stages weights)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return passt_amd.PaSST(depth=3, **SMALL)
    assert run(_net().eval()) == run(plain().eval()) == run(_net().eval(), attn_drop_seed=(1, 2))     # ignored in eval mode
    assert run(_net(rates=(0, 0, 0)).train()) == run(plain().train())
    # the draw itself: one (2,) int32 tensor from the device's default generator
    torch.manual_seed(1234)
    P.patchout_draws(plain().train(), S.X_SHAPE)
    want_state = torch.get_rng_state()
    want = P.attn_drop_draw("cpu")
    torch.set_rng_state(want_state)
    assert torch.equal(P.attn_drop_draw("cpu"), want) and want.dtype == torch.int32 and tuple(want.shape) == (2,)

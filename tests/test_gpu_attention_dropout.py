"""pa_attention_fwd_dropout / pa_attention_bwd_dropout on the device, through the C ABI with guarded buffers and padded leading
dimensions (the conventions of tests/test_gpu_attention_exact.py).  tests/attention_dropout_cases.py holds the mask rule's numpy
restatement, the f64 references, the bounds and the checkers; tests/test_attention_dropout_cpu.py runs the same checkers against plain
torch and shows the fault models they reject.  The worst got / bound per group goes to attention_dropout_parity_metrics.json in
$PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root).

Mask read-out: with q = 0 the probabilities are 1 / N, and with v[k][d] = 2^(k >> 6) where d == (k & 63) (0 elsewhere)
o[q][d] N keep is the integer whose bit g is the mask of key 64 g + d: the kernel's own mask, element by element, decoded from its
output and compared with the host entry (pa_attention_dropout_mask) by torch.equal."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import ops  # noqa: E402
from tests import attention_cases as A  # noqa: E402
from tests import attention_dropout_cases as DR  # noqa: E402
from tests.attention_cases import F32, PA_BF16, PA_F32, PA_OK, SCALE, TD, GuardedOut  # noqa: E402
from tests.test_gpu_attention_exact import DEV, Hip, guards_only  # noqa: E402

_METRICS, _COUNTS = {}, {}


def record(group, ratio):
    _METRICS[group] = max(_METRICS.get(group, 0.0), float(ratio))
    _COUNTS[group] = _COUNTS.get(group, 0) + 1
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_metrics")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "attention_dropout_parity_metrics.json"), "w") as f:
        json.dump({k: {"worst_got_over_bound": v, "checks": _COUNTS[k]} for k, v in _METRICS.items()}, f, indent=1, sort_keys=True)


def seed_words(seed):
    return torch.tensor([v - 2 ** 32 if v >= 2 ** 31 else v for v in seed], dtype=torch.int32)


class HipDrop(Hip):
    """the two dropout entries behind the calling conventions of attention_dropout_cases.TorchDropAttention"""

    def launch_fwd(self, dt, B, H, N, nq, qkv, seed, site, t, flags):
        D = H * A.HD
        q = self.gin(qkv, A.PAD_QKV)
        sd = A.guarded_in(seed_words(seed), DEV)
        o, lse = A.new_out(B * nq, D, A.PAD_O, TD[dt], DEV), GuardedOut(B * H * nq, F32, DEV)
        rc = self.lib.pa_attention_fwd_dropout(q.data_ptr(), 3 * D + A.PAD_QKV, o.ptr(), D + A.PAD_O, lse.ptr(), B, H, N, nq, SCALE, dt, flags,
                                               sd.data_ptr(), site, t, self.st)
        torch.cuda.synchronize()
        return rc, dict(o=o, lse=lse)

    def fwd_drop(self, d):
        c = d.c
        return self.launch_fwd(c.dt, c.B, c.H, c.N, c.nqk, A.attn_inputs(c)["qkv"], d.seed, d.site, d.t, c.flags & A.PRE)

    def bwd_drop(self, d, o, d_o, lse, flags=None):
        c = d.c
        qkv = A.attn_inputs(c)["qkv"]
        keep = [self.gin(qkv, A.PAD_QKV), self.gin(o, A.PAD_O), self.gin(d_o, A.PAD_O), A.guarded_in(lse, DEV), A.guarded_in(seed_words(d.seed), DEV)]
        g = A.new_out(c.T, 3 * c.D, A.PAD_DQKV, TD[c.dt], DEV)
        ws = GuardedOut(self.lib.pa_attention_bwd_ws_floats(c.B, c.H, c.nqk), F32, DEV)
        rc = self.lib.pa_attention_bwd_dropout(keep[0].data_ptr(), 3 * c.D + A.PAD_QKV, keep[1].data_ptr(), keep[2].data_ptr(), c.D + A.PAD_O,
                                               keep[3].data_ptr(), ws.ptr(), g.ptr(), 3 * c.D + A.PAD_DQKV, c.B, c.H, c.N, c.nqk, SCALE, c.dt,
                                               (c.flags & A.PRE) | (flags or 0), keep[4].data_ptr(), d.site, d.t, self.st)
        torch.cuda.synchronize()
        guards_only(ws, d.name + " delta")
        return rc, dict(dqkv=g, ws=ws)


@pytest.fixture(scope="module")
def hip():
    return HipDrop()


# ---- mask read-out -----------------------------------------------------------------------------------------------------------
READ_N = (1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 257, 512)
READ_T = (128, 64, 26, 255, 1)
GROUPS_PER_LAUNCH = {PA_F32: 8, PA_BF16: 6}      # bf16 holds 8 bits: 6 key groups decode with a margin (|error| < 64 * 2^-9 = 1 / 8)


def readout_qkv(B, H, N, dt, key_of_column, weight_of_key, seed):
    """q = 0, k arbitrary integers, v[k][d] = weight_of_key(k) where key_of_column selects it (else 0); the same v for every head"""
    g = torch.Generator().manual_seed(seed)
    D = H * A.HD
    k = torch.randint(-8, 9, (B * N, D), generator=g).float()
    v1 = torch.zeros(N, A.HD)
    for key in range(N):
        d = key_of_column(key)
        if d is not None:
            v1[key, d] = weight_of_key(key)
    v = v1.repeat(B, H)
    return torch.cat([torch.zeros(B * N, D), k, v], 1).to(TD[dt])


def decode(o, B, H, N, nq, keep, what):
    """o [B nq][H 64] -> integer [B][H][nq][64], asserting the decode is unambiguous"""
    val = o.double().view(B, nq, H, A.HD).permute(0, 2, 1, 3) * (N * keep)
    n = val.round()
    worst = float((val - n).abs().max())
    assert worst < 0.25, (what, "ambiguous decode: distance to the nearest integer", worst)
    return n.long()


def read_mask(hip, dt, B, H, N, nq, site, t, flags):
    """the kernel's keep mask bool (B, H, nq, N), its lse, and the raw o of every launch"""
    per = GROUPS_PER_LAUNCH[dt]
    ng = (N + 63) // 64
    keep = DR.keep_of(t)
    mask = torch.zeros(B, H, nq, N, dtype=torch.bool)
    outs, lse = [], None
    for g0 in range(0, ng, per):
        qkv = readout_qkv(B, H, N, dt, lambda k: (k & 63) if g0 <= (k >> 6) < g0 + per else None, lambda k: 2.0 ** ((k >> 6) - g0), 17)
        rc, f = hip.launch_fwd(dt, B, H, N, nq, qkv, DR.SEED, site, t, flags)
        assert rc == PA_OK
        c = A.AC(dt, B, H, N, "uniform", flags, nq=nq if nq < N else 0)
        o, l = A.grab_fwd(c, f)
        bits = decode(o, B, H, N, nq, keep, f"dt{dt} B{B}H{H}N{N}nq{nq}t{t}")
        for g in range(g0, min(g0 + per, ng)):
            n = min(64, N - 64 * g)
            mask[..., 64 * g:64 * g + n] = ((bits >> (g - g0)) & 1)[..., :n].bool()
        assert int(bits.max()) < 2 ** min(per, ng - g0), "a key outside the launch's groups was counted"
        outs.append(o)
        lse = l
    return mask, lse, outs


@pytest.mark.parametrize("N", READ_N)
def test_mask_read_out_equals_the_host_mask(hip, N):
    for dt in (PA_F32, PA_BF16):
        for j, (B, H) in enumerate(((1, 1), (2, 3))):
            for t in READ_T:
                flags = A.PRE * ((j + t) & 1)
                site = (N + t) % 7
                want = ops.attn_drop_mask(DR.SEED, site, B, H, N, N, t / 256.0)
                got, lse, outs = read_mask(hip, dt, B, H, N, N, site, t, flags)
                assert torch.equal(got, want), (dt, B, H, N, t, int((got != want).sum()))
                gone = ~want.any(-1)                                            # every key of the row dropped
                for o in outs:
                    assert bool((o.view(B, N, H, A.HD).permute(0, 2, 1, 3)[gone] == 0).all()), "a fully dropped row is exactly 0"
                # lse: bit-identical to pa_attention_fwd on the same operands
                c = A.AC(dt, B, H, N, "uniform", flags)
                qkv = readout_qkv(B, H, N, dt, lambda k: k & 63, lambda k: 1.0, 17)
                rc, f = hip.fwd(c, qkv)
                assert rc == PA_OK
                _, lse0 = A.grab_fwd(c, f)
                assert torch.equal(lse, lse0), "lse differs from pa_attention_fwd's"
                if N > 2:
                    # the compact nq = 2 launch: rows 0 and 1 of the full launch, bit for bit
                    got2, lse2, outs2 = read_mask(hip, dt, B, H, N, 2, site, t, flags)
                    assert torch.equal(got2, want[:, :, :2])
                    for o, o2 in zip(outs, outs2):
                        assert torch.equal(o.view(B, N, -1)[:, :2].reshape(2 * B, -1), o2), "compact rows differ from rows 0, 1 of the full launch"
                    assert torch.equal(lse2.view(B * H, 2), lse.view(B * H, N)[:, :2])


@pytest.mark.parametrize("BH", ((1, 1), (2, 3)))
def test_mask_read_out_at_1190_keys(hip, BH):
    """N = 1190 through one-hot 64-key windows: both ends, and across key 1152 (the last full tile's edge)"""
    B, H = BH
    N = 1190
    for dt, t in ((PA_F32, 26), (PA_BF16, 128), (PA_BF16, 26)):
        want = ops.attn_drop_mask(DR.SEED, 11, B, H, N, N, t / 256.0)
        for w in (0, 1120, N - 64):
            qkv = readout_qkv(B, H, N, dt, lambda k: k - w if w <= k < w + 64 else None, lambda k: 1.0, w)
            rc, f = hip.launch_fwd(dt, B, H, N, N, qkv, DR.SEED, 11, t, A.PRE)
            assert rc == PA_OK
            o, _ = A.grab_fwd(A.AC(dt, B, H, N, "uniform", A.PRE), f)
            bits = decode(o, B, H, N, N, DR.keep_of(t), f"N1190 window {w}")
            assert int(bits.max()) <= 1
            assert torch.equal(bits.bool(), want[..., w:w + 64]), (dt, t, w)


# ---- forward and backward against the f64 reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", DR.N_FWD_BWD)
def test_forward_and_backward(hip, N):
    """the four families, nq = N and 2, both types, with and without the pre-scaled q, t = 128 (exact regime) and 26; NaN behind every
    operand (guarded_in / padded); sentinel around and between every output"""
    for d in DR.fwd_bwd_cases(N):
        DR.check_dropout(hip, d, record)


@pytest.mark.parametrize("N", (33, 129, 257))
def test_backward_is_the_same_under_every_form_flag(hip, N):
    """always the dQ + dK/dV pair: PA_ATTN_BWD_TWO_PASS / _SINGLE_PASS / _SINGLE_PASS_W16 are accepted and change no bit (bf16, pre-scaled
    q, nq == N <= 512 is where pa_attention_bwd itself would switch kernels)"""
    for fam in ("graded", "pair"):
        for t in (DR.T_EXACT, DR.T_GRADED):
            d = DR.DC(A.AC(PA_BF16, 2, 3, N, fam, A.PRE, seed=N), t, site=2)
            DR.check_dropout(hip, d, record, bwd_flags=(None, A.TWO_PASS, A.SINGLE_PASS, A.SINGLE_PASS_W16))


def test_refusals_launch_nothing(hip):
    """t outside 1..255 and a NULL seed: PA_EINVAL, every output keeps the sentinel"""
    from tests.test_gpu_attention_exact import untouched
    c = A.AC(PA_BF16, 1, 1, 4, "select")
    qkv = A.attn_inputs(c)["qkv"]
    for t in (0, 256, -1):
        rc, f = hip.launch_fwd(c.dt, 1, 1, 4, 4, qkv, DR.SEED, 0, t, 0)
        assert rc == A.PA_EINVAL
        for g in f.values():
            untouched(g, f"forward with t = {t}")

"""Exact-operand and guarded-buffer parity of the attention family -- pa_attention_fwd, pa_attention_bwd as the dQ + dK/dV kernel pair,
as the single pass in its 8-wave and 16-wave forms and as the library's own choice, the packed `_varlen` entries, pa_attention_probs,
pa_attention_probs_grad and pa_attention_rollout -- through the C ABI, so that the test owns every buffer (tests/attention_cases.py holds
the case lists, operand families, conditions, f64 references, bounds and checkers; the same checkers pass against plain torch in
tests/test_attention_cases_cpu.py).  The worst got / bound per group goes to attention_exact_parity_metrics.json in
$PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root); profiles/attention_exact_parity.txt keeps them."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from tests import attention_cases as A  # noqa: E402
from tests.attention_cases import F32, PA_BF16, PA_EINVAL, PA_F32, PA_OK, SCALE, SENTINEL, TD, GuardedOut  # noqa: E402

DEV = "cuda"
_METRICS = {}
_COUNTS = {}


def record(group, ratio):
    _METRICS[group] = max(_METRICS.get(group, 0.0), float(ratio))
    _COUNTS[group] = _COUNTS.get(group, 0) + 1
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_metrics")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "attention_exact_parity_metrics.json"), "w") as f:
        json.dump({k: {"worst_got_over_bound": v, "checks": _COUNTS[k]} for k, v in _METRICS.items()}, f, indent=1, sort_keys=True)


def guards_only(g, what):
    """a workspace: only its guards are checked"""
    buf = g.buf.cpu()
    assert bool((buf[:g.lo] == SENTINEL).all()) and bool((buf[g.lo + g.n:] == SENTINEL).all()), f"{what}: a write outside the buffer"


def untouched(g, what):
    assert bool((g.buf == SENTINEL).all()), f"{what}: written"


class Hip:
    """The C entries of libpasst_amd.so behind the calling conventions of attention_cases.TorchAttention.  Every operand is a view into a
    larger allocation with NaN in front of it, behind it and in the gap columns of its padded leading dimension; every output and
    workspace is a GuardedOut filled with the sentinel."""
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self.st = torch.cuda.current_stream().cuda_stream

    @staticmethod
    def gin(t, pad=0):
        if t is None:
            return None
        return A.guarded_in(A.padded(t, t.shape[1] + pad) if pad else t, DEV)

    @staticmethod
    def ptr(t):
        return t.data_ptr() if t is not None else None

    def cu(self, c):
        return A.guarded_in(torch.tensor(c.cu, dtype=torch.int32), DEV) if c.packed else None

    def fwd(self, c, qkv, ld=None):
        ld = {**dict(ldqkv=3 * c.D + A.PAD_QKV, ldo=c.D + A.PAD_O), **(ld or {})}
        q = self.gin(qkv, A.PAD_QKV)
        o, lse, cu = A.new_out(c.o_rows, c.D, A.PAD_O, TD[c.dt], DEV), GuardedOut(c.n_lse, F32, DEV), self.cu(c)
        if c.packed:
            rc = self.lib.pa_attention_fwd_varlen(q.data_ptr(), ld["ldqkv"], o.ptr(), ld["ldo"], lse.ptr(), cu.data_ptr(), c.B, c.H, c.N, c.nqk,
                                                  SCALE, c.dt, c.flags & A.PRE, self.st)
        else:
            rc = self.lib.pa_attention_fwd(q.data_ptr(), ld["ldqkv"], o.ptr(), ld["ldo"], lse.ptr(), c.B, c.H, c.N, c.nqk, SCALE, c.dt,
                                           c.flags & A.PRE, self.st)
        torch.cuda.synchronize()
        return rc, dict(o=o, lse=lse)

    def bwd(self, c, qkv, o, d_o, lse, ld=None):
        ld = {**dict(ldqkv=3 * c.D + A.PAD_QKV, ldo=c.D + A.PAD_O, lddqkv=3 * c.D + A.PAD_DQKV), **(ld or {})}
        keep = [self.gin(qkv, A.PAD_QKV), self.gin(o, A.PAD_O), self.gin(d_o, A.PAD_O), A.guarded_in(lse, DEV), self.cu(c)]
        g = A.new_out(c.T, 3 * c.D, A.PAD_DQKV, TD[c.dt], DEV)
        if c.packed:
            ws = GuardedOut(self.lib.pa_attention_bwd_varlen_ws_floats(c.T, c.B, c.H, c.nqk), F32, DEV)
            rc = self.lib.pa_attention_bwd_varlen(keep[0].data_ptr(), ld["ldqkv"], keep[1].data_ptr(), keep[2].data_ptr(), ld["ldo"], keep[3].data_ptr(),
                                                  ws.ptr(), g.ptr(), ld["lddqkv"], keep[4].data_ptr(), c.B, c.H, c.N, c.nqk, SCALE, c.dt, c.flags, self.st)
        else:
            ws = GuardedOut(self.lib.pa_attention_bwd_ws_floats(c.B, c.H, c.nqk), F32, DEV)
            rc = self.lib.pa_attention_bwd(keep[0].data_ptr(), ld["ldqkv"], keep[1].data_ptr(), keep[2].data_ptr(), ld["ldo"], keep[3].data_ptr(), ws.ptr(),
                                           g.ptr(), ld["lddqkv"], c.B, c.H, c.N, c.nqk, SCALE, c.dt, c.flags, self.st)
        torch.cuda.synchronize()
        guards_only(ws, c.name + " delta / ws")
        if rc == PA_OK and c.single_pass:
            untouched(ws, c.name + ": the single pass leaves delta alone, but it was")
        return rc, dict(dqkv=g, ws=ws)

    def probs(self, c, qkv, lse, head_mean, d_o=None, mode=None, ld=None):
        ld = {**dict(ldqkv=3 * c.D + A.PAD_QKV, ldo=c.D + A.PAD_O), **(ld or {})}
        off = A.map_offsets(c, head_mean)
        keep = [self.gin(qkv, A.PAD_QKV), A.guarded_in(lse, DEV), self.gin(d_o, A.PAD_O), self.cu(c),
                A.guarded_in(torch.tensor(off[:-1], dtype=torch.int64), DEV) if c.packed else None]
        g = GuardedOut(off[-1], F32, DEV)
        if mode is None:
            rc = self.lib.pa_attention_probs(keep[0].data_ptr(), ld["ldqkv"], keep[1].data_ptr(), g.ptr(), self.ptr(keep[3]), self.ptr(keep[4]), c.B, c.H,
                                             c.N, c.nqk, head_mean, SCALE, c.dt, c.flags & A.PRE, self.st)
        else:
            rc = self.lib.pa_attention_probs_grad(keep[0].data_ptr(), ld["ldqkv"], self.ptr(keep[1]), keep[2].data_ptr(), ld["ldo"], A.do_compact(c), g.ptr(),
                                                  self.ptr(keep[3]), self.ptr(keep[4]), c.B, c.H, c.N, c.nqk, head_mean, mode, SCALE, c.dt,
                                                  c.flags & A.PRE, self.st)
        torch.cuda.synchronize()
        return rc, g

    def rollout(self, c, qkv, lse, d_o, r_in, mode, slices, a, b_, g_scale, ld=None):
        ld = {**dict(ldqkv=3 * c.D + A.PAD_QKV, ldo=c.D + A.PAD_O), **(ld or {})}
        keep = [self.gin(qkv, A.PAD_QKV), A.guarded_in(lse, DEV), self.gin(d_o, A.PAD_O), self.cu(c), A.guarded_in(r_in, DEV)]
        g = GuardedOut(A.NR * c.T, F32, DEV)
        ws = GuardedOut(max(1, self.lib.pa_attention_rollout_ws_floats(c.T, c.B, c.N, c.nqk, A.NR, slices)), F32, DEV)
        rc = self.lib.pa_attention_rollout(keep[0].data_ptr(), ld["ldqkv"], keep[1].data_ptr(), self.ptr(keep[2]), ld["ldo"] if d_o is not None else 0,
                                           A.do_compact(c) if d_o is not None else 0, keep[4].data_ptr(), g.ptr(), ws.ptr(), self.ptr(keep[3]), c.T, c.B,
                                           c.H, c.N, c.nqk, A.NR, mode, slices, a, b_, g_scale, SCALE, c.dt, c.flags & A.PRE, self.st)
        torch.cuda.synchronize()
        guards_only(ws, c.name + " rollout ws")
        return rc, g


@pytest.fixture(scope="module")
def hip():
    return Hip()


def run(hip, cases):
    for c in cases:
        A.check_attention(hip, c, record)


@pytest.mark.parametrize("N", A.N_PAIR_FORMS)
def test_forward_and_kernel_pair(hip, N):
    """forward and the dQ + dK/dV pair at every tile-edge length: both types, with and without the pre-scaled q, every family"""
    run(hip, A.pair_form_cases(N))


@pytest.mark.parametrize("N", A.N_SINGLE)
def test_single_pass_backward(hip, N):
    """bf16: the single pass as eight and as sixteen waves and the library's own choice, bit for bit against the f64 result rounded once"""
    run(hip, A.single_cases(N))


@pytest.mark.parametrize("N", A.NQ_N)
def test_prefix_queries(hip, N):
    """compact o / d_o / lse; the Q third of rows q >= nq keeps the sentinel"""
    run(hip, A.prefix_cases(N))


@pytest.mark.parametrize("lens", A.PACKED, ids=lambda x: "-".join(map(str, x)))
def test_packed(hip, lens):
    """every query and nq = 2: compact rows q >= N_b keep the sentinel, the Q third of rows q >= nq is zero, nothing behind cu_tok[B]"""
    run(hip, A.packed_cases(lens))


def test_sibling_entries(hip):
    for c in A.sibling_cases():
        A.check_siblings(hip, c, record)


def test_leading_dimension_refusals(hip):
    """every entry refuses a leading dimension below its row width with PA_EINVAL and launches nothing: every output keeps the sentinel"""
    for packed in (False, True):
        c = A.AC(PA_BF16, 2, 1, 4, "select", lens=(4, 3) if packed else ())
        i, r = A.attn_inputs(c), A.reference(c)
        lse = A.ref_lse(c, r)
        o = A.to_rows([rb["o"].float() for rb in r], c, "o").to(TD[c.dt])
        r_in = torch.ones(A.NR * c.T)
        small = dict(ldqkv=3 * c.D - 8, ldo=c.D - 8, lddqkv=3 * c.D - 8)
        for entry, arg in A.LD_ARG_CASES:
            if entry.endswith("_varlen") != packed and entry in ("fwd", "bwd", "fwd_varlen", "bwd_varlen"):
                continue
            ld = {arg: small[arg]}
            if entry.startswith("fwd"):
                rc, outs = hip.fwd(c, i["qkv"], ld=ld)
                outs = list(outs.values())
            elif entry.startswith("bwd"):
                rc, outs = hip.bwd(c, i["qkv"], o, i["d_o"], lse, ld=ld)
                outs = list(outs.values())
            elif entry == "probs":
                rc, g = hip.probs(c, i["qkv"], lse, 0, ld=ld)
                outs = [g]
            elif entry == "probs_grad":
                rc, g = hip.probs(c, i["qkv"], lse, 0, d_o=i["d_o"], mode=A.PGRAD_CAM, ld=ld)
                outs = [g]
            else:
                rc, g = hip.rollout(c, i["qkv"], lse, i["d_o"], r_in, A.ROLLOUT_CAM, 1, 1.0, 1.0, 1.0, ld=ld)
                outs = [g]
            assert rc == PA_EINVAL, (entry, arg, packed, rc)
            for g in outs:
                untouched(g, f"{entry} with {arg} below the row width")

"""The launch sequence of passt_amd/passt.py, op by op, without a GPU.

Every ``ops`` function the kernel sequence calls is replaced by a recorder that returns a CPU tensor of the right shape and dtype
and logs [op name, positional arguments, keyword arguments, stream]: a tensor is logged as dtype[shape], a scalar as itself, a list
(the deferred row reductions, the batched weight-gradient problems) entry by entry.  ``_SideStream`` is replaced by a recorder of
fork / join whose fork makes the stream marker "side" while it is open (when the model asked for the side stream), and the
``on_block_done`` callback logs the block index with the stream it fired from.  A depth-2, D=128 model is driven through the fixed
and the packed path, forward and backward, through the public functions and through ``net(x)`` + autograd.

The expected traces (tests/golden/sequence_traces.json) were recorded by this same harness on the commit named in the fixture's
note, when passt.py still held the fixed and the packed kernel sequence as two copies: the shared trunk must launch exactly what
each copy launched, in the same order, on the same stream.  The cases added since (``hidden=``, ``attn=``, ``varlen_train``, the
bound flat gradient buffer) were recorded on the commit the fixture's ``notes_added`` names, before the host code around the trunk
was reshaped; they also end in ["rng", digest of the CPU generator's state after the call], so the order and number of the Patchout
draws is part of the trace (the first ten cases keep their traces as recorded and have their digests in the fixture's ``rng``).
``python -m tests.test_sequence_cpu --write`` records the cases the fixture does not hold yet and leaves the others as they are.

One case has no recorded trace: ``packed_bf16_no_defer_rows``.  The packed copy of the backward never read the A/B switches; going
through the shared weight-gradient scheduling it honours them now, which is new behaviour, so the test asserts what the switch
means (no reduction is deferred to the block's finishing launch) instead of equality with the parent."""
import contextlib
import hashlib
import json
import os
import warnings

import numpy as np
import pytest
import torch

import passt_amd
from passt_amd import ops
from passt_amd import passt as P

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_traces.json")
SWITCHES = ("PASST_AMD_NO_BATCH_WGRAD", "PASST_AMD_NO_DEFER_ROWS", "PASST_AMD_NO_FUSED_BIAS", "PASST_AMD_BIAS_FROM_WGRAD", "PA_EPILOGUE_V3",
            "PASST_AMD_NO_BATCH_STAGE")
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64"}


def _brief(v):
    if torch.is_tensor(v):
        return f"{_DT[v.dtype]}{list(v.shape)}"
    if isinstance(v, np.ndarray):
        return f"np.{v.dtype}{list(v.shape)}"
    if isinstance(v, (list, tuple)):
        return [_brief(e) for e in v]
    if isinstance(v, torch.device):
        return str(v)
    assert v is None or isinstance(v, (bool, int, float, str)), type(v)
    return v


class _Recorder:
    def __init__(self):
        self.trace, self.stream = [], "main"

    def log(self, name, args=(), kwargs=None):
        self.trace.append([name, _brief(args), {k: _brief(v) for k, v in (kwargs or {}).items()}, self.stream])

    def op(self, name, result):
        def fake(*args, **kwargs):
            self.log(name, args, kwargs)          # before the stand-in runs: the deferred-job lists are logged as the op received them
            return result(*args, **kwargs)
        return fake

    @contextlib.contextmanager
    def on(self, stream):
        prev, self.stream = self.stream, stream
        try:
            yield
        finally:
            self.stream = prev


def _lp(dt):
    return ops.TORCH_DTYPE[dt]


def _e(shape, dtype=torch.float32):
    return torch.zeros(tuple(shape), dtype=dtype)


def _layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, want_lp, accumulate=False, dcolsum=None, defer=None):
    dx = _e(x.shape)
    if defer is not None and not accumulate:
        for out in (dgamma, dbeta, dcolsum):
            if out is not None:
                defer.append((_e((1,)), 1, 3 * x.shape[1], x.shape[1], out))
    return dx, dx if dy.dtype == torch.float32 else (_e(x.shape, dy.dtype) if want_lp else None)


def _dgelu_gemm(dy, Wt, pre, dt, colsum_out=None, colsum_ws=None, defer=None):
    if defer is not None and colsum_out is not None:
        defer.append((colsum_ws, 1, pre.shape[1], pre.shape[1], colsum_out))
    return _e(pre.shape, _lp(dt))


def _attention_fwd_varlen(qkv, cu_tok, B, H, max_N, scale, nq=None, flags=0):
    if nq is None:
        return _e((qkv.shape[0], H * 64), qkv.dtype), _e((H, qkv.shape[0]))
    return _e((B * nq, H * 64), qkv.dtype), _e((B * H * nq,))


def _attention_fwd(qkv, B, H, N, scale, nq=None, flags=0):
    nq = N if nq is None else nq
    return _e((B * nq, H * 64), qkv.dtype), _e((B * H * nq,))


def _layernorm_fwd(x, g, b, eps, dt, save_stats=True):
    return _e(x.shape, _lp(dt)), (_e(x.shape[:1]) if save_stats else None), (_e(x.shape[:1]) if save_stats else None)


def _layernorm_bwd2(dy, x, gamma, mean, rstd, dres, dres2, dgamma, dbeta, want_lp, accumulate=False, dcolsum=None, defer=None):
    assert dres2 is not None and dres2.shape == x.shape and dres2.dtype == torch.float32
    return _layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, want_lp, accumulate=accumulate, dcolsum=dcolsum, defer=defer)


def _tail_inject(rows, idx, n, add0, add1, dt):
    dx = _e((n, rows.shape[1]))
    return dx, dx if _lp(dt) == torch.float32 else _e(dx.shape, _lp(dt))


def _probs(qkv, lse, B, H, N, scale, nq=None, head_mean=False, flags=0, out=None):
    nq = N if nq is None else nq
    assert lse.numel() == B * H * nq and lse.dtype == torch.float32 and flags == ops.ATTN_Q_PRESCALED
    return _e((B, 1 if head_mean else H, nq, N))


def _probs_varlen(qkv, lse, cu_tok, out_off, total_out, B, H, max_N, scale, nq=None, head_mean=False, flags=0, out=None):
    assert lse.numel() == (H * qkv.shape[0] if nq is None else B * H * nq) and out_off.dtype == torch.int64 and out_off.numel() == B
    return _e((total_out,))


# op name -> what the stand-in returns (shapes and dtypes as passt_amd/ops.py documents them)
_RESULTS = {
    "upload_small": lambda host, device: torch.from_numpy(np.ascontiguousarray(host)),
    "convert": lambda x, dt: x if _lp(dt) == torch.float32 else _e(x.shape, _lp(dt)),
    "transpose": lambda x, dt, ldo=None, out=None: _e((x.shape[1], x.shape[0]), _lp(dt)),
    "patch_gather": lambda x, pf, pt, P_, fs, ts, dt: _e((x.shape[0] * pf.numel(), P_ * P_), _lp(dt)),
    "patch_pos_table": lambda bias, tp, fp, pf, pt, toff, cls, dist, npe, tok: _e((pf.numel(), tok.shape[-1])),
    "patch_gather_varlen": lambda x, rc, rf, rt, P_, fs, ts, dt: _e((rf.numel(), P_ * P_), _lp(dt)),
    "patch_pos_table_varlen": lambda bias, tp, fp, rf, rt, cls, dist, npe: _e((rf.numel(), bias.numel())),
    "gemm_nt": lambda *a, **k: None,
    "layernorm_fwd": _layernorm_fwd,
    "linear": lambda x, W, b, dt, colscale_n=0, colscale=1.0: _e((x.shape[0], W.shape[0]), _lp(dt)),
    "attention_fwd": _attention_fwd,
    "attention_fwd_varlen": _attention_fwd_varlen,
    "gather_rows": lambda x, idx: _e((idx.numel(),) + tuple(x.shape[1:]), x.dtype),
    "linear_resid": lambda x, W, b, resid, dt, out=None: _e(resid.shape),
    "linear_gelu": lambda x, W, b, dt: (_e((x.shape[0], W.shape[0]), _lp(dt)), _e((x.shape[0], W.shape[0]), _lp(dt))),
    "head_pre_fwd": lambda x, *a: (_e((x.shape[0], x.shape[2])), _e((x.shape[0], x.shape[2])), _e((x.shape[0], 6))),
    "linear_f32_fwd": lambda x, W, b: _e((x.shape[0], W.shape[0])),
    "linear_f32_bwd": lambda dy, x, W, dW, db, accumulate=False: _e(x.shape),
    "head_pre_bwd": lambda dhn, dfeat, x, *a: (_e(x.shape), _e((x.shape[0], 4 * x.shape[2]))),
    "colsum": lambda *a, **k: None,
    "colsum_f32": lambda *a, **k: None,
    "gemm_colsum_ws": lambda M, N, device, ws=None: _e((1,)) if ws is None else ws,
    "dgelu_gemm": _dgelu_gemm,
    "layernorm_bwd": _layernorm_bwd,
    "wgrad_tn": lambda dY, X, out, dt, accumulate=False, partial_ws=None, db=None: _e((1,)) if partial_ws is None else partial_ws,
    "wgrad_tn_batched": lambda problems, dt, partial_ws=None, row_jobs=None: _e((1,)) if partial_ws is None else partial_ws,
    "attention_bwd": lambda qkv, *a, **k: _e(qkv.shape, qkv.dtype),
    "attention_bwd_varlen": lambda qkv, *a, **k: _e(qkv.shape, qkv.dtype),
    "scatter_rows_into_zeros": lambda x, idx, n: _e((n,) + tuple(x.shape[1:]), x.dtype),
    "patch_bwd": lambda dtok, pf, pt, toff, Tpe, Fpe, *d_and_dt, **k: _e((dtok.shape[0] * pf.numel(), dtok.shape[2]), _lp(d_and_dt[6])),
    "patch_input_bwd": lambda dcols, pf, pt, B, F, T, *a, **k: _e((B, 1, F, T)),
    "patch_bwd_varlen": lambda *a, **k: None,
    "patch_input_bwd_varlen": lambda dcols, cu, B, F, T, *a, **k: _e((B, 1, F, T)),
    "patch_bwd_rows": lambda *a, **k: None,
    "patch_input_bwd_rows": lambda dcols, slot, F, T, *a, **k: _e((slot.shape[0], 1, F, T)),
    "layernorm_bwd2": _layernorm_bwd2,
    "tail_inject": _tail_inject,
    "attention_probs": _probs,
    "attention_probs_varlen": _probs_varlen,
}


def _install(mp, rec):
    for name, result in _RESULTS.items():
        mp.setattr(ops, name, rec.op(name, result))

    class SideStream:
        def __init__(self, device, enabled=True):
            self.enabled, self.stream = bool(enabled), None

        def fork(self, *tensors):
            rec.log("side.fork", tensors)
            return rec.on("side" if self.enabled else rec.stream)

        def join(self):
            rec.log("side.join")

    mp.setattr(P, "_SideStream", SideStream)
    mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))         # reach the launch sites on a box without a GPU
    for name in SWITCHES:
        mp.delenv(name, raising=False)


def _net(train):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 250), stride=10, num_classes=37, embed_dim=128, depth=2, num_heads=2, distilled=True,
                              s_patchout_t=6, s_patchout_f=3)
    return net.train(train)


X_SHAPE, LENGTHS = (2, 1, 128, 250), [250, 130]


def _direct(rec, net, forward, backward, frozen=False, want_dx=False):
    """Through the public kernel-sequence functions, with an ``on_block_done`` that logs where it fired."""
    logits, feat, ctx = forward(net)
    grads = None if frozen else {n: torch.zeros_like(p) for n, p in net.named_parameters() if not n.startswith("head_dist.")}
    dx = backward(net, ctx, torch.ones_like(logits), torch.ones_like(feat), grads, on_block_done=lambda i: rec.log("block_done", (i,)),
                  want_dx=want_dx)
    rec.log("returned", (logits, feat, dx))


def _autograd(rec, net, lengths=None):
    """Through PaSST.forward and the autograd node, for an input that requires a gradient."""
    x = torch.zeros(X_SHAPE, requires_grad=True)
    logits, feat = net(x) if lengths is None else net(x, lengths=lengths)
    (logits.sum() + feat.sum()).backward()
    rec.log("returned", (logits, feat, x.grad, [n for n, p in net.named_parameters() if p.grad is not None]))


def _fixed_fwd(net):
    return P.passt_forward(net, torch.zeros(X_SHAPE), save=True)


def _packed_fwd(net):
    return P.passt_forward_varlen(net, torch.zeros(X_SHAPE), LENGTHS, save=True)


def _case_fixed_train(rec, mp, precision, overlap=False, env=None):
    net = _net(True)
    net.precision, net.overlap_wgrad = precision, overlap
    if env:
        mp.setenv(env, "1")
    _direct(rec, net, _fixed_fwd, P.passt_backward)


def _case_fixed_frozen_want_dx(rec, mp):
    net = _net(False).requires_grad_(False)
    net.precision = "bf16"
    _autograd(rec, net)


def _case_fixed_input_grad(rec, mp):
    net = _net(True)
    net.precision, net.input_grad = "bf16", True
    _autograd(rec, net)


def _case_eval_forward(rec, mp, lengths=None):
    net = _net(False)
    net.precision = "bf16"
    with torch.no_grad():
        out = net(torch.zeros(X_SHAPE)) if lengths is None else net(torch.zeros(X_SHAPE), lengths=lengths)
    rec.log("returned", out)
    if lengths is not None:
        rec.log("last_dt", (net._last_dt,))           # the packed forward that saves nothing leaves it alone


def _case_packed_train(rec, mp, env=None):
    net = _net(False)
    net.precision = "bf16"
    if env:
        mp.setenv(env, "1")
    _direct(rec, net, _packed_fwd, P.passt_backward_varlen, want_dx=True)


def _case_packed_frozen_want_dx(rec, mp):
    net = _net(False).requires_grad_(False)
    net.precision, net.varlen_grad = "fp32", True
    _autograd(rec, net, LENGTHS)


def _step(rec, net, x_grad, lengths=None, **kw):
    """``net(x, ...)`` with the keywords of the newer modes + a backward of a loss on logits, features and every token output; logs
    the whole returned structure."""
    x = torch.zeros(X_SHAPE, requires_grad=x_grad)
    out = net(x, **kw) if lengths is None else net(x, lengths=lengths, **kw)
    loss = out[0].sum() + out[1].sum()
    for h in (out[2] if "hidden" in kw else ()):
        loss = loss + h.sum()
    loss.backward()
    rec.log("returned", (out, x.grad, [n for n, p in net.named_parameters() if p.grad is not None]))


def _case_fixed_keywords(rec, mp, precision, x_grad, **kw):
    net = _net(True)
    net.precision, net.input_grad = precision, x_grad
    _step(rec, net, x_grad, **kw)


def _case_keywords_nograd(rec, mp, lengths=None):
    net = _net(False)
    net.precision = "bf16"
    args = {} if lengths is None else dict(lengths=lengths)
    with torch.no_grad():
        out = net(torch.zeros(X_SHAPE), hidden=(0, "norm"), attn=(1, 0), **args)
    rec.log("returned", out)
    rec.log("last_dt", (net._last_dt,))


def _case_packed_keywords_grad(rec, mp):
    net = _net(False)
    net.precision, net.varlen_grad = "bf16", True
    _step(rec, net, True, LENGTHS, hidden=(0,), attn=(0,))


def _case_packed_varlen_train(rec, mp, frozen=False):
    net = _net(True).requires_grad_(not frozen)
    net.precision, net.varlen_train = "fp32", True
    _step(rec, net, True, LENGTHS)


def _case_fixed_flat_bound(rec, mp):
    """The single-token ``apply`` route of a model bound to an optimizer's flat gradient buffer."""
    net = _net(True)
    net.precision = "bf16"
    fl = net.bind_flat_grads(torch.zeros(net._graph_params()[1]))
    assert fl is not None and net._flat is fl and fl["fresh"]
    _step(rec, net, False)
    rec.log("flat", (fl["fresh"], all(p.grad is fl["grads"][n] for n, p in fl["named"])))


CASES = {
    "fixed_train_fp32": lambda r, mp: _case_fixed_train(r, mp, "fp32"),
    "fixed_train_bf16": lambda r, mp: _case_fixed_train(r, mp, "bf16"),
    "fixed_train_bf16_overlap_wgrad": lambda r, mp: _case_fixed_train(r, mp, "bf16", overlap=True),
    "fixed_frozen_want_dx": _case_fixed_frozen_want_dx,
    "fixed_trainable_input_grad": _case_fixed_input_grad,
    "fixed_eval_forward": lambda r, mp: _case_eval_forward(r, mp),
    "packed_eval_forward": lambda r, mp: _case_eval_forward(r, mp, LENGTHS),
    "packed_train": lambda r, mp: _case_packed_train(r, mp),
    "packed_frozen_want_dx": _case_packed_frozen_want_dx,
    "fixed_bf16_no_defer_rows": lambda r, mp: _case_fixed_train(r, mp, "bf16", env="PASST_AMD_NO_DEFER_ROWS"),
    "fixed_hidden_mid": lambda r, mp: _case_fixed_keywords(r, mp, "bf16", False, hidden=(0,)),
    "fixed_hidden_full_tail": lambda r, mp: _case_fixed_keywords(r, mp, "fp32", True, hidden=(-1, "norm")),
    "fixed_attn_prefix_mean": lambda r, mp: _case_fixed_keywords(r, mp, "bf16", False, attn=(-1, 0), attn_rows="prefix", attn_heads="mean"),
    "fixed_hidden_attn_nograd": lambda r, mp: _case_keywords_nograd(r, mp),
    "packed_hidden_attn_nograd": lambda r, mp: _case_keywords_nograd(r, mp, LENGTHS),
    "packed_hidden_attn_grad": _case_packed_keywords_grad,
    "packed_varlen_train": lambda r, mp: _case_packed_varlen_train(r, mp),
    "packed_varlen_train_frozen": lambda r, mp: _case_packed_varlen_train(r, mp, frozen=True),
    "fixed_flat_bound": _case_fixed_flat_bound,
}


def _record(case, seed=1234):
    """Trace of ``case(rec, mp)`` with every op replaced by its stand-in, closed by the digest of the CPU generator's state."""
    rec = _Recorder()
    with pytest.MonkeyPatch.context() as mp:
        _install(mp, rec)
        torch.manual_seed(seed)                    # the Patchout draws decide the token count
        case(rec, mp)
        rec.log("rng", (hashlib.sha1(torch.get_rng_state().numpy().tobytes()).hexdigest()[:16],))
    return json.loads(json.dumps(rec.trace))


def _record_run(run, seed=1234):
    """_record for a test body that needs the recorder only: the trace of ``run(rec)`` without the closing digest."""
    return _record(lambda rec, mp: run(rec), seed)[:-1]


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_is_the_recorded_one(name):
    with open(FIXTURE) as f:
        fixture = json.load(f)
    want = fixture["traces"][name]
    if want[-1][0] != "rng":                       # the first ten traces stay as recorded: their digests are kept beside them
        want = want + [fixture["rng"][name]]
    got = _record(CASES[name])
    assert len(want) > 20 and [e[0] for e in got] == [e[0] for e in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: launch {i}"


def test_packed_backward_honours_the_switches_of_the_shared_scheduling():
    """New behaviour (see the module docstring): under PASST_AMD_NO_DEFER_ROWS=1 the packed backward defers nothing either."""
    plain = _record(lambda r, mp: _case_packed_train(r, mp))[:-1]
    got = _record(lambda r, mp: _case_packed_train(r, mp, env="PASST_AMD_NO_DEFER_ROWS"))[:-1]
    deferring = [e for e in plain if e[0] in ("layernorm_bwd", "dgelu_gemm")]
    assert deferring and all(e[2].get("defer") is not None for e in deferring)
    for e in got:
        if e[0] in ("layernorm_bwd", "dgelu_gemm"):
            assert e[2].get("defer") is None
        if e[0] == "wgrad_tn_batched":
            assert e[2]["row_jobs"] is None
    assert [e[0] for e in got] == [e[0] for e in plain]          # the same launches behind the stand-ins: only who reduces changes


if __name__ == "__main__":
    import subprocess
    import sys
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python -m tests.test_sequence_cpu --write")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.run(["git", "log", "-1", "--format=%h %s"], cwd=root, capture_output=True, text=True).stdout.strip()
    with open(FIXTURE) as f:
        fixture = json.load(f)                      # what is recorded stays: only the cases it does not hold are added
    new = [name for name in CASES if name not in fixture["traces"]]
    for name in new:
        fixture["traces"][name] = _record(CASES[name])
    no_rng = [name for name, t in fixture["traces"].items() if t[-1][0] != "rng" and name not in fixture.setdefault("rng", {})]
    for name in no_rng:
        fixture["rng"][name] = _record(CASES[name])[-1]
    if new or no_rng:
        fixture.setdefault("notes_added", []).append(f"Traces {new} and the generator digests of {no_rng} recorded at commit {commit}.")
        with open(FIXTURE, "w") as f:
            json.dump(fixture, f, separators=(",", ":"))
            f.write("\n")
    print(f"added {new}, digests {no_rng} at {commit}")

"""Per-class average precision and ROC-AUC on the device (pa_eval_append / pa_eval_rank, passt_amd.metrics.EvalAccumulator) against
scikit-learn's values stored in tests/golden/eval_metrics.npz and the integer restatement of tests/eval_metrics_cases.py.

Everything goes through the C ABI in guarded buffers: the class-major key / state buffers have a capacity larger than n, their
columns at and past n hold valid positives of score +inf (a read past n changes every count), and sentinels lie in front of and
behind every buffer the kernels write.  Integer outputs are compared with torch.equal; ap and auc within 1e-12 of scikit-learn's
(at most N + 2 f64 operations on terms <= 1 at N <= 1000 stay below 2e-13 on either side).  Measured figures go to
eval_metrics_gpu.json in $PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from tests import eval_metrics_cases as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "ddp_eval_worker.py")
DEV = "cuda"
GUARD = 256                                   # elements in front of and behind every guarded buffer
KEY_INF = int(np.array([0xff800000], np.uint32).view(np.int32)[0])      # score_key(+inf)
_METRICS = {}


def record(name, **kw):
    _METRICS[name] = {k: float(v) for k, v in kw.items()}
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(ROOT, "test_metrics")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "eval_metrics_gpu.json"), "w") as f:
        json.dump(_METRICS, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def inputs():
    return dict(np.load(K.GOLDEN))


class Guarded:
    """`numel` elements between two runs of GUARD sentinel elements"""

    def __init__(self, numel, dtype, sentinel, fill=None):
        self.buf = torch.full((GUARD + numel + GUARD,), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[GUARD:GUARD + numel]
        self.sentinel = sentinel
        if fill is not None:
            self.view.fill_(fill)

    def ptr(self):
        return self.view.data_ptr()

    def take(self, what):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.sentinel).all()), f"{what}: a write in front of the buffer"
        assert bool((b[-GUARD:] == self.sentinel).all()), f"{what}: a write behind the buffer"
        return b[GUARD:-GUARD].clone()


class Columns:
    """The class-major buffers of one fill, through the C ABI."""

    def __init__(self, C, cap):
        self.lib, self.C, self.cap, self.n = _lib.load(), C, cap, 0
        self.st = torch.cuda.current_stream().cuda_stream
        self.keys = Guarded(C * cap, torch.int32, 0x5A5A5A5A, fill=KEY_INF)
        self.state = Guarded(C * cap, torch.uint8, 0xA5, fill=_lib.EVAL_POS)

    def append(self, s, t, m, B, mode=_lib.EVAL_RAW):
        """CPU arrays [n][C] in batches of B (the last one partial)"""
        dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (s, t, m)]
        for b0 in range(0, s.shape[0], B):
            sb, tb, mb = [None if a is None else a[b0:b0 + B].contiguous() for a in dev]
            rc = self.lib.pa_eval_append(sb.data_ptr(), tb.data_ptr(), None if mb is None else mb.data_ptr(), sb.shape[0], self.C, self.n,
                                         self.cap, mode, self.keys.ptr(), self.state.ptr(), self.st)
            assert rc == 0, rc
            self.n += sb.shape[0]
        return self

    def stored(self):
        """(keys uint32 [C][cap], state uint8 [C][cap]) on the CPU after the guard checks; columns at and past n untouched"""
        k = self.keys.take("keys").view(self.C, self.cap).numpy().view(np.uint32)
        s = self.state.take("state").view(self.C, self.cap).numpy()
        assert np.all(k[:, self.n:] == 0xff800000) and np.all(s[:, self.n:] == _lib.EVAL_POS), "a write at or past column n + B"
        return k, s

    def rank(self):
        C = self.C
        need = self.lib.pa_eval_ws_bytes(C, self.cap)
        assert need > 0 and need % 16 == 0
        ws = Guarded(need, torch.uint8, 0xA5)
        ints = [Guarded(C, torch.int64, -77) for _ in range(3)]
        flts = [Guarded(C, torch.float64, -77.0) for _ in range(2)]
        rc = self.lib.pa_eval_rank(self.keys.ptr(), self.state.ptr(), C, self.n, self.cap, ws.ptr(), *[g.ptr() for g in ints + flts], self.st)
        assert rc == 0, (rc, self.lib.pa_last_hip_error())
        ws.take("ws")
        self.stored()
        names = ("n_pos", "n_neg", "auc_num", "ap", "auc")
        return {k: g.take(k) for k, g in zip(names, ints + flts)}


def run(s, t, m, B, mode=_lib.EVAL_RAW, spare=37):
    return Columns(s.shape[1], s.shape[0] + spare).append(s, t, m, B, mode).rank()


def assert_close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    assert err <= 1e-12, (what, err)
    return err


def check(out, s, t, m, ap=None, auc=None, what=""):
    """integers exactly against the restatement; ap / auc against scikit-learn's stored values (or the restatement's)"""
    r = K.restate(s, t, m)
    for k in ("n_pos", "n_neg", "auc_num"):
        assert torch.equal(out[k], torch.from_numpy(r[k])), (what, k, out[k], r[k])
    e1 = assert_close(out["ap"].numpy(), r["ap"] if ap is None else ap, (what, "ap"))
    e2 = assert_close(out["auc"].numpy(), r["auc"] if auc is None else auc, (what, "auc"))
    return max(e1, e2)


def bits(out):
    return torch.cat([out[k].view(torch.int64) for k in ("n_pos", "n_neg", "auc_num", "ap", "auc")])


@pytest.mark.parametrize("C", K.CS)
@pytest.mark.parametrize("n", K.NS)
def test_every_size_and_content_against_scikit_learn(inputs, n, C):
    B, worst = K.batch_size(n, C), 0.0
    for kind in K.KINDS:
        s, t, m = K.case(inputs, kind, n, C)
        ap, auc = K.expected(inputs, kind, n, C)
        out = run(s, t, m, B)
        worst = max(worst, check(out, s, t, m, ap, auc, (kind, n, C, B)))
        # the conventions, spelled out
        P, Nn, bad = out["n_pos"].numpy(), out["n_neg"].numpy(), np.isnan(s).any(0)
        assert np.all(out["ap"].numpy()[(P == 0) & ~bad] == 0.0)
        assert np.all(np.isnan(out["auc"].numpy()[(P == 0) | (Nn == 0) | bad])) and np.all(np.isnan(out["ap"].numpy()[bad]))
    record(f"sizes/n{n}_C{C}_B{B}", max_abs_err_vs_sklearn=worst)


def test_denormal_scores_are_compared_as_integers(inputs):
    """two distinct f32 denormals must not tie, -0 must tie with +0, whatever the kernels' denormal mode"""
    s, t, m = K.case(inputs, "denormal", 257, 3)
    cols = Columns(3, 300).append(s, t, m, 20)
    k, st = cols.stored()
    assert np.array_equal(k[:, :257], K.score_key(s).T)
    assert np.array_equal(st[:, :257], np.where(t.T > 0.5, _lib.EVAL_POS, _lib.EVAL_NEG))
    assert len(np.unique(k[:, :257])) == 7


def test_more_than_one_chunk_of_positives_and_of_negatives():
    s, t, m = K.large_case()
    r = K.restate(s, t, m)
    assert r["n_pos"].min() > 1024 and r["n_neg"].min() > 1024
    record("large/n2600_C3", max_abs_err_vs_restatement=check(run(s, t, m, 64), s, t, m, what="large"))


@pytest.mark.parametrize("kind,n,C", [("ties8", 1000, 20), ("masked", 257, 65), ("dense", 1000, 3)])
def test_repeatable_and_independent_of_the_sample_order(inputs, kind, n, C):
    s, t, m = K.case(inputs, kind, n, C)
    cols = Columns(C, n + 11).append(s, t, m, 20)
    a, b = cols.rank(), cols.rank()
    assert torch.equal(bits(a), bits(b)), "two pa_eval_rank calls on one fill"
    c = run(s, t, m, 20, spare=11)
    assert torch.equal(bits(a), bits(c)), "two fresh fills"
    d = run(s, t, m, 7, spare=90)
    assert torch.equal(bits(a), bits(d)), "another batch size and capacity"
    perm = np.random.Generator(np.random.PCG64(5)).permutation(n)
    p = run(s[perm], t[perm], None if m is None else m[perm], 20)
    for k in ("n_pos", "n_neg", "auc_num"):
        assert torch.equal(a[k], p[k]), k
    assert torch.equal(a["auc"].view(torch.int64), p["auc"].view(torch.int64))       # one division of equal integers
    record(f"permuted/{kind}", ap_max_abs_diff=assert_close(p["ap"].numpy(), a["ap"].numpy(), "permuted ap"))


def test_sigmoid_mode_sweep():
    """Keys non-decreasing in z over [-103, 103]; every score within (2 x torch's worst error + 1) ulp of the float64 sigmoid, torch's
    worst error being measured here, on the same sweep, from torch.sigmoid on CPU f32.  The sweep's far negative end is where the
    exact value is an f32 denormal and both implementations return 0: the figure there is large for both, so the same bound is
    also applied to the part of the sweep whose exact value is a normal f32, with torch's error measured on that part."""
    z = K.sigmoid_sweep()
    n = len(z)
    cols = Columns(1, n + 5).append(z.reshape(n, 1), np.zeros((n, 1), np.float32), None, 64, mode=_lib.EVAL_SIGMOID)
    k, st = cols.stored()
    k = k[0, :n]
    assert np.all(st[0, :n] == _lib.EVAL_NEG)
    assert np.all(np.diff(k.astype(np.int64)) >= 0), "the stored keys decrease somewhere along the sorted sweep"
    got = K.key_score(k)
    assert got[0] == 0.0 and got[-1] == 1.0 and got[z == 0].tolist() == [0.5, 0.5]
    ref = torch.sigmoid(torch.from_numpy(z)).numpy()
    e_ref, e_got = K.ulp_error(ref, z), K.ulp_error(got, z)
    normal = 1.0 / (1.0 + np.exp(-z.astype(np.float64))) >= float(np.finfo(np.float32).tiny)
    fig = dict(torch_cpu_max_ulp=e_ref.max(), kernel_max_ulp=e_got.max(), torch_cpu_max_ulp_normal_range=e_ref[normal].max(),
               kernel_max_ulp_normal_range=e_got[normal].max(), differing_from_torch_cpu=float((ref != got).sum()), sweep=n)
    print("sigmoid sweep:", fig)
    record("sigmoid_sweep", **fig)
    assert e_got.max() <= 2 * e_ref.max() + 1
    assert e_got[normal].max() <= 2 * e_ref[normal].max() + 1


def test_sigmoid_mode_on_the_fixture_logits(inputs):
    """ranking by the kernel's sigmoid == scikit-learn on torch.sigmoid (CPU, f32) of the same logits, in every class whose
    sigmoids agree on all samples; on the fixture's logits that has to be every class"""
    logits, target, _ = K.base(inputs)
    C = K.SIGMOID_C
    s, t = np.ascontiguousarray(logits[:, :C]), np.ascontiguousarray(target[:, :C])
    cols = Columns(C, 1024).append(s, t, None, 20, mode=_lib.EVAL_SIGMOID)
    k, _ = cols.stored()
    got = K.key_score(k[:, :1000]).T
    same = (got == inputs["sigmoid_f32"]).all(0)
    share = 1.0 - same.mean()
    print("sigmoid mode: classes whose sigmoid differs from torch's on some element:", share, "elements:", int((got != inputs["sigmoid_f32"]).sum()))
    record("sigmoid_fixture", share_of_differing_classes=share, differing_elements=float((got != inputs["sigmoid_f32"]).sum()))
    out = cols.rank()
    r = K.restate(inputs["sigmoid_f32"], t)
    for name in ("n_pos", "n_neg"):
        assert torch.equal(out[name], torch.from_numpy(r[name]))
    assert torch.equal(out["auc_num"][torch.from_numpy(same)], torch.from_numpy(r["auc_num"][same]))
    assert_close(out["ap"].numpy()[same], inputs["ap_sigmoid"][same], "ap")
    assert_close(out["auc"].numpy()[same], inputs["auc_sigmoid"][same], "auc")
    assert share == 0.0


# ---- EvalAccumulator ---------------------------------------------------------------------------------------------------------
def _accumulate(acc, s, t, m, B):
    for b0 in range(0, s.shape[0], B):
        acc.update(*[None if a is None else torch.from_numpy(np.ascontiguousarray(a[b0:b0 + B])).to(DEV) for a in (s, t, m)])


def _res_equal(a, b, keys=("n_pos", "n_neg", "auc_num", "ap", "auc", "mAP", "mAUC", "n")):
    for k in keys:
        x, y = a[k].cpu().reshape(-1), b[k].cpu().reshape(-1)
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), k


def test_accumulator_grows_resets_and_keeps_the_validation_loss(inputs):
    from passt_amd.metrics import EvalAccumulator
    s, t, m = K.case(inputs, "masked", 257, 20)
    acc = EvalAccumulator(20, capacity=32)
    empty = acc.compute()                                    # nothing seen yet
    assert int(empty["n"]) == 0 and bool((empty["ap"] == 0).all()) and bool(empty["auc"].isnan().all()) and bool(empty["val_loss"].isnan())
    _accumulate(acc, s, t, m, 20)                            # 32 -> 512 columns: four doublings with earlier columns kept
    assert acc.capacity == 512 and acc.n == 257 and acc.n_batches == 13
    res = acc.compute()
    assert all(v.is_cuda for v in res.values()) and res["ap"].dtype == torch.float64 and res["n_pos"].dtype == torch.int64
    # sigmoid mode on logits within +-8 ranks like scikit-learn on the f32 sigmoid; judged against the restatement of the stored keys
    sig = K.key_score(acc._keys.cpu().numpy().view(np.uint32)[:, :257]).T
    r = K.restate(sig, t, m)
    for k in ("n_pos", "n_neg", "auc_num"):
        assert torch.equal(res[k].cpu(), torch.from_numpy(r[k])), k
    assert_close(res["ap"].cpu().numpy(), r["ap"], "ap")
    assert_close(res["auc"].cpu().numpy(), r["auc"], "auc")
    assert int(res["n"]) == 257
    assert np.isnan(float(res["mAUC"])) == bool(np.isnan(r["auc"]).any()) and abs(float(res["mAP"]) - r["ap"].mean()) < 1e-12
    want = np.mean([float(torch.nn.functional.binary_cross_entropy_with_logits(torch.from_numpy(s[b:b + 20]), torch.from_numpy(t[b:b + 20])))
                    for b in range(0, 257, 20)])
    assert abs(float(res["val_loss"]) - want) < 1e-6, (float(res["val_loss"]), want)
    _res_equal(res, acc.compute())
    acc.reset()
    assert acc.n == 0 and int(acc.compute()["n"]) == 0
    _accumulate(acc, s, t, m, 64)                            # after reset(): the same epoch again, no growth this time
    again = acc.compute()
    _res_equal(res, again)
    assert acc.capacity == 512 and abs(float(again["val_loss"]) - float(torch.nn.functional.binary_cross_entropy_with_logits(
        torch.from_numpy(s[:256]), torch.from_numpy(t[:256]))) * 4 / 5 - float(torch.nn.functional.binary_cross_entropy_with_logits(
            torch.from_numpy(s[256:]), torch.from_numpy(t[256:]))) / 5) < 1e-6


def test_accumulator_raw_scores_match_the_c_abi(inputs):
    from passt_amd.metrics import EvalAccumulator
    s, t, m = K.case(inputs, "ties8", 255, 65)
    acc = EvalAccumulator(65, capacity=64, scores="raw")
    _accumulate(acc, s, t, m, 7)
    res = acc.compute()
    ap, auc = K.expected(inputs, "ties8", 255, 65)
    check({k: v.cpu() for k, v in res.items()}, s, t, m, ap, auc, "accumulator raw")
    assert bool(res["val_loss"].isnan())


def _free_port():
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    return port


def test_two_ranks_equal_one_process_on_the_concatenation(tmp_path):
    """two gloo ranks on the one GPU, holding 150 and 107 samples; both must return exactly what one process returns on all 257"""
    outs = []
    for world in (1, 2):
        port, procs = _free_port(), []
        out = str(tmp_path / f"w{world}")
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                       HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, WORKER, "--out", out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        logs = []
        for p in procs:
            try:
                o, _ = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                raise
            logs.append(o.decode(errors="replace")[-2000:])
        assert all(p.returncode == 0 for p in procs), "\n".join(logs)
        outs.append([torch.load(f"{out}.rank{r}.pt") for r in range(world)])
    (one,), (r0, r1) = outs
    assert int(one["n"]) == 257 and int(r0["n"]) == 257
    _res_equal(one, r0)
    _res_equal(one, r1)
    # the loss is a mean over BATCHES, and the ranks cut the samples into other batches (8 + 6 against 13): the same on both ranks,
    # and near the single process's
    assert float(r0["val_loss"]) == float(r1["val_loss"]) and abs(float(r0["val_loss"]) - float(one["val_loss"])) < 0.05

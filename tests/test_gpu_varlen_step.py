"""GPU tests of ragged batches in the fused training step, ``TrainStep.step(x, y, lengths=)``: the ragged mixup kernel
(pa_mixup_varlen) on the cases of tests/varlen_mixup_cases.py, and the step on top -- against the oracle run clip after clip, against
the drop-in autograd path, from the waveform, with accumulation and clipping, its refusals and its fall-backs.

Model: the depth-2, 768-wide, 256-frame network and the cases of tests/golden/make_varlen_train_golden.py.  Bounds are the project's
own: losses 2e-5 (fp32) / 3e-3 (bf16) and the drop-in comparison's 1e-5 / 2e-4 from tests/test_gpu_model.py, first-step gradients 1e-3
(fp32) / BF16_GRADS (bf16) from tests/test_gpu_varlen_train.py.  Every figure is printed and recorded before it is asserted.
"""
import functools
import math
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import passt_amd  # noqa: E402
from oracle import detgen  # noqa: E402
from oracle import passt_oracle as O  # noqa: E402
from passt_amd import ops  # noqa: E402
from passt_amd._lib import PasstAmdError  # noqa: E402
from tests import varlen_mixup_cases as M  # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_train_golden as VT  # noqa: E402
from tests.test_gpu_model import BF16_GRADS, build, record, rel  # noqa: E402

DEV = "cuda"
ALPHA = 0.3
# chosen on the CPU: under manual_seed(s) and manual_seed(s + 1) randperm(B) is not the identity and pairs some clip with a longer
# and some clip with a shorter partner (asserted below)
STEP_SEEDS = {"a": 4100, "c": 4101}


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
class GpuMixup:
    """the checkers' flat guarded buffers on the device, the views through ops.mixup_varlen(out=)"""

    def mixup_varlen(self, xbuf, x_lo, obuf, o_lo, shape, lens, perm, lam, pad):
        xb, ob = xbuf.to(DEV), obuf.to(DEV)
        n = math.prod(shape)
        x, out = xb[x_lo:x_lo + n].view(shape), ob[o_lo:o_lo + n].view(shape)
        assert ops.mixup_varlen(x, lens.to(DEV), perm.to(DEV), lam.to(DEV), pad, out=out) is out
        torch.cuda.synchronize()
        return xb.cpu(), ob.cpu()

    def mixup(self, x, perm, lam):
        return ops.mixup(x.to(DEV), perm.to(DEV), lam.to(DEV)).cpu()


@pytest.mark.parametrize("case", M.CASES, ids=[c.id for c in M.CASES])
def test_mixup_varlen_kernel(case):
    worst = M.check_case(GpuMixup(), case)
    record(f"mixup_varlen[{case.id}]", error_over_bound=worst)
    print(f"mixup_varlen {case.id}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("case", M.FULL_CASES, ids=[c.id for c in M.FULL_CASES])
def test_mixup_varlen_full_lengths_equal_mixup_bitwise(case):
    M.check_full(GpuMixup(), case)


def test_mixup_varlen_binding():
    """a new tensor for (B, 1, F, T) and (B, F, T); the refusals of the wrapper and of the entry (out == x)"""
    case = M.CASES[0]
    x, lens, perm, lam, pad = M.operands(case)
    want, _ = M.definition(x, lens, perm, lam, pad)
    xd, ld, pd, md = x.to(DEV), lens.to(DEV), perm.to(DEV), lam.to(DEV)
    o3, o4 = ops.mixup_varlen(xd, ld, pd, md, pad), ops.mixup_varlen(xd[:, None], ld, pd, md, pad)
    assert o3.shape == xd.shape and o4.shape == (M.B, 1, case.rows, case.ldt) and o3.data_ptr() != xd.data_ptr()
    assert torch.equal(o3.cpu(), want.float()) and torch.equal(o4[:, 0].cpu(), want.float())
    # lengths outside [0, ldt] are clamped in the kernel
    wild = torch.tensor([-3, case.ldt + 100, 18, 5], dtype=torch.int32)
    o5 = ops.mixup_varlen(torch.nan_to_num(xd, nan=7.0), wild.to(DEV), pd, md, pad).cpu()
    assert bool((o5[0] == 0).all()) and bool(torch.isfinite(o5).all()) and bool((o5[1] != 0).any())
    for bad in (lambda: ops.mixup_varlen(xd, ld, pd, md, pad, out=xd), lambda: ops.mixup_varlen(xd, ld[:3], pd, md, pad),
                lambda: ops.mixup_varlen(xd, ld.long(), pd, md, pad), lambda: ops.mixup_varlen(xd[0], ld, pd, md, pad),
                lambda: ops.mixup_varlen(xd.cpu(), ld, pd, md, pad)):
        with pytest.raises(PasstAmdError):
            bad()
    assert torch.equal(ops.mixup_varlen(xd, ld, pd, md, pad), o3)               # still works after the rejected calls


# ---- helpers of the step tests -------------------------------------------------------------------------------------------------------
def _net(case, precision):
    m = build(case, precision).train()
    m.varlen_train = True
    return m


def _x_nan(case):
    """the case's input with NaN behind every clip's length"""
    x = torch.from_numpy(VT.inputs(case)[0])
    for i, n in enumerate(case["lengths"]):
        x[i, :, :, n:] = float("nan")
    return x


def _targets(case, loss):
    cfg, B = case["cfg"], len(case["lengths"])
    if loss == "ce":
        return np.floor(detgen.uniform(case["seed"], "cls", (B,), 0.0, float(cfg["num_classes"]))).astype(np.int64).clip(0, cfg["num_classes"] - 1)
    return (detgen.uniform(case["seed"], "y", (B, cfg["num_classes"]), 0.0, 1.0) < 0.1).astype(np.float32)


def _mix_by_definition(x, lengths, rn, lam, pad):
    """the mixed ragged batch by the definition, in f32 torch: a list of (1, 1, F, n_i) clips"""
    clips = []
    for i, n in enumerate(lengths):
        j, nj = int(rn[i]), lengths[int(rn[i])]
        c = torch.full((x.shape[2], n), pad, dtype=torch.float32)
        c[:, :min(n, nj)] = x[j, 0, :, :min(n, nj)]
        clips.append((x[i, 0, :, :n] * lam[i] + c * (1.0 - lam[i]))[None, None])
    return clips


def _rng_states():
    s = np.random.get_state()
    return torch.get_rng_state().clone(), (s[0], s[1].copy(), s[2], s[3], s[4])


def _same_states(a, b):
    return torch.equal(a[0], b[0]) and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


# ---- 2. two steps against the oracle -------------------------------------------------------------------------------------------------
LR, WD = 1e-3, 1e-2


@functools.lru_cache(maxsize=None)
def _oracle_two_steps(name, loss):
    """The reference side, once per (case, loss): losses of both steps, every gradient of the first, the generators' final states."""
    from passt_amd.train import MIXUP_PAD
    case = VT.CASES[name]
    cfg, lengths, B = case["cfg"], case["lengths"], len(case["lengths"])
    x, y = torch.from_numpy(VT.inputs(case)[0]), torch.from_numpy(_targets(case, loss))
    sd = O.to_torch(detgen.passt_state_dict(cfg, case["seed"]), requires_grad=True)
    opt = torch.optim.AdamW([v for k, v in sd.items() if not k.startswith("head_dist.")], lr=LR, weight_decay=WD)
    losses, grads, perms = [], None, []
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for step in range(2):
        torch.manual_seed(STEP_SEEDS[name] + step)
        np.random.seed(STEP_SEEDS[name] + step)
        rn, lam = O.my_mixup(B, ALPHA)
        perms.append(rn.tolist())
        clips = _mix_by_definition(x, lengths, rn, lam, MIXUP_PAD)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lo = torch.cat([O.passt_forward(sd, c, cfg, training=True)[0] for c in clips])
        if loss == "bce":
            lv = O.bce_loss(lo, y * lam.reshape(B, 1) + y[rn] * (1.0 - lam.reshape(B, 1)))
        else:
            lv = O.ce_mixup_loss(lo, y, rn, lam)
        opt.zero_grad()
        lv.backward()
        if step == 0:
            grads = {k: v.grad.detach().clone() for k, v in sd.items() if v.grad is not None}
        opt.step()
        losses.append(float(lv.detach()))
    return dict(losses=losses, grads=grads, perms=perms, states=_rng_states())


@pytest.mark.parametrize("loss", ["bce", "ce"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["a", "c"])
def test_ragged_step_two_steps_vs_oracle(name, precision, loss):
    """mel=None, use_mixup=True: two consecutive ragged steps against the oracle run clip after clip on the batch mixed by the
    definition, under torch.optim.AdamW and the same seeds; the step's input has NaN behind every clip.
    Measured on MI355X: loss differences <= 1.7e-6 (fp32) / 1.9e-3 (bf16), worst first-step gradient 1.8e-6 (fp32) / 5.8e-3 (bf16)."""
    from passt_amd.train import TrainStep
    case = VT.CASES[name]
    lengths, B = list(case["lengths"]), len(case["lengths"])
    ref = _oracle_two_steps(name, loss)
    for p in ref["perms"]:              # the seeds show what they are there to show
        assert p != list(range(B)), p
    pairs = [(lengths[i], lengths[j]) for p in ref["perms"] for i, j in enumerate(p)]
    assert any(nj > ni for ni, nj in pairs) and any(nj < ni for ni, nj in pairs), pairs
    net = _net(case, precision)
    ts = TrainStep(net, None, lr=LR, weight_decay=WD, mixup_alpha=ALPHA, use_mixup=True, loss=loss)
    xg, yg = _x_nan(case).to(DEV), torch.from_numpy(_targets(case, loss)).to(DEV)
    losses, w = [], dict(worst_grad=0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(2):
            torch.manual_seed(STEP_SEEDS[name] + step)
            np.random.seed(STEP_SEEDS[name] + step)
            losses.append(float(ts.step(xg, yg, lengths=lengths).item()))
            if step == 0:
                worst_name = None
                for k, g in ts.grads.items():
                    e = rel(g.cpu(), ref["grads"][k])
                    if e > w["worst_grad"]:
                        w["worst_grad"], worst_name = e, k
    states = _rng_states()
    w.update(loss0=abs(losses[0] - ref["losses"][0]), loss1=abs(losses[1] - ref["losses"][1]))
    record(f"varlen_step.{name}[{precision},{loss}]", **w)
    print(f"varlen_step.{name}[{precision},{loss}]: losses {losses} oracle {ref['losses']} {w} (worst gradient: {worst_name})")
    assert all(math.isfinite(v) for v in losses)
    assert ts.t == 2 and set(ts.grads) <= set(ref["grads"])
    assert _same_states(states, ref["states"])                      # the draws of the reference loop, no more, no less
    ltol = 2e-5 if precision == "fp32" else 3e-3
    assert w["loss0"] < ltol and w["loss1"] < ltol, (losses, ref["losses"])
    assert w["worst_grad"] < (1e-3 if precision == "fp32" else BF16_GRADS), (worst_name, w)


# ---- 3. against the drop-in path -----------------------------------------------------------------------------------------------------
def test_ragged_step_matches_the_autograd_path():
    """use_mixup=False, fp32, three steps: net(x, lengths=) + BCE + torch.optim.AdamW against TrainStep.step(x, y, lengths=)."""
    from passt_amd.train import TrainStep
    case = VT.CASES["a"]
    lengths = list(case["lengths"])
    m1, m2 = _net(case, "fp32"), _net(case, "fp32")
    xg, yg = _x_nan(case).to(DEV), torch.from_numpy(_targets(case, "bce")).to(DEV)
    opt = torch.optim.AdamW([p for n, p in m1.named_parameters() if not n.startswith("head_dist")], lr=LR, weight_decay=WD)
    ts = TrainStep(m2, None, lr=LR, weight_decay=WD, use_mixup=False)
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(3):
            torch.manual_seed(50 + step)
            lg, _ = m1(xg, lengths=lengths)
            loss1 = torch.nn.functional.binary_cross_entropy_with_logits(lg, yg, reduction="none").mean()
            opt.zero_grad()
            loss1.backward()
            opt.step()
            state = torch.get_rng_state()
            torch.manual_seed(50 + step)
            loss2 = ts.step(xg, yg, lengths=lengths)
            assert torch.equal(torch.get_rng_state(), state)
            d = abs(loss1.item() - loss2.item())
            worst = max(worst, d)
            print(f"varlen_step.vs_autograd step {step}: losses {loss1.item():.7f} {loss2.item():.7f} diff {d:.2e}")
            assert d < 1e-5, step
    wp = max(rel(p2.detach().cpu(), p1.detach().cpu()) for (_, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()))
    record("varlen_step.vs_autograd[fp32]", loss=worst, params=wp)
    print(f"varlen_step.vs_autograd: worst loss diff {worst:.2e}, worst parameter rel {wp:.2e}")
    assert wp < 2e-4, wp


# ---- 4. from the waveform ------------------------------------------------------------------------------------------------------------
def test_ragged_step_from_the_waveform():
    """TrainStep(net, mel), both in training mode with their switches on: B = 3 clips of 0.5 - 1.5 s.  One step: a finite loss, the
    generators where the documented host sequence leaves them, and the loss of the same pieces called by hand."""
    from passt_amd.train import MIXUP_PAD, TrainStep
    case = VT.CASES["a"]
    samples = [16000, 48000, 30000]
    wave = torch.from_numpy(detgen.uniform(77, "wave", (3, 48000), -0.2, 0.2))
    for i, n in enumerate(samples):
        wave[i, n:] = 0.0
    y = torch.from_numpy((detgen.uniform(77, "y", (3, case["cfg"]["num_classes"]), 0.0, 1.0) < 0.1).astype(np.float32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mel = passt_amd.AugmentMelSTFT(freqm=16, timem=10, fmin_aug_range=10, fmax_aug_range=2000).to(DEV).train()
    mel.varlen_train = True
    wg, yg = wave.to(DEV), y.to(DEV)
    net, net2 = _net(case, "fp32"), _net(case, "fp32")                         # (built ahead of the seeds: construction draws)
    ts = TrainStep(net, mel, lr=LR, weight_decay=WD, mixup_alpha=ALPHA, use_mixup=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(9)
        np.random.seed(9)
        loss = float(ts.step(wg[:, None], yg, lengths=samples).item())          # (B, 1, L_max)
        states = _rng_states()
        # the documented host sequence, with the library's own draw functions
        torch.manual_seed(9)
        np.random.seed(9)
        d = M.host_draws(mel, net2, samples, ALPHA)
        assert _same_states(_rng_states(), states)
        # the same pieces by hand
        torch.manual_seed(9)
        np.random.seed(9)
        spec, frames = mel(wg, lengths=samples)
        assert frames.tolist() == d["frames"] == [50, 150, 94]
        perm = torch.randperm(3)
        lam = np.random.beta(ALPHA, ALPHA, 3).astype(np.float32)
        lam = np.maximum(lam, 1.0 - lam)
        assert torch.equal(perm, d["perm"]) and np.array_equal(lam, d["lam"])
        pd, ld = perm.to(torch.int32).to(DEV), torch.from_numpy(lam).to(DEV)
        xm = ops.mixup_varlen(spec.unsqueeze(1), frames.to(torch.int32).to(DEV), pd, ld, MIXUP_PAD)
        with torch.no_grad():
            lg, _ = net2(xm, lengths=frames)
        hand = float(torch.nn.functional.binary_cross_entropy_with_logits(lg, ops.mixup(yg, pd, ld), reduction="none").mean().item())
        assert _same_states(_rng_states(), states)
    record("varlen_step.wave[fp32]", loss=loss, by_hand=hand, diff=abs(loss - hand))
    print(f"varlen_step.wave: loss {loss:.7f} by hand {hand:.7f} diff {abs(loss - hand):.2e}")
    assert math.isfinite(loss) and ts.t == 1
    assert abs(loss - hand) < 2e-5, (loss, hand)


# ---- 5. accumulation and clipping ----------------------------------------------------------------------------------------------------
def test_ragged_step_accumulation_and_clipping():
    """use_mixup=False, lr=0, clip_grad_norm=1e30: accumulate=2 on the two halves of a ragged batch against accumulate=1 on the whole
    batch, one seed, the clips drawing their Patchout in the same order."""
    from passt_amd.train import TrainStep
    case = VT.CASES["a"]
    lengths = list(case["lengths"])
    xg, yg = _x_nan(case).to(DEV), torch.from_numpy(_targets(case, "bce")).to(DEV)
    kw = dict(lr=0.0, weight_decay=WD, use_mixup=False, clip_grad_norm=1e30)
    whole, halves = TrainStep(_net(case, "fp32"), None, **kw), TrainStep(_net(case, "fp32"), None, accumulate=2, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(61)
        whole.step(xg, yg, lengths=lengths)
        state = torch.get_rng_state()
        torch.manual_seed(61)
        halves.step(xg[:2], yg[:2], lengths=lengths[:2])
        assert halves.t == 0
        halves.step(xg[2:], yg[2:], lengths=lengths[2:])
    torch.cuda.synchronize()
    assert torch.equal(torch.get_rng_state(), state) and whole.t == halves.t == 1
    e = rel(halves.flat_acc.cpu(), whole.flat_g.cpu())
    n1, n2 = float(whole.grad_norm.item()), float(halves.grad_norm.item())
    record("varlen_step.accumulate[fp32]", flat=e, norm_whole=n1, norm_halves=n2)
    print(f"varlen_step.accumulate: flat_acc vs flat_g rel {e:.3e}, grad_norm {n1:.6e} / {n2:.6e}")
    assert e < 1e-3, e
    assert n1 > 0 and abs(n1 - n2) / n1 < 1e-3, (n1, n2)


# ---- 6. refusals and fall-backs ------------------------------------------------------------------------------------------------------
def _small(depth=1, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(img_size=(128, 256), stride=10, num_classes=5, embed_dim=64, depth=depth, num_heads=1, distilled=True, **kw)
    net.precision = "fp32"
    return net.to(DEV).train()


def _refused(ts, exc, match, *args, **kw):
    """the call raises, with both generators and the step's buffers exactly as they were"""
    before = _rng_states()
    bufs = [b.clone() for b in (ts.flat_p, ts.flat_g, ts.m, ts.v)]
    with pytest.raises(exc, match=match):
        ts.step(*args, **kw)
    torch.cuda.synchronize()
    assert _same_states(_rng_states(), before), match
    assert all(torch.equal(a, b) for a, b in zip(bufs, (ts.flat_p, ts.flat_g, ts.m, ts.v))) and ts.t == 0, match


def test_ragged_step_refusals_consume_nothing():
    from passt_amd.train import TrainStep
    x = torch.from_numpy(detgen.uniform(3, "x", (2, 1, 128, 120), -1.5, 1.5)).to(DEV)
    y = torch.zeros(2, 5, device=DEV)
    wave = torch.from_numpy(detgen.uniform(3, "wave", (2, 32000), -0.2, 0.2)).to(DEV)
    torch.manual_seed(1)
    np.random.seed(1)
    # the network's switch
    net = _small(s_patchout_t=2)
    ts = TrainStep(net, None)
    _refused(ts, NotImplementedError, "varlen_train", x, y, lengths=[120, 60])
    net.varlen_train = True
    # the checks of lengths (frames) and the Patchout feasibility of every clip
    _refused(ts, ValueError, "3 entries for a batch of 2", x, y, lengths=[120, 60, 30])
    _refused(ts, ValueError, "1-D integer tensor", x, y, lengths=torch.tensor([120.0, 60.0]))
    _refused(ts, ValueError, "clip 1: length 121 exceeds", x, y, lengths=[120, 121])
    _refused(ts, ValueError, "clip 1: 12 frames are shorter than one patch", x, y, lengths=[120, 12])
    _refused(ts, ValueError, "clip 1: 2 patch columns", x, y, lengths=[120, 26])
    # the front end's switch, and the checks of lengths (samples)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mel = passt_amd.AugmentMelSTFT(freqm=16, timem=10).to(DEV).train()
    tm = TrainStep(_small(s_patchout_t=2), mel)
    tm.net.varlen_train = True
    _refused(tm, NotImplementedError, "mel.varlen_train", wave, y, lengths=[32000, 16000])
    mel.varlen_train = True
    _refused(tm, ValueError, "clip 0: length 32001 exceeds", wave, y, lengths=[32001, 16000])
    _refused(tm, PasstAmdError, "reflect padding", wave, y, lengths=[32000, 500])
    _refused(tm, ValueError, "clip 1: 2 patch columns", wave, y, lengths=[32000, 8320])       # 26 frames, s_patchout_t = 2
    # stochastic depth: the refusal of net(x, lengths=)
    nd = _small(depth=2, drop_path_rate=0.1)            # (the rates rise linearly from 0: the second block's is the active one)
    nd.varlen_train = True
    td = TrainStep(nd, None)
    _refused(td, NotImplementedError, "drop_path_rate", x, y, lengths=[120, 60])
    with pytest.raises(NotImplementedError, match="drop_path_rate") as e1:
        nd(x, lengths=[120, 60])
    with pytest.raises(NotImplementedError) as e2:
        td.step(x, y, lengths=[120, 60])
    assert str(e1.value) == str(e2.value)
    # and a step that passes still runs on each of them
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert math.isfinite(ts.step(x, y, lengths=[120, 60]).item()) and math.isfinite(tm.step(wave, y, lengths=[32000, 16000]).item())
    assert ts.t == tm.t == 1


def test_graph_mode_runs_a_ragged_step_eagerly_and_keeps_its_graph():
    """graph=True: after the graph exists a lengths= step runs the eager sequence and the next fixed-shape step replays the same graph
    -- bit-identical to the eager TrainStep over the whole sequence."""
    from passt_amd.train import TrainStep
    case = dict(G.CASES["model_small_train"], seed=951)
    x, y = G.model_inputs(case)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    ragged = {5: [250, 200, 150]}                       # steps 0-2 eager warm-up, 3 captures, 4 replays, 5 is ragged, 6 replays
    outs = []
    for graph in (False, True):
        net = build(case, "bf16").train()
        net.varlen_train = True
        ts = TrainStep(net, None, lr=1e-3, weight_decay=1e-2, use_mixup=True, graph=graph)
        losses, g_before = [], None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for step in range(7):
                torch.manual_seed(80 + step)
                np.random.seed(80 + step)
                if step in ragged:
                    g_before = ts._g["graph"] if graph else None
                    assert not graph or "graph" in ts._g
                losses.append(ts.step(xg, yg, lengths=ragged.get(step)))
                if step in ragged and graph:
                    assert ts._g["graph"] is g_before and not ts._g["capturing"]
        torch.cuda.synchronize()
        assert ts.t == 7 and (not graph or ts._g["graph"] is g_before)
        outs.append((torch.cat([l.reshape(1) for l in losses]).cpu(), ts.flat_p.clone(), ts.m.clone(), ts.v.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all()) and len(set(outs[0][0].tolist())) == 7


def test_fixed_shape_step_is_untouched_by_ragged_steps_elsewhere():
    """step(x, y) gives bit-identical losses and parameters whether or not a lengths= step was ever taken on another TrainStep"""
    from passt_amd.train import TrainStep
    case = dict(G.CASES["model_small_train"], seed=952)
    x, y = G.model_inputs(case)
    xg, yg = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)

    def fixed_steps():
        ts = TrainStep(build(case, "bf16").train(), None, lr=1e-3, weight_decay=1e-2, use_mixup=True)
        losses = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for step in range(2):
                torch.manual_seed(90 + step)
                np.random.seed(90 + step)
                losses.append(ts.step(xg, yg).item())
        return losses, ts.flat_p.clone()
    l1, p1 = fixed_steps()
    other = build(case, "bf16").train()
    other.varlen_train = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        TrainStep(other, None, lr=1e-3, weight_decay=1e-2, use_mixup=True).step(xg, yg, lengths=[250, 200, 150])
    l2, p2 = fixed_steps()
    assert l1 == l2 and torch.equal(p1, p2)

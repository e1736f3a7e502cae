"""Fixture of the gradient w.r.t. the waveform through the front end: tests/golden/wave_grad.npz, from the real reference
implementation (kkoutini/PaSST, imported read-only through oracle/ref_import.py with the torchaudio stand-ins exactly as
make_golden.gen_frontend_case does; none of its text is here).

In the reference ``AugmentMelSTFT.forward`` is plain torch, so ``wave.requires_grad_()`` is plain autograd.  Every front-end case
runs the reference module on CPU on ``frontend_inputs(case)`` waves that require a gradient, with the loss ``(mel * g).sum()``,
``g = detgen.uniform(seed, "g", mel.shape, -1, 1)``, and records per clip i

    <case>.dwave.<i>          keep(dwave[i]): the first and last EDGE samples (where the reflect padding folds back) and SAMPLE evenly
                              spaced ones; the whole clip when it is not longer than that
    <case>.dwave.<i>.stats    (L2 norm, largest magnitude) of the WHOLE dwave[i], so nothing outside the sample can hide
    <case>.mask               train mode: the drawn (fmin, fmax, fmask_start, fmask_end, tmask_start, tmask_end)

Whole 32 000 ... 80 000-sample gradients of every clip would be 1.7 MB, more than a committed file may hold; the tests therefore check
this library against the fixture on the kept samples and the whole-clip statistics, and against the float64 oracle on EVERY sample
(the oracle itself is checked against this fixture on CPU).

``ragged``: clips of RAGGED_LENS samples; each is run ALONE through the reference at batch 1 (the contract of ``lengths=``), with the
rows of one padded (B, n_mels, T_max) detgen ``g`` cut to the clip's own frames.
``e2e``: reference mel (eval) + reference PaSST (G.SMALL config, frozen, eval), loss as make_input_grad_golden.loss_of.

Waves, upstream gradients and weights are oracle/detgen.py streams: the tests regenerate them instead of storing them.

    python tests/golden/make_wave_grad_golden.py        (CPU, about a minute)
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import detgen, ref_import  # noqa: E402
from oracle import passt_oracle as O   # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_input_grad_golden as IG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EDGE, SAMPLE = 640, 2048
TEN_S_SAMPLE = 8192

# name -> front-end case (make_golden's geometry and seeds; "torch_seed": train mode draws)
CASES = {k: G.FRONTEND_CASES[k] for k in ("frontend_eval", "frontend_eval_10s", "frontend_train", "frontend_esc50")}
# one case per non-default STFT hop of live_frontend.npz (make_golden.STFT_CASES), on make_golden.STFT_LIVE's waves, eval mode
for _kw in G.STFT_CASES:
    if "hopsize" in _kw:
        CASES[f"hop{_kw['hopsize']}"] = dict(G.STFT_LIVE, training=False, kw=dict(G.STFT_LIVE["kw"], **_kw))
RAGGED_LENS = [32000, 9731, 20480, 600]
RAGGED = dict(B=4, L=32000, seed=25, training=False, kw=dict(fmin_aug_range=10, fmax_aug_range=2000))
E2E = dict(B=2, L=80000, seed=26, training=False, kw=dict(fmin_aug_range=10, fmax_aug_range=2000), cfg=O.make_cfg(**G.SMALL), net_seed=57)


def keep_index(n):
    """Indices of a clip's n-sample gradient the fixture keeps."""
    if n <= 2 * EDGE + SAMPLE:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.concatenate([np.arange(EDGE), np.linspace(0, n - 1, SAMPLE).astype(np.int64), np.arange(n - EDGE, n)]))


def upstream(case, shape):
    return detgen.uniform(case["seed"], "g", tuple(shape), -1.0, 1.0)


def frames_of(n, hop=320):
    return 1 + (n - 1) // hop


def e2e_inputs(case):
    cfg, B = case["cfg"], case["B"]
    a = detgen.uniform(case["seed"], "a", (B, cfg["num_classes"]), -1.0, 1.0)
    b = detgen.uniform(case["seed"], "b", (B, cfg["embed_dim"]), -1.0, 1.0)
    return a, b


def _into(out, key, dw, ten_s=False):
    dw = np.ascontiguousarray(dw, np.float32)
    out[key] = G.pin_sample(dw, TEN_S_SAMPLE) if ten_s else dw[keep_index(dw.size)].copy()
    out[key + ".stats"] = np.array([np.linalg.norm(dw.astype(np.float64)), np.abs(dw).max()])


def reference_mel(case):
    _, ref_pre = ref_import.load_reference()
    mel = ref_import.run_silently(ref_pre.AugmentMelSTFT, **case["kw"])
    mel.train(case["training"])
    return mel


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, case in CASES.items():
            mel = reference_mel(case)
            wave = torch.from_numpy(G.frontend_inputs(case)).requires_grad_()
            if "torch_seed" in case:
                torch.manual_seed(case["torch_seed"])
            spec = mel(wave)
            (spec * torch.from_numpy(upstream(case, spec.shape))).sum().backward()
            for i in range(case["B"]):
                _into(out, f"{name}.dwave.{i}", wave.grad[i].numpy(), ten_s=name == "frontend_eval_10s")
            if case["training"]:                              # replay the draws (same seed, same order) so the fixture holds them
                torch.manual_seed(case["torch_seed"])
                kw = dict(O.MEL_DEFAULTS, **case["kw"])
                fmax = O.resolve_fmax(kw["sr"], kw["fmax"], kw["fmax_aug_range"])
                fmin_d = kw["fmin"] + torch.randint(kw["fmin_aug_range"], (1,)).item()
                fmax_d = fmax + kw["fmax_aug_range"] // 2 - torch.randint(kw["fmax_aug_range"], (1,)).item()
                fm = O.draw_mask_params(kw["freqm"], spec.shape[1])
                tm = O.draw_mask_params(kw["timem"], spec.shape[2])
                out[name + ".mask"] = np.array([fmin_d, fmax_d, *fm, *tm], np.float64)
            print(name, tuple(wave.shape), "dwave norm / absmax per clip", [out[f"{name}.dwave.{i}.stats"].tolist() for i in range(case["B"])])

        # ragged: every clip alone at batch 1
        case = RAGGED
        mel = reference_mel(case)
        waves = G.frontend_inputs(case)
        g = upstream(case, (case["B"], 128, frames_of(max(RAGGED_LENS))))
        for i, n in enumerate(RAGGED_LENS):
            w = torch.from_numpy(waves[i:i + 1, :n].copy()).requires_grad_()
            spec = mel(w)
            assert spec.shape[2] == frames_of(n)
            (spec * torch.from_numpy(g[i:i + 1, :, :spec.shape[2]].copy())).sum().backward()
            _into(out, f"ragged.dwave.{i}", w.grad[0].numpy())
        print("ragged", RAGGED_LENS, [out[f"ragged.dwave.{i}.stats"].tolist() for i in range(len(RAGGED_LENS))])

        # end to end: reference mel -> reference PaSST (frozen, eval)
        case = E2E
        mel = reference_mel(case)
        net = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["net_seed"]))
        net.eval()
        net.requires_grad_(False)
        wave = torch.from_numpy(G.frontend_inputs(case)).requires_grad_()
        logits, feat = ref_import.run_silently(net, mel(wave)[:, None])
        a, b = e2e_inputs(case)
        IG.loss_of(logits, feat, torch.from_numpy(a), torch.from_numpy(b)).backward()
        out["e2e.logits"], out["e2e.features"] = logits.detach().numpy(), feat.detach().numpy()
        for i in range(case["B"]):
            _into(out, f"e2e.dwave.{i}", wave.grad[i].numpy())
        print("e2e", [out[f"e2e.dwave.{i}.stats"].tolist() for i in range(case["B"])])
    np.savez_compressed(os.path.join(HERE, "wave_grad.npz"), **out)


if __name__ == "__main__":
    main()

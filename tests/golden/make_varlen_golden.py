"""Fixture of the ragged-batch eval forward: tests/golden/varlen_eval.npz, from the real reference implementation
(kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_golden.py does; none of its text is here).

The reference's answer to clips of different lengths is batch size 1 (ex_fsd50k.py:53-56, the ``variable_eval`` config), so that
is what is recorded: the reference ``PaSST.eval()`` run ONE CLIP AT A TIME on LENGTHS (frames) for two models, and the reference
``AugmentMelSTFT.eval()`` run one waveform at a time on WAVE_LENGTHS (samples).  Weights and inputs are oracle/detgen.py streams,
so the tests regenerate them instead of storing them.

    <model>.logits  (B, n_classes)   <model>.features  (B, D)      row i = clip i alone, cropped to LENGTHS[i]
    mel.<i>         pin_sample(spectrogram of waveform i, MEL_SAMPLE)   mel.<i>.stats = (L2 norm, largest magnitude)
    mel.frames      frames per waveform

The reference accepts every length of both mixes (16 frames = exactly one patch column; 640 samples = 2 frames, just above the
n_fft / 2 limit of the centred reflect padding).

    python tests/golden/make_varlen_golden.py        (CPU, about a minute)
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

HERE = os.path.dirname(os.path.abspath(__file__))

# frames at hop 320 into a 998-frame model (stride 10, patch 16): full length twice, one clip past the positional embedding (cut),
# exactly one patch column, one clip just above it
LENGTHS = [998, 437, 1203, 16, 251, 640, 998, 33]
WAVE_LENGTHS = [320000, 140001, 41234, 5120, 640, 320000]
MODELS = {
    "small": dict(cfg=O.make_cfg(**dict(G.SMALL, img_size=(128, 998))), seed=41),
    "d768": dict(cfg=O.make_cfg(embed_dim=768, depth=2, num_heads=12), seed=42),
}
WAVE_SEED = 43
MEL_KW = dict(fmin_aug_range=10, fmax_aug_range=2000)
MEL_SAMPLE = 16384


def model_input(case):
    """(B, 1, n_mels, max LENGTHS) -- clip i is its first LENGTHS[i] frames."""
    return detgen.uniform(case["seed"], "x", (len(LENGTHS), 1, case["cfg"]["img_size"][0], max(LENGTHS)), -1.5, 1.5)


def wave_input():
    """(B, max WAVE_LENGTHS) -- waveform i is its first WAVE_LENGTHS[i] samples (make_golden.frontend_inputs' signal)."""
    return G.frontend_inputs(dict(seed=WAVE_SEED, B=len(WAVE_LENGTHS), L=max(WAVE_LENGTHS)))


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in MODELS.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.eval()
        x = model_input(case)
        lo, fe = [], []
        for i, n in enumerate(LENGTHS):
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                logits, feat = ref_import.run_silently(m, torch.from_numpy(np.ascontiguousarray(x[i:i + 1, :, :, :n])))
            lo.append(logits.numpy()[0])
            fe.append(feat.numpy()[0])
        out[name + ".logits"], out[name + ".features"] = np.stack(lo), np.stack(fe)
        print(name, "logits absmax", float(np.abs(out[name + ".logits"]).max()))
    _, ref_pre = ref_import.load_reference()
    mel = ref_import.run_silently(ref_pre.AugmentMelSTFT, **MEL_KW)
    mel.eval()
    w = wave_input()
    frames = []
    for i, n in enumerate(WAVE_LENGTHS):
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = mel(torch.from_numpy(np.ascontiguousarray(w[i:i + 1, :n])))[0].numpy()
        frames.append(spec.shape[-1])
        G._pinned_into(out, f"mel.{i}", spec, MEL_SAMPLE)
        print("mel", i, spec.shape)
    out["mel.frames"] = np.array(frames, np.int64)
    np.savez_compressed(os.path.join(HERE, "varlen_eval.npz"), **out)


if __name__ == "__main__":
    main()

"""Fixture of the training-mode front end on a ragged batch: tests/golden/varlen_mel_train.npz, from the real reference implementation
(kkoutini/PaSST, imported read-only through oracle/ref_import.py with the torchaudio stand-ins exactly as make_golden.py does; none of
its text is here).

The reference's answer to clips of different lengths is batch size 1, so that is what is recorded: the reference
``AugmentMelSTFT(**MEL_KW).train()`` run on CPU ONE CLIP AFTER THE OTHER under one ``torch.manual_seed(TORCH_SEED)``, on the first
LENGTHS[i] samples of row i of ``wave_input()``, with the loss ``(mel * g).sum()``, ``g`` = the clip's own frames of row i of
``upstream()``.  Every clip therefore has its own fmin / fmax jitter, its own frequency band and its own time band, the latter drawn
against its own frame count.  Per clip i:

    draw.<i>            (fmin, fmax, fmask_start, fmask_end, tmask_start, tmask_end) -- the reference's draws, replayed from the
                        generator state in front of the clip with the same calls in the same order (the replay must end in the
                        state the reference left, or the generator stops)
    mel.<i>             pin_sample(spectrogram of clip i, MEL_SAMPLE)      mel.<i>.stats = (L2 norm, largest magnitude)
    dwave.<i>           make_wave_grad_golden.keep_index samples of dwave  dwave.<i>.stats = (L2 norm, largest magnitude) of all of it
    frames              frames per clip            rng = the generator state behind the last clip

LENGTHS: 48000 (several backward workgroups), 5120 (exactly 16 frames = one full tile of the forward), 20001 (ends in the middle of a
tile), 640 (2 frames: the time band's start can be negative and the band can cover the clip), 48000 again.  TORCH_SEED is chosen so
that the reference's own draws make the fixture worth having; ``check_draws`` states what that means and stops the generator otherwise.
Waves and upstream gradients are oracle/detgen.py streams: the tests regenerate them instead of storing them.

    python tests/golden/make_varlen_mel_train_golden.py        (CPU, seconds)
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
from tests.golden import make_wave_grad_golden as WG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

LENGTHS = [48000, 5120, 20001, 640, 48000]
MEL_KW = dict(freqm=24, timem=40, fmin_aug_range=10, fmax_aug_range=2000)
WAVE_SEED = 47
TORCH_SEED = 14
MEL_SAMPLE = 16384
N_MELS, HOP = 128, 320


def frames_of(n):
    return 1 + (n - 1) // HOP


def wave_input():
    """(B, max LENGTHS) -- clip i is its first LENGTHS[i] samples (make_golden.frontend_inputs' signal)."""
    return G.frontend_inputs(dict(seed=WAVE_SEED, B=len(LENGTHS), L=max(LENGTHS)))


def upstream():
    """(B, n_mels, T_max) upstream gradient -- clip i uses its first frames_of(LENGTHS[i]) columns."""
    return detgen.uniform(WAVE_SEED, "g", (len(LENGTHS), N_MELS, frames_of(max(LENGTHS))), -1.0, 1.0)


def masked_cells(draw, T):
    """(n_mels, T) bool: the cells of a clip of T frames its two bands cover"""
    _, _, fs, fe, ts, te = (int(v) for v in draw)
    m = np.zeros((N_MELS, T), bool)
    m[max(fs, 0):max(fe, 0), :] = True
    m[:, max(ts, 0):max(te, 0)] = True
    return m


def check_draws(draws):
    """What makes the fixture meaningful; ``draws``: one (fmin, fmax, fs, fe, ts, te) per clip."""
    d = np.asarray(draws, np.float64)
    assert len(set(d[:, 1])) >= 2, "no two clips differ in fmax"
    assert len(set(map(tuple, d[:, 2:4]))) >= 2 and len(set(map(tuple, d[:, 4:6]))) >= 2, "no two clips differ in a mask"
    inside = [0 < fs < fe < N_MELS and 0 < ts < te < frames_of(n) for (_, _, fs, fe, ts, te), n in zip(d, LENGTHS)]
    assert any(inside), "no clip has a non-empty frequency band and a non-empty time band strictly inside it"
    for row, n in zip(d, LENGTHS):
        if frames_of(n) > 2:
            assert masked_cells(row, frames_of(n)).mean() <= 0.5, f"the {n}-sample clip has more than half of its cells masked"


def replay_draws(T):
    """The draws of one reference forward in training mode on a clip of T frames: the reference's calls in its order."""
    kw = dict(O.MEL_DEFAULTS, **MEL_KW)
    fmax = O.resolve_fmax(kw["sr"], kw["fmax"], kw["fmax_aug_range"])
    fmin_d = kw["fmin"] + torch.randint(kw["fmin_aug_range"], (1,)).item()
    fmax_d = fmax + kw["fmax_aug_range"] // 2 - torch.randint(kw["fmax_aug_range"], (1,)).item()
    fm = O.draw_mask_params(kw["freqm"], N_MELS)
    tm = O.draw_mask_params(kw["timem"], T)
    return [fmin_d, fmax_d, *fm, *tm]


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    _, ref_pre = ref_import.load_reference()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mel = ref_import.run_silently(ref_pre.AugmentMelSTFT, **MEL_KW)
    mel.train()
    waves, g = wave_input(), upstream()
    out, draws = {}, []
    torch.manual_seed(TORCH_SEED)
    for i, n in enumerate(LENGTHS):
        before = torch.get_rng_state()
        w = torch.from_numpy(waves[i:i + 1, :n].copy()).requires_grad_()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spec = mel(w)
        assert spec.shape == (1, N_MELS, frames_of(n))
        (spec * torch.from_numpy(g[i:i + 1, :, :spec.shape[2]].copy())).sum().backward()
        after = torch.get_rng_state()
        torch.set_rng_state(before)
        draws.append(replay_draws(spec.shape[2]))
        assert torch.equal(torch.get_rng_state(), after), "the replay does not consume what the reference consumed"
        spec = spec.detach().numpy()[0]
        # the replayed bands are the cells the reference set to the mask constant
        assert np.all(np.abs(spec[masked_cells(draws[-1], spec.shape[1])] - 0.9) < 1e-7), i
        out[f"draw.{i}"] = np.array(draws[-1], np.float64)
        G._pinned_into(out, f"mel.{i}", spec, MEL_SAMPLE)
        WG._into(out, f"dwave.{i}", w.grad[0].numpy())
        print(i, n, spec.shape, draws[-1], "masked", float(masked_cells(draws[-1], spec.shape[1]).mean()))
    check_draws(draws)
    out["frames"] = np.array([frames_of(n) for n in LENGTHS], np.int64)
    out["rng"] = torch.get_rng_state().numpy()
    np.savez_compressed(os.path.join(HERE, "varlen_mel_train.npz"), **out)


if __name__ == "__main__":
    main()

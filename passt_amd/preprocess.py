"""AugmentMelSTFT on MI355X: drop-in for the reference's ``models/preprocess.py``.

Same constructor kwargs, buffers (non-persistent => empty ``state_dict``), RNG consumption order
and ``forward(x: (B, L)) -> (B, n_mels, 1 + (L-1)//hop)`` as the reference class
(models/preprocess.py:19-86).  The whole chain -- pre-emphasis, STFT, power, kaldi mel filterbank,
log, SpecAugment masks, normalisation -- is ONE fused HIP kernel (pa_mel_frontend_fwd); the host only
draws the random numbers (same torch CPU RNG calls, same order) and passes five scalars.
"""
import math

import torch
import torch.nn as nn

from . import ops
from ._lib import MelClipParams, MelParams, PasstAmdError, compile_opaque


class _MelWaveGrad(torch.autograd.Function):
    """The forward launch with a gradient w.r.t. the waveform (pa_mel_frontend_bwd / _bwd_varlen).  Only entered when autograd
    records and the waveform requires a gradient; the forward launches exactly what the plain call launches and saves no
    activation: the node keeps the float waveform and the MelParams the launch used (the jittered fmin / fmax and the drawn masks,
    so the backward sees the forward's draw) -- for a ragged training batch the per-clip table on the device as well -- and the
    backward recomputes the spectrum from the waveform."""

    @staticmethod
    def forward(ctx, x, window, bin_mel, twiddle, p, lens_dev, clip_dev):
        ctx.c = (x, window, bin_mel, twiddle, p, lens_dev, clip_dev)
        return ops.mel_forward(x, (window, bin_mel, twiddle), p, lens_dev, clip_dev, fill=0.0)

    @staticmethod
    @torch.autograd.function.once_differentiable          # create_graph=True is not supported: the gradient is a plain tensor
    def backward(ctx, g):
        c, ctx.c = ctx.c, None
        if c is None:
            raise RuntimeError("passt_amd.AugmentMelSTFT: the saved waveform of this forward was already consumed by a backward "
                               "pass (retain_graph / double backward are not supported: run the forward again)")
        x, window, bin_mel, twiddle, p, lens_dev, clip_dev = c
        dx = ops.mel_backward(x, (window, bin_mel, twiddle), p, g.contiguous().float(), lens_dev, clip_dev)
        return dx, None, None, None, None, None, None


def _draw_mask(mask_param, size):
    """The band [start, end) torchaudio.functional.mask_along_axis draws (0.13.1 with the transforms' default p = 1.0 --
    ``_get_mask_param`` leaves mask_param unclamped there -- and 0.11.0, which has no clamp at all; non-iid path, because the
    reference hands the transforms a 3-D tensor: SURVEY.md App. A.4).  Two CPU ``torch.rand(1)`` draws; for an axis shorter
    than mask_param the start can be negative and the band can cover the whole axis, as in torchaudio."""
    if mask_param < 1:
        return 0, 0
    value = torch.rand(1) * mask_param
    min_value = torch.rand(1) * (size - value)
    start = int(min_value.long())
    return start, start + int(value.long())


class _AxisMasking(nn.Module):
    """What ``self.freqm`` / ``self.timem`` are in the reference (models/preprocess.py:47-54: torchaudio.transforms.
    FrequencyMasking / TimeMasking(param, iid_masks=True), nn.Identity for 0): parameter-free modules carrying
    ``mask_param`` / ``axis`` / ``iid_masks``, so ``print(mel)``, ``mel.freqm.mask_param`` and ``isinstance(mel.freqm,
    nn.Identity)`` read as they do there.  The masking itself is a predicate inside the fused front-end kernel; the module
    only holds the draw (``draw(size)``), called by AugmentMelSTFT.forward in the reference's order."""

    def __init__(self, mask_param, axis, iid_masks):
        super().__init__()
        self.mask_param, self.axis, self.iid_masks, self.p = int(mask_param), axis, iid_masks, 1.0

    def draw(self, size):
        return _draw_mask(self.mask_param, size)

    def forward(self, specgram, mask_value=0.0):
        raise PasstAmdError("the SpecAugment masks are applied inside pa_mel_frontend_fwd (AugmentMelSTFT.forward); this module "
                            "only carries mask_param")


class FrequencyMasking(_AxisMasking):
    def __init__(self, freq_mask_param, iid_masks=False):
        super().__init__(freq_mask_param, 1, iid_masks)


class TimeMasking(_AxisMasking):
    def __init__(self, time_mask_param, iid_masks=False):
        super().__init__(time_mask_param, 2, iid_masks)


def checked_lengths(mel, lengths, B=None, L=None):
    """``lengths`` of ``forward(x, lengths=)`` as a list of ints, after every check the ragged call makes (``B``, ``L``: rows and
    samples per row of the batch, None = not known).  Pure host code; raises before any random number is drawn."""
    if torch.is_tensor(lengths):
        if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError("lengths must be a sequence of ints or a 1-D integer tensor")
        lengths = lengths.tolist()
    lengths = [int(v) for v in lengths]
    if B is not None and len(lengths) != B:
        raise ValueError(f"lengths has {len(lengths)} entries for a batch of {B} waveforms")
    for i, n in enumerate(lengths):
        if L is not None and n > L:
            raise ValueError(f"clip {i}: length {n} exceeds the batch's {L} samples")
        if n - 1 <= mel.n_fft // 2:
            raise PasstAmdError(f"pa_mel_frontend_fwd_varlen failed: unsupported configuration: clip {i} has {n} samples; the "
                                f"centred reflect padding needs more than {mel.n_fft // 2 + 1} (torch.stft rule)")
    return lengths


def varlen_clip_draws(mel, lengths, B=None, L=None):
    """The training-mode draws of a ragged batch, clip after clip in the order the reference consumes the CPU generator when it
    processes the clips one at a time (models/preprocess.py:63-64, 80-82): per clip ``randint(fmin_aug_range)``,
    ``randint(fmax_aug_range)``, two ``rand(1)`` for the frequency band (if ``freqm``), two ``rand(1)`` for the time band (if
    ``timem``) -- the time band against the clip's OWN frame count.  ``torch.manual_seed(s)`` + this function therefore leaves the
    generator where ``torch.manual_seed(s)`` + the batch-1 loop leaves it.  Pure host code (``mel`` is an AugmentMelSTFT on any
    device); every check of ``lengths`` runs before the first draw.

    Returns a dict: ``frames`` (B,), ``fmin`` / ``fmax`` (B,), ``fmask`` / ``tmask`` (B, 2) [start, end) and ``table``, the
    ``pa_mel_clip_params[B]`` (ctypes array of MelClipParams) the kernels read."""
    lengths = checked_lengths(mel, lengths, B, L)
    frames = [1 + (n - 1) // mel.hopsize for n in lengths]
    table = (MelClipParams * len(lengths))()
    fmins, fmaxs, fmask, tmask = [], [], [], []
    for c, T in zip(table, frames):
        fmin = mel.fmin + torch.randint(mel.fmin_aug_range, (1,)).item()                                  # :63
        fmax = mel.fmax + mel.fmax_aug_range // 2 - torch.randint(mel.fmax_aug_range, (1,)).item()        # :64
        fm = mel.freqm.draw(mel.n_mels) if isinstance(mel.freqm, _AxisMasking) else (0, 0)                # :81
        tm = mel.timem.draw(T) if isinstance(mel.timem, _AxisMasking) else (0, 0)                         # :82
        mel_low = 1127.0 * math.log(1.0 + fmin / 700.0)
        mel_high = 1127.0 * math.log(1.0 + fmax / 700.0)
        c.mel_low, c.inv_mel_delta = mel_low, (mel.n_mels + 1) / (mel_high - mel_low)
        (c.fmask_start, c.fmask_end), (c.tmask_start, c.tmask_end) = fm, tm
        fmins.append(fmin), fmaxs.append(fmax), fmask.append(fm), tmask.append(tm)
    return dict(frames=frames, fmin=fmins, fmax=fmaxs, fmask=fmask, tmask=tmask, table=table)


class AugmentMelSTFT(nn.Module):
    def __init__(self, n_mels=128, sr=32000, win_length=800, hopsize=320, n_fft=1024, freqm=48, timem=192,
                 htk=False, fmin=0.0, fmax=None, norm=1, fmin_aug_range=1, fmax_aug_range=1000):
        torch.nn.Module.__init__(self)
        self.win_length, self.n_mels, self.n_fft, self.sr, self.htk, self.fmin = win_length, n_mels, n_fft, sr, htk, fmin
        if fmax is None:
            fmax = sr // 2 - fmax_aug_range // 2
            print(f"Warning: FMAX is None setting to {fmax} ")
        self.fmax, self.norm, self.hopsize = fmax, norm, hopsize
        self.register_buffer('window', torch.hann_window(win_length, periodic=False), persistent=False)
        assert fmin_aug_range >= 1, f"fmin_aug_range={fmin_aug_range} should be >=1; 1 means no augmentation"
        assert fmax_aug_range >= 1, f"fmax_aug_range={fmax_aug_range} should be >=1; 1 means no augmentation"
        self.fmin_aug_range, self.fmax_aug_range = fmin_aug_range, fmax_aug_range
        self.register_buffer("preemphasis_coefficient", torch.as_tensor([[[-.97, 1]]]), persistent=False)
        self.freqm = nn.Identity() if freqm == 0 else FrequencyMasking(freqm, iid_masks=True)      # :47-50
        self.timem = nn.Identity() if timem == 0 else TimeMasking(timem, iid_masks=True)           # :51-54
        # constant tables of the fused kernel (f64 -> f32), non-persistent like the reference buffers
        left = (n_fft - win_length) // 2
        wpad = torch.zeros(n_fft)
        wpad[left:left + win_length] = self.window                      # torch.stft centres the window
        k = torch.arange(n_fft // 2, dtype=torch.float64)
        bin_mel = 1127.0 * torch.log1p(k * (sr / n_fft) / 700.0)         # kaldi mel of FFT bin k
        ang = 2.0 * math.pi * k / n_fft
        tw = torch.stack([torch.cos(ang), -torch.sin(ang)], dim=1)
        self.register_buffer("_window_padded", wpad, persistent=False)
        self.register_buffer("_bin_mel", bin_mel.float(), persistent=False)
        self.register_buffer("_twiddle", tw.float().contiguous(), persistent=False)
        self.varlen_train = False       # True: train mode accepts lengths= (every clip its own jitter and masks, see forward)

    def _params(self, fmin, fmax, n_frames):
        """The MelParams of one launch: the filterbank between ``fmin`` and ``fmax``, ``n_frames`` output columns, no mask bands."""
        p = MelParams()
        p.n_fft, p.hop, p.n_mels, p.n_frames = self.n_fft, self.hopsize, self.n_mels, n_frames
        p.preemph = 0.97
        mel_low = 1127.0 * math.log(1.0 + fmin / 700.0)
        mel_high = 1127.0 * math.log(1.0 + fmax / 700.0)
        p.mel_low = mel_low
        p.inv_mel_delta = (self.n_mels + 1) / (mel_high - mel_low)
        p.log_eps, p.out_add, p.out_scale = 0.00001, 4.5, 1.0 / 5.0
        p.fmask_start = p.fmask_end = p.tmask_start = p.tmask_end = 0
        return p

    @compile_opaque                 # ONE opaque eager call under torch.compile, like PaSST.forward
    def forward(self, x, lengths=None):
        """x: (B, L) waveforms -> (B, n_mels, 1 + (L-1)//hop).

        A waveform that requires a gradient gets one (train and eval mode, with and without ``lengths``): masked cells and the
        frames behind a clip's end contribute nothing, samples behind ``lengths[i]`` get exactly 0.  One backward per forward;
        ``create_graph=True`` is not supported.

        ``lengths`` (sequence of ints or 1-D integer tensor): valid samples per row of a zero-padded batch of clips of different
        lengths (left-aligned).  Returns ``(spec, frames)``: spec (B, n_mels, T_max), T_max = frames of the longest clip, row i equal
        to ``forward(x[i:i+1, :lengths[i]])`` in its first frames[i] columns (pre-emphasis and reflect padding at the clip's own
        end; samples behind lengths[i] are never read) and exactly 0.0 behind them; ``frames``: int64 CPU tensor, ready for
        ``PaSST.forward(spec[:, None], lengths=frames)``.  A device tensor of lengths costs one host read.

        ``lengths`` in train mode needs ``self.varlen_train = True`` (off by default: NotImplementedError).  Every clip then gets what
        ``self.train()(x[i:i+1, :lengths[i]])`` gives it alone: its own fmin / fmax jitter, its own frequency band and its own time
        band, drawn against its own frames[i]; the CPU generator is consumed clip after clip in the reference's order
        (``varlen_clip_draws``), so the same seed in front of this call and in front of the batch-1 loop gives the same draws and the
        same final generator state.  Masked cells hold 0.9, the columns behind a clip's frames exactly 0.0.  Eval mode ignores the
        switch (two ``randint`` per call, no masks)."""
        if lengths is not None:
            return self._forward_varlen(x, lengths)
        if not x.is_cuda:
            raise PasstAmdError("passt_amd.AugmentMelSTFT runs on a HIP device only (no CPU fallback)")
        if x.dim() != 2:
            raise ValueError("expected (batch, samples)")
        x = x.contiguous().float()                  # outside the autograd node: autograd casts the gradient back to x's dtype / layout
        B, L = x.shape
        # RNG order of the reference: both randint calls always execute (:63-64)
        fmin = self.fmin + torch.randint(self.fmin_aug_range, (1,)).item()
        fmax = self.fmax + self.fmax_aug_range // 2 - torch.randint(self.fmax_aug_range, (1,)).item()
        if not self.training:
            fmin, fmax = self.fmin, self.fmax
        p = self._params(fmin, fmax, 1 + (L - 1) // self.hopsize)
        if self.training:
            if isinstance(self.freqm, _AxisMasking):
                p.fmask_start, p.fmask_end = self.freqm.draw(self.n_mels)                 # :81
            if isinstance(self.timem, _AxisMasking):
                p.tmask_start, p.tmask_end = self.timem.draw(p.n_frames)                  # :82
        if torch.is_grad_enabled() and x.requires_grad:
            return _MelWaveGrad.apply(x, self._window_padded, self._bin_mel, self._twiddle, p, None, None)
        return ops.mel_frontend(x, self._window_padded, self._bin_mel, self._twiddle, p)

    def _forward_varlen(self, x, lengths):
        if self.training and not self.varlen_train:
            raise NotImplementedError("AugmentMelSTFT.forward(x, lengths=...) in train mode needs the switch varlen_train = True (every "
                                      "clip then gets its own fmin / fmax jitter and its own frequency / time masks, as if it were "
                                      "processed alone); it is off by default")
        if not x.is_cuda:
            raise PasstAmdError("passt_amd.AugmentMelSTFT runs on a HIP device only (no CPU fallback)")
        if x.dim() != 2:
            raise ValueError("expected (batch, samples)")
        lengths = checked_lengths(self, lengths, *x.shape)
        x = x.contiguous().float()
        clip_dev = None
        if self.training:
            # every clip its own draws, in the order of the batch-1 loop; the kernel reads them from the table, not from p
            draws = varlen_clip_draws(self, lengths)
            frames = draws["frames"]
            clip_dev = ops.upload_mel_clips(draws["table"], x.device)
        else:
            # RNG order of the reference: both randint calls always execute (:63-64), once per call here
            torch.randint(self.fmin_aug_range, (1,))
            torch.randint(self.fmax_aug_range, (1,))
            frames = [1 + (n - 1) // self.hopsize for n in lengths]
        p = self._params(self.fmin, self.fmax, max(frames))
        lens_dev = ops.upload_small(torch.tensor(lengths, dtype=torch.int32), x.device)
        tables = (self._window_padded, self._bin_mel, self._twiddle)
        if torch.is_grad_enabled() and x.requires_grad:
            spec = _MelWaveGrad.apply(x, *tables, p, lens_dev, clip_dev)
        else:
            spec = ops.mel_forward(x, tables, p, lens_dev, clip_dev, fill=0.0)
        return spec, torch.tensor(frames, dtype=torch.int64)

    def extra_repr(self):
        return 'winsize={}, hopsize={}'.format(self.win_length, self.hopsize)


try:  # reference: ``model_ing = Ingredient("spectrograms")`` with AugmentMelSTFT as a command (:10,:18)
    from ba3l.ingredients.ingredient import Ingredient  # type: ignore

    model_ing = Ingredient("spectrograms")
    AugmentMelSTFT = model_ing.command(AugmentMelSTFT)
except Exception:
    model_ing = None

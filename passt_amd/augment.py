"""Waveform-side augmentation on the GPU, ahead of the fused front end.

The reference applies these per clip inside DataLoader workers (audioset/dataset.py): device-impulse-response convolution and
gain (``pydub_augment`` :103-112, with ``get_ir_sample`` :84-100), ``pad_or_truncate`` (:73-78), ``roll_func`` (:315-329) and
``MixupDataset`` (:115-140).  Here the loader only hands over raw clips; ``WaveAugment`` draws the same random variables on the
host (same distributions, per clip, in the reference's per-item order: IR decision, IR index on a hit, gain, roll, then mix
decision, partner, beta) and the kernels produce the ``(B, 1, L)`` batch and the mixed targets: ``pa_wave_ir_convolve`` (an
overlap-save FFT convolution, ``scipy.signal.convolve(waveform, ir, 'full')`` cut or padded to L) for the clips an IR was drawn
for, then the kernel pair ``pa_wave_augment`` on its output, so the batch contract ``(waveform (B,1,L) f32, target (B,C) f32)``
of ``ex_audioset.py:155-160`` is unchanged.  One deliberate difference: the mixing partner is another clip of the SAME batch
(the reference indexes the whole dataset); as there, it is the partner's IR-convolved clip that is mixed in.

``IRBank`` holds the impulse responses (already at the clip sample rate: reading ``.wav`` files and resampling stay with the
caller, the reference uses librosa for both) and their spectra, prepared once per device on first use.
"""
import numpy as np
import torch

from . import ops


class IRBank:
    """A bank of device impulse responses for ``WaveAugment(ir_bank=..., ir_augment=p)``.  ``irs``: a sequence of 1-D float
    arrays or tensors (what ``get_ir_sample``'s ``irs_arr`` holds), each of 1..8192 taps."""

    def __init__(self, irs):
        irs = [np.asarray(h.detach().cpu() if torch.is_tensor(h) else h, dtype=np.float32) for h in irs]
        if not irs:
            raise ValueError("IRBank: the bank is empty")
        for i, h in enumerate(irs):
            if h.ndim != 1 or h.size < 1:
                raise ValueError(f"IRBank: impulse response {i} must be a non-empty 1-D array, got shape {h.shape}")
            if h.size > ops.IR_MAX_TAPS:
                raise ValueError(f"IRBank: impulse response {i} has {h.size} taps; at most {ops.IR_MAX_TAPS} are supported: "
                                 f"truncate it (ir[:{ops.IR_MAX_TAPS}]) before building the bank")
        self.ir_len = np.array([h.size for h in irs], np.int32)
        self.max_taps = int(self.ir_len.max())
        self.irs = np.zeros((len(irs), self.max_taps), np.float32)
        for i, h in enumerate(irs):
            self.irs[i, :h.size] = h
        self._prepared = {}

    def __len__(self):
        return len(self.ir_len)

    def spectra(self, device):
        """The bank's ``ops.IRSpectra`` on ``device`` (prepared on first use, then kept)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._prepared:
            self._prepared[device] = ops.ir_bank_prepare(torch.from_numpy(self.irs).to(device), torch.from_numpy(self.ir_len).to(device))
        return self._prepared[device]


class WaveAugment:
    def __init__(self, clip_samples=320000, gain_augment=7, roll_shift_range=50, wavmix_rate=0.5, wavmix_beta=2.0, ir_bank=None,
                 ir_augment=0.0):
        self.L, self.gain_augment = int(clip_samples), int(gain_augment)
        self.roll_shift_range, self.wavmix_rate, self.wavmix_beta = int(roll_shift_range), float(wavmix_rate), wavmix_beta
        self.ir_bank, self.ir_augment = ir_bank, float(ir_augment or 0.0)
        if self.ir_augment > 0 and ir_bank is None:
            raise ValueError("WaveAugment: ir_augment > 0 needs ir_bank=IRBank([...])")
        if ir_bank is not None and not isinstance(ir_bank, IRBank):
            raise ValueError("WaveAugment: ir_bank must be an IRBank")

    def draw(self, B):
        """Host-side random parameters of one batch: (gain_db, shift, partner, lam) as numpy arrays; with ``ir_augment > 0``
        (gain_db, shift, partner, lam, ir_idx), ir_idx[b] = -1 where no IR was drawn."""
        gain_db = np.zeros(B, np.int32)
        shift = np.zeros(B, np.int32)
        partner = np.full(B, -1, np.int32)
        lam = np.ones(B, np.float32)
        ir_idx = np.full(B, -1, np.int32)
        for b in range(B):
            if self.ir_augment and float(torch.rand(1)) < self.ir_augment:                                 # :105
                ir_idx[b] = int(np.random.randint(0, len(self.ir_bank)))                                   # :100
            if self.gain_augment:
                gain_db[b] = int(torch.randint(self.gain_augment * 2, (1,)).item()) - self.gain_augment   # :108
            if self.roll_shift_range:
                shift[b] = int(np.random.randint(-self.roll_shift_range, self.roll_shift_range + 1))       # :323 (inclusive)
        for b in range(B):
            if self.wavmix_rate and float(torch.rand(1)) < self.wavmix_rate:                               # :124
                partner[b] = int(torch.randint(B, (1,)).item())                                            # :126
                lam[b] = np.random.beta(self.wavmix_beta, self.wavmix_beta)                                # :128
        if self.ir_augment:
            return gain_db, shift, partner, lam, ir_idx
        return gain_db, shift, partner, lam

    def __call__(self, raw, target=None, lengths=None, params=None, ragged=False):
        """raw (B, ldx) f32 on the GPU (zero padded rows; ``lengths`` int32 valid samples per row).  ``params``: what ``draw``
        returns, with or without ir_idx.  Returns (wave (B,1,L), mixed target or None).

        ``ragged=True``: nothing is padded.  Clip b keeps ``n_b = min(lengths[b], clip_samples)`` samples and gets what it would
        get alone, the fixed path run with ``clip_samples = n_b``: its roll wraps at n_b, its partner is cut to n_b or continued
        with zeros, rolled by its own shift modulo n_b and centred by its mean over n_b samples (``pa_wave_augment_varlen``).
        Returns (wave (B, 1, max n_b), exactly 0 behind every n_b; mixed target or None; n, the list of the n_b): the arguments of
        ``TrainStep.step(wave, target, lengths=n)`` and ``mel(wave.squeeze(1), lengths=n)``.  ``lengths`` is required and read on
        the host (a sequence of ints, a CPU tensor, or a device tensor, synced once); the draws are ``draw(B)``, unchanged."""
        B = raw.shape[0]
        host, n = self._ragged_lengths(raw, lengths) if ragged else (None, None)     # refusals come before any draw or launch
        params = params if params is not None else self.draw(B)
        gain_db, shift, partner, lam = params[:4]
        ir_idx = np.asarray(params[4], np.int32) if len(params) > 4 else None
        dev = raw.device
        amp = torch.from_numpy((10.0 ** (np.asarray(gain_db, np.float64) / 20.0)).astype(np.float32)).to(dev)
        sh = torch.from_numpy(np.asarray(shift, np.int32)).to(dev)
        pt = torch.from_numpy(np.asarray(partner, np.int32)).to(dev)
        lm = torch.from_numpy(np.asarray(lam, np.float32)).to(dev)
        if ragged:
            lengths = torch.tensor(host, dtype=torch.int32).to(dev)
        elif lengths is not None:
            lengths = lengths.to(device=dev, dtype=torch.int32)
        raw = raw.contiguous().float()
        L = max(n) if ragged else self.L
        if ir_idx is not None and (ir_idx >= 0).any():                         # convolve(waveform, ir, 'full'), :107
            if self.ir_bank is None:
                raise ValueError("WaveAugment: params carry IR indices but no ir_bank was given")
            if int(ir_idx.max()) >= len(self.ir_bank):
                raise ValueError(f"WaveAugment: IR index {int(ir_idx.max())} outside the bank of {len(self.ir_bank)}")
            raw, lengths = ops.wave_ir_convolve(raw, L, lengths, torch.from_numpy(ir_idx).to(dev), self.ir_bank.spectra(dev))
        if ragged:                                                             # an IR's tail is cut at n_b, as at L on the fixed path
            wave = ops.wave_augment_varlen(raw, L, lengths, torch.tensor(n, dtype=torch.int32).to(dev), amp, sh, pt, lm)
        else:
            wave = ops.wave_augment(raw, L, lengths, amp, sh, pt, lm)
        if target is not None:                                                 # y = w y1 + (1 - w) y2, :137
            w = np.where(np.asarray(partner) >= 0, np.maximum(lam, 1.0 - np.asarray(lam)), 1.0).astype(np.float32)
            perm = np.where(np.asarray(partner) >= 0, partner, np.arange(B)).astype(np.int32)
            target = ops.mixup(target.contiguous().float(), torch.from_numpy(perm).to(dev), torch.from_numpy(w).to(dev))
        if ragged:
            return wave.unsqueeze(1), target, n
        return wave.unsqueeze(1), target

    @staticmethod
    def _host_lengths(lengths):
        if torch.is_tensor(lengths):
            return [int(v) for v in lengths.detach().reshape(-1).cpu().tolist()]       # a device tensor: the one sync
        return [int(v) for v in np.asarray(lengths).reshape(-1).tolist()]

    def _ragged_lengths(self, raw, lengths):
        """(lengths on the host, the output lengths n_b) of a ragged call, or ValueError: nothing is drawn, launched or written
        before this returns."""
        if lengths is None:
            raise ValueError("WaveAugment(ragged=True) needs lengths: the valid samples of every clip")
        if raw.dim() != 2:
            raise ValueError(f"WaveAugment(ragged=True): raw must be (B, samples), got shape {tuple(raw.shape)}")
        B, ldx = raw.shape
        host = self._host_lengths(lengths)
        if len(host) != B:
            raise ValueError(f"WaveAugment(ragged=True): lengths holds {len(host)} entries for a batch of {B} clips")
        for b, v in enumerate(host):
            if v < 1:
                raise ValueError(f"WaveAugment(ragged=True): clip {b} has length {v}; every clip needs at least one sample")
            if v > ldx:
                raise ValueError(f"WaveAugment(ragged=True): clip {b} has length {v}, raw holds {ldx} samples per row")
        return host, [min(v, self.L) for v in host]

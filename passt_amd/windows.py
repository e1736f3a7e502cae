"""Tagging long recordings from the waveform: the front end once over the whole recordings, then PaSST.forward_windows.

Windows are cut at the SPECTROGRAM level: the mel front end runs once over every whole recording, and a window is a span of its
frames.  The STFT frames at a window's edge therefore see the neighbouring audio of the recording.  A pipeline that first cuts the
waveform into windows and runs the front end on each piece (hear21passt's scene embeddings do) gives those edge frames a
reflect-padded signal instead, and applies the pre-emphasis filter from the piece's own first sample: its outputs differ from these
in the frames within n_fft / 2 samples of a window edge.  Only the recording's own two ends are reflect-padded here.
"""
from .passt import Windows  # noqa: F401


def seconds_to_frames(mel, seconds):
    """A duration in seconds as frames of the front end ``mel`` (its sample rate over its hop), rounded to the nearest frame."""
    return int(round(float(seconds) * mel.sr / mel.hopsize))


def tag(mel, net, wave, lengths=None, window_s=10.0, hop_s=5.0, **kw):
    """(B, L) waveforms -> ``net.forward_windows``' (logits, features, win), window and hop given in seconds.

    ``mel``: the AugmentMelSTFT front end (eval mode), ``net``: a PaSST or EnsembelerModel (eval mode).  ``lengths``: valid samples
    per waveform (None: all L).  The front end runs ONCE over the whole recordings -- ``mel(wave, lengths=)`` -- and the windows are
    spans of its frames (see the module's note on what that means at a window's edge).  ``window_s`` / ``hop_s`` become frames with
    the front end's own hop (seconds_to_frames).  ``kw`` goes to forward_windows (tail, pool, pool_of, max_tokens).  ``win.start`` /
    ``win.length`` are in frames: frame k starts at sample k * mel.hopsize."""
    if lengths is None:
        lengths = [wave.shape[-1]] * wave.shape[0]
    spec, frames = mel(wave, lengths=lengths)
    return net.forward_windows(spec[:, None], frames, window=seconds_to_frames(mel, window_s), hop=seconds_to_frames(mel, hop_s), **kw)

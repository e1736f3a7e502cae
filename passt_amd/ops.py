"""Tensor-level wrappers over the C ABI (include/passt_amd.h).

Every function takes CUDA(HIP) torch tensors, passes raw device pointers + the current stream to
libpasst_amd.so and returns the output tensors it allocated (torch is the allocator only).
No fallback: a non-CUDA tensor or a missing library raises.
"""
import collections
import ctypes as C
import functools
import math
import threading
import os

import numpy as np
import torch

from . import _lib
from ._lib import (GEMM_BLOCKED_PRE, EPI_DGELU, EPI_GELU, EPI_PARTIAL, EPI_RESID, EPI_STORE, PA_BF16, PA_F32,
                   GemmArgs, MelParams, check)

TORCH_DTYPE = {PA_F32: torch.float32, PA_BF16: torch.bfloat16}
PA_DTYPE = {torch.float32: PA_F32, torch.bfloat16: PA_BF16}


class _CallState(threading.local):
    """Per-thread (the extension is entered from the trainer thread AND the autograd thread): the device of the
    tensors of the C-ABI call being assembled -- set by _p(), consumed by _stream()."""
    dev = None
    gemm_flags = 0      # ambient pa_gemm_args.reserved bits of the model whose kernel sequence this thread is issuing


_call = _CallState()


class gemm_flags:
    """``with ops.gemm_flags(bits):`` -- every pa_gemm_nt call issued by THIS thread inside the block carries ``bits`` in
    pa_gemm_args.reserved (PA_GEMM_NO_PERSIST for a model whose backward shares the CUs with an all-reduce).  Per model and
    per thread, so one data-parallel TrainStep does not change how other models of the process launch their GEMMs."""

    def __init__(self, bits):
        self.bits = int(bits or 0)

    def __enter__(self):
        self.prev, _call.gemm_flags = _call.gemm_flags, self.bits

    def __exit__(self, *exc):
        _call.gemm_flags = self.prev


def _stream():
    """HIP stream the call is ordered on: the current stream OF THE DEVICE THE CALL'S TENSORS LIVE ON (not of
    torch.cuda.current_device(): a model on cuda:1 without set_device must not launch on cuda:0's stream).  Every
    wrapper passes its tensors through _p() first and _stream() last."""
    dev, _call.dev = _call.dev, None
    return torch.cuda.current_stream(dev).cuda_stream


def _p(t, dtype=None, strided=False):
    """Raw device pointer of ``t`` for the C ABI, after the checks the kernels rely on: HIP tensor, the expected
    element type (``dtype``: a torch dtype, PA_F32 / PA_BF16, or None = any), dense rows (contiguous; ``strided`` =
    only the last dimension must be dense, the leading dimension is passed separately) and the same device as the
    other tensors of the call.  The kernels reinterpret memory: a wrong dtype or a strided view would read garbage or
    out of bounds, so this raises instead."""
    if t is None:
        return None
    if not t.is_cuda:
        _call.dev = None
        raise _lib.PasstAmdError("passt_amd kernels need CUDA/HIP tensors (no CPU fallback)")
    if dtype is not None:
        want = TORCH_DTYPE.get(dtype, dtype)
        if t.dtype != want:
            _call.dev = None
            raise _lib.PasstAmdError(f"expected a {want} tensor, got {t.dtype}")
    if not (t.is_contiguous() or (strided and t.dim() >= 1 and (t.shape[-1] <= 1 or t.stride(-1) == 1))):
        _call.dev = None
        raise _lib.PasstAmdError(f"expected a {'row-dense' if strided else 'contiguous'} tensor, got strides {tuple(t.stride())} "
                                 f"for shape {tuple(t.shape)}")
    if _call.dev is None:
        _call.dev = t.device
    elif t.device != _call.dev:
        d0, _call.dev = _call.dev, None
        raise _lib.PasstAmdError(f"tensors of one kernel call live on different devices: {d0} and {t.device}")
    return t.data_ptr()


class _PinnedRing:
    """Small per-step host arrays (Patchout indices, mixup permutation / lambda) reach the device through page-locked
    staging buffers: a copy from pageable memory is a synchronous staging copy that serialises against the communication
    stream in a data-parallel run.  Four slots per (device, dtype, length) rotate; a slot is reused only after the event
    behind its last copy has fired."""

    MAX_RINGS = 32          # distinct (device, dtype, length) rings kept: variable-length uploads must not pin memory without bound

    def __init__(self, slots=4):
        self.slots, self.rings = slots, {}

    def upload(self, host, device):
        host = torch.as_tensor(host)
        key = (str(device), host.dtype, host.numel())
        ring = self.rings.pop(key, None)            # re-inserted below: the dict is kept in least-recently-used order
        if ring is None:
            while len(self.rings) >= self.MAX_RINGS:
                old = self.rings.pop(next(iter(self.rings)))
                for ev in old["ev"]:                # its copies must have left the page-locked buffers before they are freed
                    if ev is not None:
                        ev.synchronize()
            ring = {"i": 0, "buf": [torch.empty(host.numel(), dtype=host.dtype).pin_memory() for _ in range(self.slots)],
                    "ev": [None] * self.slots}
        self.rings[key] = ring
        i = ring["i"]
        ring["i"] = (i + 1) % self.slots
        if ring["ev"][i] is not None:
            ring["ev"][i].synchronize()
        ring["buf"][i].copy_(host.reshape(-1))
        out = ring["buf"][i].to(device, non_blocking=True).view(host.shape)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        ring["ev"][i] = ev
        return out


_pinned = threading.local()


def upload_small(host, device):
    """host (numpy array / CPU tensor) -> device tensor through a pinned staging ring (asynchronous H2D)."""
    ring = getattr(_pinned, "ring", None)
    if ring is None:
        ring = _pinned.ring = _PinnedRing()
    return ring.upload(host, torch.device(device))


# bench.py sets this to a dict to time every GEMM launch with HIP events on the launch stream:
# {epilogue: [(start_event, end_event, algorithmic_flops)]}
GEMM_PROFILE = None
PROFILE_BY_SHAPE = bool(os.environ.get("PASST_AMD_PROFILE_BY_SHAPE"))     # bench.py per_epilogue keyed by (epilogue, M, N, K)
GEMM_TUNE = 0          # pa_gemm_args.tune for every pa_gemm_nt call (0 = library default)
TN_BATCH_ORDER = int(os.environ.get("PASST_AMD_TN_ORDER", "0"))   # 2: problem-major item order (A/B only, see gemm.hip)
# pa_gemm_args.reserved of every pa_gemm_nt call (probe builds: tools/probe_epilogue.py; A/B: PASST_AMD_GEMM_FLAGS=0x1000 =
# _lib.GEMM_EPILOGUE_V3, the LDS-free epilogues)
GEMM_RESERVED = int(os.environ.get("PASST_AMD_GEMM_FLAGS", "0"), 0)
_EPI_NAME = {EPI_STORE: "store", EPI_GELU: "gelu", EPI_RESID: "resid", EPI_DGELU: "dgelu", EPI_PARTIAL: "wgrad_partial"}


def _timed(kind, work, fn):
    """Run fn(); when bench.py profiles this step, bracket it with HIP events on the launch stream and file
    (start, end, work) under `kind` (work = algorithmic FLOPs or bytes of the call)."""
    if GEMM_PROFILE is None:
        return fn()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    r = fn()
    ev1.record()
    GEMM_PROFILE.setdefault(kind, []).append((ev0, ev1, work))
    return r


def kpad(dtype):
    """GEMM K granularity in elements (128 bytes)."""
    return 64 if dtype == PA_BF16 else 32


def round_up(a, b):
    return (a + b - 1) // b * b


def _aligned16(t):
    """Entries that move 16-byte vectors refuse a base pointer off 16-byte alignment (include/passt_amd.h); an offset view gets a copy.
    An aligned tensor -- every tensor torch allocated itself -- passes through: no launch is added."""
    return t.clone() if t is not None and t.is_cuda and t.is_contiguous() and t.data_ptr() % 16 else t


def _into_aligned16(out, make, fill):
    """`fill(dst)` writes an entry's output; a caller's `out` off 16-byte alignment is filled through an aligned temporary"""
    if out.is_cuda and out.data_ptr() % 16:
        tmp = make()
        fill(tmp)
        out.copy_(tmp)
    else:
        fill(out)
    return out


# ---- front end -----------------------------------------------------------------------------
def _mel_wave(wave):
    """The front end takes the alignment of its 16-byte and 8-byte loads from the element index, so the waveform's base pointer must be
    16-byte aligned (include/passt_amd.h); an offset view gets a copy."""
    return wave.clone() if wave.is_cuda and wave.is_contiguous() and wave.data_ptr() % 16 else wave


def _mel_begin(what, wave, lens_dev, clip_dev):
    """Where both directions start.  ``lens_dev`` selects the packed form, ``clip_dev`` (with it) the per-clip form; ``what`` is the
    fixed-length function's name, the messages and the C entry carry the form's suffix.  Returns (what, suffix, aligned wave)."""
    if clip_dev is not None and lens_dev is None:
        raise _lib.PasstAmdError(f"{what}: the per-clip table belongs to the packed form, lens_dev is missing")
    form = ("_varlen" if lens_dev is not None else "") + ("_aug" if clip_dev is not None else "")
    what += form
    wave = _mel_wave(wave)
    if lens_dev is not None and (wave.dim() != 2 or lens_dev.dim() != 1 or lens_dev.numel() != wave.shape[0]):
        raise _lib.PasstAmdError(f"{what}: wave {tuple(wave.shape)} needs one length per row, got {tuple(lens_dev.shape)}")
    B, L = wave.shape
    if clip_dev is not None:
        _mel_clip_table(clip_dev, B, what)
    return what, form, wave


def _mel_launch(kind, work, entry, wave, tables, params, lens_dev, clip_dev, mid):
    """entry(wave, B, pitch, [lens,] window, bin_mel, twiddle, mid()..., params, [clip,] stream), filed under ``kind``"""
    fn = getattr(_lib.load(), entry)
    B, L = wave.shape
    window, bin_mel, twiddle = tables

    def call():               # the arguments in the entry's order: _p() checks them left to right, _stream() comes last
        return check(fn(_p(wave, torch.float32), B, *((L,) if lens_dev is None else (wave.stride(0), _p(lens_dev, torch.int32))),
                        _p(window, torch.float32), _p(bin_mel, torch.float32), _p(twiddle, torch.float32), *mid(), C.byref(params),
                        *(() if clip_dev is None else (_p(clip_dev, torch.uint8),)), _stream()), entry)
    _timed(kind, work, call)


def mel_forward(wave, tables, params: MelParams, lens_dev=None, clip_dev=None, fill=0.0):
    """mel_frontend, mel_frontend_varlen (with ``lens_dev``) or mel_frontend_varlen_aug (with ``clip_dev`` as well); ``tables`` is
    (window, bin_mel, twiddle)."""
    _, form, wave = _mel_begin("mel_frontend", wave, lens_dev, clip_dev)
    out = torch.empty((wave.shape[0], params.n_mels, params.n_frames), device=wave.device, dtype=torch.float32)
    packed = () if lens_dev is None else (params.n_frames, float(fill))
    _mel_launch("mel", 4.0 * (wave.numel() + out.numel()), "pa_mel_frontend_fwd" + form, wave, tables, params, lens_dev, clip_dev,
                lambda: (_p(out),) + packed)
    return out


def mel_backward(wave, tables, params: MelParams, dout, lens_dev=None, clip_dev=None):
    """mel_frontend_bwd, mel_frontend_bwd_varlen or mel_frontend_bwd_varlen_aug, chosen as in mel_forward."""
    what, form, wave = _mel_begin("mel_frontend_bwd", wave, lens_dev, clip_dev)
    B = wave.shape[0]
    if tuple(dout.shape) != (B, params.n_mels, params.n_frames):
        raise _lib.PasstAmdError(f"{what}: dout {tuple(dout.shape)} for a ({B}, {params.n_mels}, {params.n_frames}) output")
    dwave = torch.empty_like(wave)
    packed = () if lens_dev is None else (params.n_frames,)
    _mel_launch("mel_bwd", 4.0 * (2 * wave.numel() + dout.numel()), "pa_mel_frontend_bwd" + form, wave, tables, params, lens_dev, clip_dev,
                lambda: (_p(dout, torch.float32),) + packed + (_p(dwave), None, 0))
    return dwave


def mel_frontend(wave, window, bin_mel, twiddle, params: MelParams):
    return mel_forward(wave, (window, bin_mel, twiddle), params)


def mel_frontend_varlen(wave, lens_dev, window, bin_mel, twiddle, params: MelParams, fill=0.0):
    """Ragged batch: wave (B, L_max) f32 with clips left-aligned, lens_dev (B,) int32 on the device (valid samples per row; the
    caller has checked 1 + n_fft/2 < len <= L_max on the host).  Returns (B, n_mels, params.n_frames); the frames behind a clip's
    own end hold ``fill``."""
    return mel_forward(wave, (window, bin_mel, twiddle), params, lens_dev, fill=fill)


def mel_frontend_bwd(wave, window, bin_mel, twiddle, params: MelParams, dout):
    """Gradient of mel_frontend w.r.t. ``wave`` (B, L) f32 for the upstream gradient ``dout`` (B, n_mels, n_frames) f32; ``params`` is
    the forward call's (mask ranges included).  Nothing was saved: the spectrum is recomputed from the wave.  Deterministic."""
    return mel_backward(wave, (window, bin_mel, twiddle), params, dout)


def mel_frontend_bwd_varlen(wave, lens_dev, window, bin_mel, twiddle, params: MelParams, dout):
    """Gradient of mel_frontend_varlen w.r.t. ``wave`` (B, L_max): row i equals the clip's own gradient in its first lens[i] samples and
    is exactly 0 behind them; ``dout`` behind a clip's frames is not used."""
    return mel_backward(wave, (window, bin_mel, twiddle), params, dout, lens_dev)


def upload_mel_clips(clips, device):
    """The per-clip table of the ragged training front end -- a (B, 6) float64 / int array-like or a ctypes array of MelClipParams, one
    row (mel_low, inv_mel_delta, fmask_start, fmask_end, tmask_start, tmask_end) per clip -- as the device bytes pa_mel_clip_params[B]
    (uint8, 24 per clip), through the pinned ring like the lengths."""
    if not isinstance(clips, C.Array):
        rows = [tuple(r) for r in clips]
        clips = (_lib.MelClipParams * len(rows))(*[_lib.MelClipParams(float(r[0]), float(r[1]), *(int(v) for v in r[2:])) for r in rows])
    host = torch.frombuffer(bytearray(bytes(clips)), dtype=torch.uint8)
    return upload_small(host, device)


def _mel_clip_table(clip_dev, B, what):
    if clip_dev.dtype != torch.uint8 or clip_dev.dim() != 1 or clip_dev.numel() != B * C.sizeof(_lib.MelClipParams):
        raise _lib.PasstAmdError(f"{what}: the per-clip table must be {B} x {C.sizeof(_lib.MelClipParams)} bytes (ops.upload_mel_clips), got "
                                 f"{clip_dev.dtype} {tuple(clip_dev.shape)}")
    return clip_dev


def mel_frontend_varlen_aug(wave, lens_dev, clip_dev, window, bin_mel, twiddle, params: MelParams, fill=0.0):
    """mel_frontend_varlen with every clip's own filterbank edges and SpecAugment bands: ``clip_dev`` is ops.upload_mel_clips' table
    (its six values replace params.mel_low / inv_mel_delta / fmask_* / tmask_*, which are not read; the caller guarantees finite
    mel_low and inv_mel_delta > 0).  The frames behind a clip's own end hold ``fill``, never the mask constant."""
    return mel_forward(wave, (window, bin_mel, twiddle), params, lens_dev, clip_dev, fill)


def mel_frontend_bwd_varlen_aug(wave, lens_dev, clip_dev, window, bin_mel, twiddle, params: MelParams, dout):
    """Gradient of mel_frontend_varlen_aug w.r.t. ``wave``; ``clip_dev`` is the forward call's table."""
    return mel_backward(wave, (window, bin_mel, twiddle), params, dout, lens_dev, clip_dev)


# ---- staging ---------------------------------------------------------------------------------
def _rowscale(rowscale, M, what):
    """A row-factor argument: None, or one f32 per row, contiguous."""
    if rowscale is not None and (rowscale.dtype != torch.float32 or rowscale.shape != (M,) or not rowscale.is_contiguous()):
        raise _lib.PasstAmdError(f"{what}: rowscale must be a contiguous f32 [{M}] tensor, got {rowscale.dtype} {tuple(rowscale.shape)}")
    return rowscale


def convert(x_f32, dtype, rowscale=None):
    """The copy of ``x_f32`` the next GEMM reads.  ``rowscale`` ([M] f32, x_f32 [M][D]): out[m] = rowscale[m] * x_f32[m] -- the gradient
    entering a branch that carries a stochastic-depth row factor; always a fresh buffer, in f32 mode too."""
    if rowscale is not None:
        M, D = x_f32.shape
        out = torch.empty((M, D), device=x_f32.device, dtype=TORCH_DTYPE[dtype])
        x_f32 = _aligned16(x_f32)
        check(_lib.load().pa_convert_f32_rowscale(_p(x_f32, torch.float32), _p(_rowscale(rowscale, M, "convert"), torch.float32), _p(out), M, D,
                                                  dtype, _stream()), "pa_convert_f32_rowscale")
        return out
    if dtype == PA_F32:
        return x_f32
    out = torch.empty(x_f32.shape, device=x_f32.device, dtype=TORCH_DTYPE[dtype])
    check(_lib.load().pa_convert_f32(_p(x_f32, torch.float32), _p(out), x_f32.numel(), dtype, _stream()), "pa_convert_f32")
    return out


def convert_f32(x_f32, out_lp):
    """out_lp[i] = (bf16 / f32) x_f32[i] into an existing tensor"""
    check(_lib.load().pa_convert_f32(_p(x_f32, torch.float32), _p(out_lp), x_f32.numel(), PA_DTYPE[out_lp.dtype], _stream()),
          "pa_convert_f32")


def convert_to_f32(x_lp, out_f32):
    """out_f32[i] = (float) x_lp[i]"""
    check(_lib.load().pa_convert_to_f32(_p(x_lp), PA_DTYPE[x_lp.dtype], _p(out_f32, torch.float32), x_lp.numel(), _stream()),
          "pa_convert_to_f32")


def transpose(x, out_dtype, ldo=None, out=None):
    """x [R][C] (contiguous rows, any supported dtype) -> [C][ldo] (ldo >= R, zero padded)."""
    R, Cc = x.shape
    ldo = R if ldo is None else ldo
    if out is None:
        out = torch.empty((Cc, ldo), device=x.device, dtype=TORCH_DTYPE[out_dtype])
    check(_lib.load().pa_transpose(_p(x, None, True), PA_DTYPE[x.dtype], R, Cc, x.stride(0), _p(out), out_dtype, ldo,
                                   _stream()), "pa_transpose")
    return out


def make_stage_table(entries, device):
    """entries: [(src f32 [R][C] contiguous, dst or None, dst_t or None)] -> (device table, n, total_tiles) for
    stage_weights; the tensors must stay alive (and in place) for as long as the table is used."""
    import numpy as np
    from ._lib import StageDesc
    arr = (StageDesc * len(entries))()
    tiles = 0
    for d, (src, dst, dst_t) in zip(arr, entries):
        R, Cc = src.shape
        assert src.is_contiguous() and src.dtype == torch.float32
        d.src, d.dst, d.dst_t = _p(src), _p(dst), _p(dst_t)
        d.rows, d.cols, d.tile_begin = R, Cc, tiles
        tiles += ((R + 63) // 64) * ((Cc + 63) // 64)
    host = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
    return host.to(device), len(entries), tiles


def make_adamw_stage_table(entries, device):
    """entries: [(offset, rows, cols, dst or None, dst_t or None)] in flat-buffer order -> (device table, n, total work items) for
    adamw_update (pa_adamw_stage_desc; a parameter without copies is one run of 4096 elements per work item)."""
    import numpy as np
    from ._lib import AdamwStageDesc
    arr = (AdamwStageDesc * len(entries))()
    items = 0
    for d, (off, rows, cols, dst, dst_t) in zip(arr, entries):
        d.offset, d.rows, d.cols, d.dst, d.dst_t, d.tile_begin = off, rows, cols, _p(dst), _p(dst_t), items
        items += ((rows + 63) // 64) * ((cols + 63) // 64) if (dst is not None or dst_t is not None) else (rows * cols + 4095) // 4096
    host = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
    return host.to(device), len(entries), items


def make_adamw_scales(pairs, device):
    """pairs: [(lr_scale, wd_scale)], one per table entry in table order -> the f32 [n][2] device array of adamw_update's ``scales``"""
    import numpy as np
    return torch.from_numpy(np.asarray(pairs, dtype=np.float32).reshape(-1, 2)).to(device)


_ADAMW_FLAT = ("pa_adamw", "pa_adamw_dev", "pa_adamw_clip")
_ADAMW_TABLE = ("pa_adamw_stage", "pa_adamw_stage_groups", "pa_adamw_groups", "pa_adamw_stage_clip")


def adamw_update(p, g, m, v, hyper, *, table=None, scales=None, dtype=None, gscale=None, entry=None):
    """One AdamW launch on the flat f32 buffers p / g / m / v (g is read only), whichever C entry serves it.
    hyper: the step's scalars by value, (lr, beta1, beta2, eps, weight_decay, step), or the 7-float device row of adamw_hyper (a launch
    whose arguments never change: capturable in a hipGraph).
    table: what make_adamw_stage_table / _Staged.adamw_table returned -- the parameters the launch covers (offsets relative to the
    buffers) and their GEMM-ready copies of ``dtype``, written in the same pass; None: the whole of p as one flat span.
    scales: make_adamw_scales' parameter groups -- table entry i is updated with lr * scales[i, 0] and weight_decay * scales[i, 1].
    gscale: one device float, the clip factor: the update is that of g * gscale.
    The entry is the one the combination names: flat pa_adamw / pa_adamw_dev (device row), pa_adamw_clip with gscale; table
    pa_adamw_stage, pa_adamw_stage_groups with scales, pa_adamw_groups with scales and no dtype (a table without copies),
    pa_adamw_stage_clip with gscale.  ``entry`` names another one that takes the same arguments (the parity tests drive all seven)."""
    by_value = not torch.is_tensor(hyper)
    if entry is None:
        if table is None:
            entry = "pa_adamw_clip" if gscale is not None else "pa_adamw" if by_value else "pa_adamw_dev"
        else:
            entry = ("pa_adamw_stage_clip" if gscale is not None else "pa_adamw_stage" if scales is None else
                     "pa_adamw_groups" if dtype is None else "pa_adamw_stage_groups")
    if entry not in (_ADAMW_FLAT if table is None else _ADAMW_TABLE):
        raise _lib.PasstAmdError(f"adamw_update: {entry} is no AdamW entry {'without' if table is None else 'with'} a table")
    lr, beta1, beta2, eps, wd, step = hyper if by_value else (0.0, 0.0, 0.0, 0.0, 0.0, 0)
    bufs = (_p(p, torch.float32), _p(g, torch.float32), _p(m, torch.float32), _p(v, torch.float32))
    scalars = (float(lr), float(beta1), float(beta2), float(eps), float(wd), int(step))
    row, factor = _p(None if by_value else hyper, torch.float32), _p(gscale, torch.float32)
    if table is None:
        args = {"pa_adamw": scalars, "pa_adamw_dev": (row,), "pa_adamw_clip": scalars + (row, factor)}[entry]
        args = (p.numel(),) + args
    else:
        tab, n, items = table[:3]
        assert scales is None or (scales.dtype == torch.float32 and scales.numel() == 2 * n and scales.is_contiguous())
        geo = (n, items) if entry == "pa_adamw_groups" else (n, items, dtype)
        sc = () if entry == "pa_adamw_stage" else (_p(scales),)
        args = (_p(tab),) + sc + geo + scalars + ((row, factor) if entry == "pa_adamw_stage_clip" else (row,))
    check(getattr(_lib.load(), entry)(*bufs, *args, _stream()), entry)


def stage_weights(table, n, tiles, dtype):
    check(_lib.load().pa_stage_weights(_p(table), n, tiles, dtype, _stream()), "pa_stage_weights")


# ---- layer norm ------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps, dtype, save_stats=True):
    M, D = x.shape
    y = torch.empty((M, D), device=x.device, dtype=TORCH_DTYPE[dtype])
    mean = torch.empty(M, device=x.device, dtype=torch.float32) if save_stats else None
    rstd = torch.empty(M, device=x.device, dtype=torch.float32) if save_stats else None
    check(_lib.load().pa_layernorm_fwd(_p(x, torch.float32), _p(gamma, torch.float32), _p(beta, torch.float32), _p(y), dtype, _p(mean), _p(rstd), M, D, eps,
                                       _stream()), "pa_layernorm_fwd")
    return y, mean, rstd


def _layernorm_bwd_rowscale(dy, x, gamma, mean, rstd, dres, dres2, rowscale, dgamma, dbeta, want_lp, accumulate, dcolsum, defer):
    """layernorm_bwd / layernorm_bwd2 with a row factor: dx stays unscaled, the copy (a second f32 buffer in f32 mode) and dcolsum are
    those of rowscale[m] * dx[m]."""
    M, D = x.shape
    dtype = PA_DTYPE[dy.dtype]
    lib = _lib.load()
    _rowscale(rowscale, M, "layernorm_bwd")
    dx = torch.empty((M, D), device=x.device, dtype=torch.float32)
    dx_lp = torch.empty((M, D), device=x.device, dtype=dy.dtype) if (want_lp or dtype == PA_F32) else None
    ws = torch.empty(lib.pa_layernorm_bwd_ws_floats(M, D), device=x.device, dtype=torch.float32)
    lead = (_p(dy), dtype, _p(x, torch.float32), _p(gamma, torch.float32), _p(mean, torch.float32), _p(rstd, torch.float32),
            _p(dres, torch.float32), _p(dres2, torch.float32), _p(rowscale, torch.float32), _p(dx), _p(dx_lp))
    if defer is not None and not accumulate:
        check(lib.pa_layernorm_bwd_partial_rowscale(*lead, _p(ws), M, D, _stream()), "pa_layernorm_bwd_partial_rowscale")
        rows = lib.pa_layernorm_bwd_rows(M)
        for j, out in enumerate((dgamma, dbeta, dcolsum)):
            if out is not None:
                defer.append((ws[j * D:], rows, 3 * D, D, out))
        return dx, dx_lp
    check(lib.pa_layernorm_bwd_rowscale(*lead, _p(dgamma), _p(dbeta), _p(dcolsum), int(accumulate), _p(ws), M, D, _stream()),
          "pa_layernorm_bwd_rowscale")
    return dx, dx_lp


def layernorm_bwd(dy, x, gamma, mean, rstd, dres, dgamma, dbeta, want_lp, accumulate=False, dcolsum=None, defer=None, rowscale=None):
    """Returns (dx f32, dx_lp or None).  dgamma/dbeta (and dcolsum = column sums of dx, if given) are written in place.
    defer: a list -- the parameter gradients stay as partial rows and (partial, rows, pitch, n, out) jobs are appended to it for
    the block's ONE finishing launch (wgrad_tn_batched(..., row_jobs=defer)) instead of a reduction launch per LayerNorm.
    rowscale ([M] f32): the factor of the branch the gradient enters (stochastic depth); dx stays the residual gradient, dx_lp --
    in f32 mode a second f32 buffer -- and dcolsum are those of rowscale[m] * dx[m]."""
    if rowscale is not None:
        return _layernorm_bwd_rowscale(dy, x, gamma, mean, rstd, dres, None, rowscale, dgamma, dbeta, want_lp, accumulate, dcolsum, defer)
    M, D = x.shape
    dtype = PA_DTYPE[dy.dtype]
    lib = _lib.load()
    dx = torch.empty((M, D), device=x.device, dtype=torch.float32)
    dx_lp = torch.empty((M, D), device=x.device, dtype=dy.dtype) if (want_lp and dtype != PA_F32) else None
    ws = torch.empty(lib.pa_layernorm_bwd_ws_floats(M, D), device=x.device, dtype=torch.float32)
    if defer is not None and not accumulate:
        check(lib.pa_layernorm_bwd_partial(_p(dy), dtype, _p(x, torch.float32), _p(gamma, torch.float32), _p(mean, torch.float32),
                                           _p(rstd, torch.float32), _p(dres, torch.float32), _p(dx), _p(dx_lp), _p(ws), M, D, _stream()),
              "pa_layernorm_bwd_partial")
        rows = lib.pa_layernorm_bwd_rows(M)
        for j, out in enumerate((dgamma, dbeta, dcolsum)):
            if out is not None:
                defer.append((ws[j * D:], rows, 3 * D, D, out))
        return dx, (dx if dtype == PA_F32 else dx_lp)
    check(lib.pa_layernorm_bwd(_p(dy), dtype, _p(x, torch.float32), _p(gamma, torch.float32), _p(mean, torch.float32), _p(rstd, torch.float32), _p(dres, torch.float32), _p(dx), _p(dx_lp),
                               _p(dgamma), _p(dbeta), _p(dcolsum), int(accumulate), _p(ws), M, D, _stream()),
          "pa_layernorm_bwd")
    return dx, (dx if dtype == PA_F32 else dx_lp)


def layernorm_bwd2(dy, x, gamma, mean, rstd, dres, dres2, dgamma, dbeta, want_lp, accumulate=False, dcolsum=None, defer=None,
                   rowscale=None):
    """layernorm_bwd with a second addend: dx = dres + dres2 + LN'(dy) -- ``dres2`` [M][D] f32 is a gradient injected into the
    residual stream at this LayerNorm's input; the 16-bit copy and ``dcolsum`` include it.  Same returns, ``defer`` and ``rowscale``
    contract (the injected gradient joins dx before the scaling)."""
    M, D = x.shape
    dtype = PA_DTYPE[dy.dtype]
    lib = _lib.load()
    if dres2 is None or dres2.shape != (M, D):
        raise _lib.PasstAmdError(f"layernorm_bwd2: dres2 must be an f32 [{M}][{D}] tensor")
    if rowscale is not None:
        return _layernorm_bwd_rowscale(dy, x, gamma, mean, rstd, dres, dres2, rowscale, dgamma, dbeta, want_lp, accumulate, dcolsum, defer)
    dx = torch.empty((M, D), device=x.device, dtype=torch.float32)
    dx_lp = torch.empty((M, D), device=x.device, dtype=dy.dtype) if (want_lp and dtype != PA_F32) else None
    ws = torch.empty(lib.pa_layernorm_bwd_ws_floats(M, D), device=x.device, dtype=torch.float32)
    if defer is not None and not accumulate:
        check(lib.pa_layernorm_bwd2_partial(_p(dy), dtype, _p(x, torch.float32), _p(gamma, torch.float32), _p(mean, torch.float32),
                                            _p(rstd, torch.float32), _p(dres, torch.float32), _p(dres2, torch.float32), _p(dx), _p(dx_lp),
                                            _p(ws), M, D, _stream()), "pa_layernorm_bwd2_partial")
        rows = lib.pa_layernorm_bwd_rows(M)
        for j, out in enumerate((dgamma, dbeta, dcolsum)):
            if out is not None:
                defer.append((ws[j * D:], rows, 3 * D, D, out))
        return dx, (dx if dtype == PA_F32 else dx_lp)
    check(lib.pa_layernorm_bwd2(_p(dy), dtype, _p(x, torch.float32), _p(gamma, torch.float32), _p(mean, torch.float32), _p(rstd, torch.float32),
                                _p(dres, torch.float32), _p(dres2, torch.float32), _p(dx), _p(dx_lp), _p(dgamma), _p(dbeta), _p(dcolsum),
                                int(accumulate), _p(ws), M, D, _stream()), "pa_layernorm_bwd2")
    return dx, (dx if dtype == PA_F32 else dx_lp)


# ---- GEMM ------------------------------------------------------------------------------------
# A/B knobs: the tile variant of every plain-store / residual NT GEMM of the step (PASST_AMD_TUNE_STORE / PASST_AMD_TUNE_RESID =
# a pa_gemm_args.tune value, e.g. 13 = the 192 x 128 two-workgroups-per-CU tile with epilogue v2)
_TUNE_BY_EPI = {EPI_STORE: int(os.environ.get("PASST_AMD_TUNE_STORE", "0")), EPI_RESID: int(os.environ.get("PASST_AMD_TUNE_RESID", "0"))}


def gemm_nt(A, B, dtype, epilogue=EPI_STORE, bias=None, resid=None, aux=None, out_f32=None, out_lp=None,
            out_lp2=None, row_mod=0, out_batch_rows=0, out_row_off=0, split_k=1, M=None, N=None, K=None,
            colsum_out=None, colsum_ws=None, colsum_accumulate=False, flags=0, colscale_n=0, colscale=1.0, tune=None, rowscale=None):
    """C[M][N] = A[M][K] B[N][K]^T with the fused epilogues of include/passt_amd.h.  EPI_DGELU can also return the
    column sums of its output (colsum_out [N] f32; colsum_ws from gemm_colsum_ws).  rowscale ([M] f32, EPI_RESID without the row
    remap): out_f32[m] = resid[m] + rowscale[m] * (A B^T + bias)[m] (pa_gemm_nt_rowscale / pa_gemm_nt_splitk_rowscale)."""
    a = GemmArgs()
    a.dtype, a.epilogue = dtype, epilogue
    a.M = A.shape[0] if M is None else M
    a.N = B.shape[0] if N is None else N
    a.K = A.shape[1] if K is None else K
    a.lda, a.ldb = A.stride(0), B.stride(0)
    a.A, a.B = _p(A, dtype, True), _p(B, dtype, True)
    a.bias = _p(bias, torch.float32)
    a.resid = _p(resid, torch.float32, True)
    a.ldr = resid.stride(0) if resid is not None else 0
    a.row_mod, a.out_batch_rows, a.out_row_off = row_mod, out_batch_rows, out_row_off
    a.aux = _p(aux, dtype, True)
    a.ldaux = aux.stride(0) if aux is not None else 0
    a.out_f32 = _p(out_f32, torch.float32, True)
    a.ldo32 = (out_f32.stride(-2) if out_f32 is not None else 0)
    a.out_lp = _p(out_lp, dtype, True)
    a.ldolp = out_lp.stride(0) if out_lp is not None else 0
    a.out_lp2 = _p(out_lp2, dtype, True)
    a.ldolp2 = out_lp2.stride(0) if out_lp2 is not None else 0
    a.split_k = split_k
    if tune is None:
        tune = _TUNE_BY_EPI.get(epilogue) or GEMM_TUNE
    a.tune = tune
    a.reserved = GEMM_RESERVED | _call.gemm_flags | flags
    a.colscale_n, a.colscale = colscale_n, colscale
    a.colsum_out, a.colsum_ws, a.colsum_accumulate = _p(colsum_out, torch.float32), _p(colsum_ws, torch.float32), int(colsum_accumulate)
    # problems that leave most CUs idle (few [M][768] tiles, long K) go through the split-K entry with a workspace
    ws_n = 0
    if epilogue in (EPI_STORE, EPI_RESID) and dtype == PA_BF16 and row_mod == 0 and split_k == 1 and not tune:
        ws_n = _splitk_ws_floats(a.M, a.N, a.K, epilogue, dtype)

    if rowscale is not None:
        if epilogue != EPI_RESID or row_mod:
            raise _lib.PasstAmdError("gemm_nt: rowscale goes with EPI_RESID without the row remap")
        _rowscale(rowscale, a.M, "gemm_nt")

    def launch():
        if rowscale is not None:
            rs = _p(rowscale, torch.float32)
            if ws_n:
                ws = _splitk_ws(A.device, ws_n)
                check(_lib.load().pa_gemm_nt_splitk_rowscale(C.byref(a), rs, ws.data_ptr(), ws_n, _stream()), "pa_gemm_nt_splitk_rowscale")
            else:
                check(_lib.load().pa_gemm_nt_rowscale(C.byref(a), rs, _stream()), "pa_gemm_nt_rowscale")
        elif ws_n:
            ws = _splitk_ws(A.device, ws_n)
            check(_lib.load().pa_gemm_nt_splitk(C.byref(a), ws.data_ptr(), ws_n, _stream()), "pa_gemm_nt_splitk")
        else:
            check(_lib.load().pa_gemm_nt(C.byref(a), _stream()), "pa_gemm_nt")

    if GEMM_PROFILE is None:
        launch()
        return
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    launch()
    ev1.record()
    kind = _EPI_NAME[epilogue] + ("_rowscale" if rowscale is not None else "")
    if PROFILE_BY_SHAPE:
        kind = f"{kind}_M{a.M}_N{a.N}_K{a.K}"
    GEMM_PROFILE.setdefault(kind, []).append((ev0, ev1, 2.0 * a.M * a.N * a.K))


@functools.lru_cache(maxsize=None)
def _splitk_ws_floats(M, N, K, epilogue, dtype):
    return int(_lib.load().pa_gemm_nt_splitk_ws_floats(M, N, K, epilogue, dtype))


_SPLITK_WS = {}


def _splitk_ws(device, n):
    """f32 workspace of pa_gemm_nt_splitk, one per (device, stream, host thread): the partial tiles live only between the two
    launches of one call and calls of one thread on one stream are ordered; two host threads on the same stream (trainer +
    autograd thread) could interleave their launch pairs, so they do not share a workspace."""
    key = (device, torch.cuda.current_stream(device).cuda_stream, threading.get_ident())
    ws = _SPLITK_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _SPLITK_WS[key] = torch.empty(n, device=device, dtype=torch.float32)
    return ws


def gemm_colsum_ws(M, N, device, ws=None):
    """f32 workspace for gemm_nt(..., colsum_out=...); reuses `ws` when it is large enough."""
    n = _lib.load().pa_gemm_colsum_ws_floats(M, N)
    if ws is None or ws.numel() < n:
        ws = torch.empty(n, device=device, dtype=torch.float32)
    return ws


def linear(x_lp, W_lp, bias, dtype, colscale_n=0, colscale=1.0):
    """out_lp[M][N] = x W^T + b; the first colscale_n output columns times colscale (the qkv Linear hands attention
    q * scale * log2(e): ATTN_Q_PRESCALED)"""
    out = torch.empty((x_lp.shape[0], W_lp.shape[0]), device=x_lp.device, dtype=TORCH_DTYPE[dtype])
    gemm_nt(x_lp, W_lp, dtype, EPI_STORE, bias=bias, out_lp=out, colscale_n=colscale_n, colscale=colscale)
    return out


class BlockedPre:
    """The pre-activation of an MLP in the library's blocked layout (PA_GEMM_BLOCKED_PRE): opaque storage written by the
    fc1 + GELU epilogue and read by the GELU' epilogue of the matching input-gradient GEMM, nothing else."""
    __slots__ = ("buf", "shape")

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, shape


@functools.lru_cache(maxsize=None)
def _lib_blocked_pre_ok(M, N, K):
    return bool(_lib.load().pa_gemm_blocked_pre_ok(M, N, K))


def blocked_pre_ok(M, N, K):
    # only the library query is cached: GEMM_TUNE and the environment switch are read on every call (a
    # result cached under a forced variant disabled -- or wrongly enabled -- the blocked path for the rest of the process)
    return not GEMM_TUNE and not os.environ.get("PASST_AMD_NO_BLOCKED_PRE") and _lib_blocked_pre_ok(M, N, K)


# A/B knobs (tools/bench_epi13.py, profiles/r06_gemm_variants_epi13.txt): the tile variant of the two MLP-epilogue GEMMs in the
# step, blocked pre-activation kept (every variant listed in csrc/gemm.hip launch_gemm's blocked switch has it)
TUNE_GELU = int(os.environ.get("PASST_AMD_TUNE_GELU", "0")) or None
TUNE_DGELU = int(os.environ.get("PASST_AMD_TUNE_DGELU", "0")) or None


def linear_gelu(x_lp, W_lp, bias, dtype):
    """(pre, act): act = gelu(x W^T + b) row-major; pre = x W^T + b, row-major or -- where the library has the blocked
    form for this shape -- a BlockedPre that only dgelu_gemm() can consume."""
    M, N = x_lp.shape[0], W_lp.shape[0]
    act = torch.empty((M, N), device=x_lp.device, dtype=TORCH_DTYPE[dtype])
    if dtype == PA_BF16 and blocked_pre_ok(M, N, x_lp.shape[1]):
        buf = torch.empty(_lib.load().pa_gemm_blocked_pre_elems(M, N), device=x_lp.device, dtype=TORCH_DTYPE[dtype])
        # blocks of rows no wave tile of this GEMM writes: the GELU' epilogue of the last row tile adds and subtracts them
        # for the fused bias sums, so they must be finite whatever tile height the two GEMMs resolve to
        buf[(M + 31) // 32 * 32 * N:].zero_()
        gemm_nt(x_lp, W_lp, dtype, EPI_GELU, bias=bias, out_lp=buf.view(-1, N), out_lp2=act, flags=GEMM_BLOCKED_PRE, tune=TUNE_GELU)
        return BlockedPre(buf, (M, N)), act
    pre = torch.empty((M, N), device=x_lp.device, dtype=TORCH_DTYPE[dtype])
    gemm_nt(x_lp, W_lp, dtype, EPI_GELU, bias=bias, out_lp=pre, out_lp2=act)
    return pre, act


def dgelu_gemm(dy_lp, Wt_lp, pre, dtype, colsum_out=None, colsum_ws=None, defer=None):
    """d_pre[M][N] = (dy Wt^T) * gelu'(pre): the input gradient of fc2 times the GELU derivative; pre as returned by
    linear_gelu (row-major tensor or BlockedPre).  defer (a list, with colsum_out): the column sums stay as one partial row per
    wave tile in colsum_ws and a (partial, rows, pitch, n, out) job is appended for the block's finishing launch."""
    blocked = isinstance(pre, BlockedPre)
    M, N = pre.shape
    d_pre = torch.empty((M, N), device=dy_lp.device, dtype=TORCH_DTYPE[dtype])
    deferred = defer is not None and colsum_out is not None
    gemm_nt(dy_lp, Wt_lp, dtype, EPI_DGELU, aux=pre.buf.view(-1, N) if blocked else pre, out_lp=d_pre,
            colsum_out=colsum_out, colsum_ws=colsum_ws, flags=(GEMM_BLOCKED_PRE if blocked else 0) | (_lib.GEMM_COLSUM_DEFER if deferred else 0),
            tune=TUNE_DGELU if blocked else None)
    if deferred:
        defer.append((colsum_ws, _lib.load().pa_gemm_last_colsum_rows(), N, N, colsum_out))
    return d_pre


def linear_resid(x_lp, W_lp, bias, resid_f32, dtype, out=None, rowscale=None):
    """out_f32[M][N] = resid + x W^T + b; with rowscale ([M] f32): resid[m] + rowscale[m] * (x W^T + b)[m]"""
    if out is None:
        out = torch.empty_like(resid_f32)
    if rowscale is None:
        gemm_nt(x_lp, W_lp, dtype, EPI_RESID, bias=bias, resid=resid_f32, out_f32=out)
    else:
        gemm_nt(x_lp, W_lp, dtype, EPI_RESID, bias=bias, resid=resid_f32, out_f32=out, rowscale=rowscale)
    return out


def pick_split_k(n_out_tiles, ksteps):
    """Enough workgroups to fill 256 CUs x 2, at least 8 K-steps per slice."""
    s = max(1, min(64, (768 + n_out_tiles - 1) // n_out_tiles))
    return max(1, min(s, ksteps // 8 if ksteps >= 8 else 1))


def wgrad(dY_t, X_t, out_f32, dtype, accumulate=False, partial_ws=None):
    """out[N][K] (+)= dY_t[N][Mp] . X_t[K][Mp]^T  -- the weight gradient dY^T X from transposed,
    zero-padded operands; deterministic split-K (f32 partial slabs + ordered reduction)."""
    N, Mp = dY_t.shape
    K = X_t.shape[0]
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    ksteps = Mp // kpad(dtype)
    S = pick_split_k(tiles, ksteps)
    need = S * N * K
    if partial_ws is None or partial_ws.numel() < need:
        partial_ws = torch.empty(need, device=dY_t.device, dtype=torch.float32)
    part = partial_ws[:need].view(S, N, K)
    gemm_nt(dY_t, X_t, dtype, EPI_PARTIAL, out_f32=part, split_k=S)
    check(_lib.load().pa_reduce_partials(_p(part), S, N * K, _p(out_f32), int(accumulate), _stream()),
          "pa_reduce_partials")
    return partial_ws


def tn_step_rows():
    """PA_TN_STEP_ROWS of the loaded library: tokens per pipeline stage of the bf16 role-split TN kernel."""
    return _lib.load().pa_gemm_tn_step_rows()



def pick_split_k_slots(tiles, steps, slots=256):
    """split count for the one-workgroup-per-CU kernels: fill whole rounds of `slots` workgroups
    (tile quantisation), at least 8 reduction steps per slice, prefer fewer slices on ties."""
    best, best_score = 1, -1.0
    for S in range(1, max(1, min(64, steps // 8)) + 1):
        blocks = tiles * S
        eff = blocks / (((blocks + slots - 1) // slots) * slots)
        score = eff - 0.003 * S
        if score > best_score:
            best, best_score = S, score
    return best


_SPLITS_CACHE = {}
_FORCE_SLICES = int(os.environ.get("PASST_AMD_WGRAD_SLICES", "0"))


def pick_batched_splits(probs, slots=256):
    """Memoised front of _pick_batched_splits (the search walks ~470 slice lengths in Python: ~1 ms per call, and the step
    asks the same question once per transformer block)."""
    key = (tuple(probs), slots)
    hit = _SPLITS_CACHE.get(key)
    if hit is None:
        hit = _SPLITS_CACHE[key] = _pick_batched_splits(list(probs), slots)
        if _FORCE_SLICES:       # A/B knob (profiles/r06_wgrad_slices.txt): every problem cut into this many token slices
            hit = _SPLITS_CACHE[key] = [max(1, min(_FORCE_SLICES, st)) for _, st in probs]
    return hit


def _pick_batched_splits(probs, slots=256):
    """probs: [(tiles, k_steps)] of the problems sharing one launch.  Every work item is one 256x256 tile x one K slice of
    L steps of 48 tokens (S_p = ceil(steps_p / L)).  Cost model (us, MI355X measurements): rounds x (L + 4) x 1.2 for the K loops and
    per-item epilogues, with rounds = ceil(#items / slots), plus 0.05 per item for the f32 partial slab it writes and the
    reduction reads back (256 KiB each way; about half of it hides under the K loops -- calibrated on the passt_s block:
    7 slices beat 2 and 4, run 82)."""
    best, best_cost = None, None
    for L in range(max(p[1] for p in probs), 3, -1):
        S = [max(1, min(64, -(-st // L))) for _, st in probs]
        items = sum(t * s_ for (t, _), s_ in zip(probs, S))
        per = max(-(-st // s_) for (_, st), s_ in zip(probs, S))
        cost = -(-items // slots) * (per + 4) * 1.2 + items * 0.05        # 48-token steps: ~1.2 us each, ~4.8 us fixed per item
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = S, cost
    return best if best is not None else [1] * len(probs)


_PLAN_CACHE = {}
# A/B switch of the long/short plan (profiles/r07_wgrad_long_short.txt), read once: PASST_AMD_WGRAD_PLAN=uniform cuts equal
# token slices everywhere, as _pick_batched_splits does; =long_short lets the planner below decide.  A forced slice count
# (PASST_AMD_WGRAD_SLICES) is a uniform plan too.
WGRAD_PLAN_DEFAULT = "long_short"       # in the step at batch 64: 21.38 -> 21.07 ms, weight gradients 377 -> 357 us per block
_SHORT_ITEM_COST = 1.25       # modelled cost of a short item's steps relative to a long item's (see _long_short_cost)
_PLAN_MIN_GAIN = 0.04         # modelled gain below which the long/short plan is not taken
_FORCE_UNIFORM = os.environ.get("PASST_AMD_WGRAD_PLAN", WGRAD_PLAN_DEFAULT) == "uniform" or _FORCE_SLICES > 0


def pick_batched_plan(probs, slots=256):
    """Memoised front of _pick_batched_plan: (n_long, long_steps, splits).  n_long = 0: the uniform plan, splits[p] equal
    slices of problem p (pa_gemm_tn_batched).  n_long >= 1: every tile is cut into n_long slices of long_steps token steps and
    one short slice of the rest (pa_gemm_tn_batched_plan); splits[p] = n_long + 1 slabs."""
    if _FORCE_UNIFORM:
        return 0, 0, pick_batched_splits(probs, slots)
    key = (tuple(probs), slots)
    hit = _PLAN_CACHE.get(key)
    if hit is None:
        hit = _PLAN_CACHE[key] = _pick_batched_plan(list(probs), slots)
    return hit


def _uniform_cost(probs, S, slots=256):
    """Modelled us of the uniform plan S (slices per problem): the cost _pick_batched_splits minimises."""
    items = sum(t * s_ for (t, _), s_ in zip(probs, S))
    per = max(-(-st // s_) for (_, st), s_ in zip(probs, S))
    return -(-items // slots) * (per + 4) * 1.2 + items * 0.05


def _long_short_cost(tiles, steps, a, L, slots=256):
    """Modelled us of `a` long slices of L steps + one short slice of steps - a * L per tile, with the constants of
    _pick_batched_splits (1.2 us per step, 4 steps' worth fixed per item, 0.05 per slab).  The makespan comes from dealing the
    items in launch order -- all long items, then all short ones -- each onto the CU that frees first.  A short item is
    charged _SHORT_ITEM_COST times its steps (re-fitted on MI355X, profiles/r07_wgrad_long_short.txt: with the short items'
    three rounds as long as one long item, the model's optimum, the launch ran 90 us over the model; it met the model once the
    short rounds were 0.8 of a long item or less; supposed cause: a freed CU waits for the next item in launch order that is
    bound to ITS XCD, so the short rounds slip)."""
    import heapq
    free = [0.0] * slots
    end = 0.0
    for steps_item, count, k in ((L, a * tiles, 1.0), (steps - a * L, tiles, _SHORT_ITEM_COST)):
        dur = (steps_item + 4) * 1.2 * k
        for _ in range(count):
            t = free[0] + dur
            heapq.heapreplace(free, t)
            end = max(end, t)
    return end + tiles * (a + 1) * 0.05


def _pick_batched_plan(probs, slots=256):
    """The cheaper of the best uniform split and the best long/short plan (a = 1 or 2 long slices of L steps, a short slice
    of R = steps - a * L, 1 <= R <= L) under one cost model.  With equal slices tiles x slices has to land just under a
    multiple of the CU count or the last round runs partly empty, which is what keeps the passt_s block at 7 slices (756
    items, 2.95 rounds); two long slices on 216 CUs with the short third dealt onto the other 40 last the same 3/7 of the
    token axis with 324 prologues, epilogues and slabs.  Problems with different token counts keep the uniform plan, and so
    does a launch whose equal slices already fit one round (the ESC-50 block: 2 x 108 items): there is no partly empty round
    to win back, and the model's constants are not fine enough to rank plans half a microsecond apart."""
    S = _pick_batched_splits(probs, slots)
    steps = probs[0][1]
    tiles = sum(t for t, _ in probs)
    if any(st != steps for _, st in probs) or sum(t * s_ for (t, _), s_ in zip(probs, S)) <= slots:
        return 0, 0, S
    best, best_cost = (0, 0, S), _uniform_cost(probs, S, slots)
    for a in (1, 2):
        for L in range((steps - 1) // a, -(-steps // (a + 1)) - 1, -1):        # 1 <= R <= L; on a tie the shorter short slice
            cost = _long_short_cost(tiles, steps, a, L, slots)
            if cost < best_cost - 1e-9:
                best, best_cost = (a, L, [a + 1] * len(probs)), cost
    # the model is within a few per cent of the measured launches, not better: a smaller modelled gain keeps the uniform plan
    return best if best_cost < (1.0 - _PLAN_MIN_GAIN) * _uniform_cost(probs, S, slots) else (0, 0, S)


def wgrad_batched_ws_floats(splits, shapes):
    """f32 elements of the partial workspace of wgrad_tn_batched: splits[p] slabs of problem p's N x K gradient, and of its N
    column sums where it has a bias gradient.  shapes: [(N, K, has_db)]."""
    return sum(S * N * (K + (1 if has_db else 0)) for S, (N, K, has_db) in zip(splits, shapes))


def wgrad_tn(dY, X, out_f32, dtype, accumulate=False, partial_ws=None, db=None):
    """out[N][K] (+)= dY[M][N]^T X[M][K], operands read in place (pa_gemm_tn), deterministic split-K.  db [N] f32 (bf16
    role-split kernel only, see wgrad_tn_fuses_bias): (+)= column sums of dY out of the same launch."""
    Mtok, N = dY.shape
    K = X.shape[1]
    if dtype == PA_BF16 and GEMM_TUNE != 1:      # role-split 256x256 kernel, one workgroup per CU
        tiles = ((N + 255) // 256) * ((K + 255) // 256)
        S = pick_split_k_slots(tiles, (Mtok + tn_step_rows() - 1) // tn_step_rows())
    else:
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        mrows = 64 if dtype == PA_BF16 else 32
        S = pick_split_k(tiles, (Mtok + mrows - 1) // mrows)
    assert db is None or wgrad_tn_fuses_bias(dtype)
    need = S * N * K + (S * N if db is not None else 0)
    if partial_ws is None or partial_ws.numel() < need:
        partial_ws = torch.empty(need, device=dY.device, dtype=torch.float32)
    part = partial_ws[:S * N * K].view(S, N, K)
    a = GemmArgs()
    a.dtype, a.epilogue = dtype, EPI_PARTIAL
    a.M, a.N, a.K = N, K, Mtok
    a.lda, a.ldb = dY.stride(0), X.stride(0)
    a.A, a.B = _p(dY, dtype, True), _p(X, dtype, True)
    a.out_f32, a.ldo32 = _p(part), K
    a.split_k = S
    a.tune = GEMM_TUNE
    bpart = partial_ws[S * N * K:need] if db is not None else None
    a.colsum_ws = _p(bpart)
    lib = _lib.load()
    # the bracket covers the split-K reductions too: they are part of what a weight gradient costs
    ev0 = ev1 = None
    if GEMM_PROFILE is not None:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    check(lib.pa_gemm_tn(C.byref(a), _stream()), "pa_gemm_tn")
    check(lib.pa_reduce_partials(_p(part), S, N * K, _p(out_f32), int(accumulate), _stream()), "pa_reduce_partials")
    if db is not None:
        check(lib.pa_reduce_partials(_p(bpart), S, N, _p(db, torch.float32), int(accumulate), _stream()), "pa_reduce_partials")
    if ev0 is not None:
        ev1.record()
        GEMM_PROFILE.setdefault("wgrad_tn", []).append((ev0, ev1, 2.0 * N * K * Mtok))
    return partial_ws


def wgrad_tn_fuses_bias(dtype):
    """True when wgrad_tn / wgrad_tn_batched can return colsum(dY) from the weight-gradient launch itself."""
    return dtype == PA_BF16 and GEMM_TUNE != 1


def wgrad_tn_batched(problems, dtype, partial_ws=None, row_jobs=None, plan=None):
    """problems: up to 4 of (dY [M][N], X [M][K], out [N][K] f32, accumulate[, db [N] f32 or None]): all weight gradients of a
    block in ONE pa_gemm_tn_batched launch + ONE batched finishing reduction.  A problem with db also gets its bias gradient
    (column sums of dY) out of the same launch.  row_jobs: (partial, rows, pitch, n, out) reductions of many short partial rows
    (deferred LayerNorm / GELU' parameter gradients of the block, see layernorm_bwd / dgelu_gemm) that ride in the same finishing
    launch.  plan=(n_long, long_steps) forces that long/short plan (pick_batched_plan; tests), plan=(0, 0) the uniform one.
    Returns the (possibly grown) partial workspace."""
    from ._lib import ReduceDesc
    assert dtype == PA_BF16 and 1 <= len(problems) <= 4
    problems = [tuple(p) + (None,) * (5 - len(p)) for p in problems]
    metas = []
    for dY, X, out, acc, db in problems:
        Mtok, N = dY.shape
        metas.append((Mtok, N, X.shape[1]))
    shapes = [(((N + 255) // 256) * ((K + 255) // 256), (Mtok + tn_step_rows() - 1) // tn_step_rows()) for Mtok, N, K in metas]
    if plan is None:
        n_long, long_steps, splits = pick_batched_plan(shapes)
    elif plan[0] == 0:
        n_long, long_steps, splits = 0, 0, pick_batched_splits(shapes)
    else:
        n_long, long_steps = plan
        splits = [n_long + 1] * len(problems)
    need = wgrad_batched_ws_floats(splits, [(m[1], m[2], p[4] is not None) for m, p in zip(metas, problems)])
    if partial_ws is None or partial_ws.numel() < need:
        partial_ws = torch.empty(need, device=problems[0][0].device, dtype=torch.float32)
    row_jobs = row_jobs or []
    nred = len(problems) + sum(1 for p in problems if p[4] is not None) + len(row_jobs)
    args = (GemmArgs * len(problems))()
    red = (ReduceDesc * nred)()
    off, flops, k = 0, 0.0, len(problems)
    for a, r, (dY, X, out, acc, db), (Mtok, N, K), S in zip(args, red, problems, metas, splits):
        part = partial_ws[off:off + S * N * K]
        off += S * N * K
        a.dtype, a.epilogue = dtype, EPI_PARTIAL
        a.M, a.N, a.K = N, K, Mtok
        a.lda, a.ldb = dY.stride(0), X.stride(0)
        a.A, a.B = _p(dY, dtype, True), _p(X, dtype, True)
        a.out_f32, a.ldo32 = _p(part), K
        a.split_k, a.tune = S, TN_BATCH_ORDER
        r.partial, r.out, r.n, r.splits, r.accumulate = _p(part), _p(out, torch.float32), N * K, S, int(acc)
        if db is not None:              # bias partials [S][N] behind the weight partials; one more slab set to reduce
            bpart = partial_ws[off:off + S * N]
            off += S * N
            a.colsum_ws = _p(bpart)
            rb = red[k]
            k += 1
            rb.partial, rb.out, rb.n, rb.splits, rb.accumulate = _p(bpart), _p(db, torch.float32), N, S, int(acc)
        flops += 2.0 * N * K * Mtok
    for part_rows, rows, pitch, n, out in row_jobs:
        rb = red[k]
        k += 1
        rb.partial, rb.out, rb.n, rb.splits, rb.accumulate = _p(part_rows, torch.float32, True), _p(out, torch.float32), n, rows, 0
        rb.pitch, rb.mode = pitch, _lib.REDUCE_ROWS
    lib = _lib.load()
    ev0 = ev1 = None
    if GEMM_PROFILE is not None:        # the bracket covers the batched split-K reduction too
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
    if n_long:
        check(lib.pa_gemm_tn_batched_plan(args, len(problems), n_long, long_steps, _stream()), "pa_gemm_tn_batched_plan")
    else:
        check(lib.pa_gemm_tn_batched(args, len(problems), _stream()), "pa_gemm_tn_batched")
    # a normal block fills the launch exactly (4 weight gradients + qkv.bias + 2 x 3 LayerNorm rows + fc1.bias = 12 =
    # PA_REDUCE_BATCH_MAX); anything beyond goes out as a second launch instead of failing in the middle of a backward
    for lo in range(0, nred, REDUCE_BATCH_MAX):
        n = min(REDUCE_BATCH_MAX, nred - lo)
        check(lib.pa_reduce_partials_batched(C.cast(C.byref(red, lo * C.sizeof(ReduceDesc)), C.POINTER(ReduceDesc)), n, _stream()),
              "pa_reduce_partials_batched")
    if ev0 is not None:
        ev1.record()
        GEMM_PROFILE.setdefault("wgrad_tn", []).append((ev0, ev1, flops))
    return partial_ws


REDUCE_BATCH_MAX = 12         # include/passt_amd.h PA_REDUCE_BATCH_MAX


def colsum(x, out_f32, accumulate=False):
    """out[C] (+)= column sums of the tall matrix x[R][C] (bf16 or f32)."""
    R, Cc = x.shape
    lib = _lib.load()
    ws = torch.empty(lib.pa_colsum_ws_floats(R, Cc), device=x.device, dtype=torch.float32)
    check(lib.pa_colsum(_p(x, None, True), PA_DTYPE[x.dtype], R, Cc, x.stride(0), _p(out_f32, torch.float32), int(accumulate), _p(ws),
                        _stream()), "pa_colsum")


def rowsum(x, out_f32, ncols=None, accumulate=False):
    R, Cc = x.shape
    check(_lib.load().pa_rowsum(_p(x, None, True), PA_DTYPE[x.dtype], R, Cc if ncols is None else ncols, x.stride(0),
                                _p(out_f32), int(accumulate), _stream()), "pa_rowsum")


def colsum_f32(x, out_f32, accumulate=False):
    R, Cc = x.shape
    check(_lib.load().pa_colsum_f32(_p(x, torch.float32, True), R, Cc, x.stride(0), _p(out_f32, torch.float32), int(accumulate), _stream()),
          "pa_colsum_f32")


# ---- attention -------------------------------------------------------------------------------
ATTN_Q_PRESCALED = 1          # include/passt_amd.h PA_ATTN_Q_PRESCALED
ATTN_BWD_TWO_PASS = 2         # PA_ATTN_BWD_TWO_PASS: force the dQ + dK/dV kernel pair (A/B, tests); PASST_AMD_ATTN_BWD=two_pass sets it everywhere
ATTN_BWD_SINGLE_PASS = 4      # PA_ATTN_BWD_SINGLE_PASS: force the single-pass kernel wherever it applies; PASST_AMD_ATTN_BWD=single_pass
ATTN_BWD_SINGLE_PASS_W16 = 8  # PA_ATTN_BWD_SINGLE_PASS_W16 (ABI 6): the single pass as sixteen waves of 32 keys; PASST_AMD_ATTN_BWD=single_pass_w16
_ATTN_BWD_FORCE = {"two_pass": ATTN_BWD_TWO_PASS, "single_pass": ATTN_BWD_SINGLE_PASS,
                   "single_pass_w16": ATTN_BWD_SINGLE_PASS_W16}.get(os.environ.get("PASST_AMD_ATTN_BWD", ""), 0)
LOG2E = 1.4426950408889634


def attention_fwd(qkv, B, H, N, scale, nq=None, flags=0):
    """o[(b*nq+q)][H*64], lse[(b*H+h)*nq+q] for the first nq queries of every sequence (nq=None: all N).
    flags=ATTN_Q_PRESCALED: the q third of qkv holds q * scale * log2(e)."""
    dtype = PA_DTYPE[qkv.dtype]
    nq = N if nq is None else nq
    D = H * 64
    o = torch.empty((B * nq, D), device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty((B * H * nq,), device=qkv.device, dtype=torch.float32)
    _timed("attn_fwd", 4.0 * nq * N * 64 * B * H,
           lambda: check(_lib.load().pa_attention_fwd(_p(qkv, None, True), qkv.stride(0), _p(o), o.stride(0), _p(lse), B, H, N, nq,
                                                      scale, dtype, flags, _stream()), "pa_attention_fwd"))
    return o, lse


def attention_fwd_varlen(qkv, cu_tok, B, H, max_N, scale, nq=None, flags=0):
    """Packed sequences: sequence b owns rows cu_tok[b] .. cu_tok[b+1] of qkv [total][3*H*64] (cu_tok: B + 1 int32 on the device,
    cu_tok[B] == qkv.shape[0]; max_N >= the longest sequence).  nq=None: every query -> o [total][H*64] packed like qkv,
    lse [H][total].  nq < max_N (the model's nq=2): compact o [(b*nq+q)][H*64], lse [(b*H+h)*nq+q]; rows of a sequence shorter
    than nq stay zero."""
    return _attention_fwd_varlen("attention_fwd_varlen", qkv, cu_tok, B, H, max_N, scale, nq, flags, None)


def _attention_fwd_varlen(name, qkv, cu_tok, B, H, max_N, scale, nq, flags, drop):
    """the packed forward; ``drop``: None (pa_attention_fwd_varlen) or the checked (seed, site, t) of pa_attention_fwd_varlen_dropout"""
    dtype = PA_DTYPE[qkv.dtype]
    total, D = qkv.shape[0], H * 64
    if qkv.dim() != 2 or qkv.shape[1] != 3 * D or cu_tok.dim() != 1 or cu_tok.numel() != B + 1 or not 1 <= max_N <= total:
        raise _lib.PasstAmdError(f"{name}: qkv {tuple(qkv.shape)}, cu_tok {tuple(cu_tok.shape)}, B={B}, H={H}, max_N={max_N}")
    if nq is None or nq >= max_N:
        nq = max_N
        o = torch.empty((total, D), device=qkv.device, dtype=qkv.dtype)
        lse = torch.empty((H, total), device=qkv.device, dtype=torch.float32)
        work = None
    else:
        if nq < 1:
            raise _lib.PasstAmdError(f"{name}: nq must be >= 1")
        o = torch.zeros((B * nq, D), device=qkv.device, dtype=qkv.dtype)
        lse = torch.zeros((B * H * nq,), device=qkv.device, dtype=torch.float32)
        work = 4.0 * nq * total * 64 * H
    # executed FLOPs of the all-queries form depend on the lengths, which live on the device: the per-launch profile files the
    # upper bound B * max_N^2 (bench_kernels.py reports the exact figure from its host copy of the lengths)
    work = work if work is not None else 4.0 * max_N * max_N * 64 * B * H
    if drop is None:
        _timed("attn_fwd", work,
               lambda: check(_lib.load().pa_attention_fwd_varlen(_p(qkv, None, True), qkv.stride(0), _p(o), o.stride(0), _p(lse),
                                                                 _p(cu_tok, torch.int32), B, H, max_N, nq, scale, dtype, flags, _stream()),
                             "pa_attention_fwd_varlen"))
    else:
        seed, site, t = drop
        _timed("attn_fwd_drop", work,
               lambda: check(_lib.load().pa_attention_fwd_varlen_dropout(_p(qkv, None, True), qkv.stride(0), _p(o), o.stride(0), _p(lse),
                                                                         _p(cu_tok, torch.int32), B, H, max_N, nq, scale, dtype, flags,
                                                                         _p(seed), site, t, _stream()),
                             "pa_attention_fwd_varlen_dropout"))
    return o, lse


def _f32_out(name, out, shape, device):
    """``out``, which must hold as many elements as ``shape``, or a fresh f32 tensor of that shape"""
    n = int(np.prod(shape))
    if out is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    if out.numel() != n:
        raise _lib.PasstAmdError(f"{name}: out has {out.numel()} elements, expected {n}")
    return out


def _packed_ok(qkv, cu_tok, B, H, max_N):
    """the shapes every packed attention entry asks of qkv [total][3*H*64], cu_tok [B + 1] and max_N"""
    return qkv.dim() == 2 and qkv.shape[1] == 3 * H * 64 and cu_tok.dim() == 1 and cu_tok.numel() == B + 1 and 1 <= max_N <= qkv.shape[0]


def _packed_nq(name, nq, lse, B, H, max_N, total, do_compact=False, lse_optional=False):
    """The nq a packed entry hands to the library: max_N stands for every query (lse [H][total]), a smaller one for the compact
    prefix form (lse [(b*H+h)*nq+q], the only one a compact d_o goes with).  Checks lse's size against it."""
    if nq is None or nq >= max_N:
        nq, nlse = max_N, H * total
        if do_compact:
            raise _lib.PasstAmdError(f"{name}: do_compact needs nq < max_N")
    else:
        if nq < 1:
            raise _lib.PasstAmdError(f"{name}: nq must be >= 1")
        nlse = B * H * nq
    if not (lse is None and lse_optional) and lse.numel() != nlse:
        raise _lib.PasstAmdError(f"{name}: lse has {lse.numel()} elements, expected {nlse}")
    return nq


def attention_probs(qkv, lse, B, H, N, scale, nq=None, head_mean=False, flags=0, out=None):
    """The attention probabilities softmax(q k^T * scale) of the attention_fwd call that made ``lse`` (same qkv, nq, flags): f32
    (B, H, nq, N), or (B, 1, nq, N) = the mean over heads with ``head_mean``.  out: an f32 tensor of that many elements to write
    instead of a fresh one (tests put guard rows behind it)."""
    dtype = PA_DTYPE[qkv.dtype]
    nq = N if nq is None else nq
    Ho = 1 if head_mean else H
    if qkv.dim() != 2 or qkv.shape[0] != B * N or qkv.shape[1] != 3 * H * 64 or lse.numel() != B * H * nq or not 1 <= nq <= N:
        raise _lib.PasstAmdError(f"attention_probs: qkv {tuple(qkv.shape)}, lse {tuple(lse.shape)}, B={B}, H={H}, N={N}, nq={nq}")
    out = _f32_out("attention_probs", out, (B, Ho, nq, N), qkv.device)
    _timed("attn_probs", 4.0 * out.numel(),
           lambda: check(_lib.load().pa_attention_probs(_p(qkv, None, True), qkv.stride(0), _p(lse, torch.float32), _p(out, torch.float32),
                                                        None, None, B, H, N, nq, int(bool(head_mean)), scale, dtype, flags, _stream()),
                         "pa_attention_probs"))
    return out.view(B, Ho, nq, N)


def attention_probs_offsets(ntok, H_out, nq=None):
    """Host layout of the packed attention maps: sequence b of ntok[b] tokens owns H_out * min(nq, ntok[b]) * ntok[b] floats, the
    sequences back to back.  Returns (int64 numpy array of len(ntok) element offsets, total elements).  nq=None: every query."""
    n = np.asarray(ntok, dtype=np.int64).reshape(-1)
    if n.size == 0 or (n < 1).any() or H_out < 1 or (nq is not None and nq < 1):
        raise ValueError(f"attention_probs_offsets: ntok={list(n)}, H_out={H_out}, nq={nq}")
    rows = n if nq is None else np.minimum(n, int(nq))
    size = int(H_out) * rows * n
    off = np.zeros(n.size, dtype=np.int64)
    np.cumsum(size[:-1], out=off[1:])
    return off, int(size.sum())


def attention_probs_varlen(qkv, lse, cu_tok, out_off, total_out, B, H, max_N, scale, nq=None, head_mean=False, flags=0, out=None):
    """Packed sequences (attention_fwd_varlen's qkv / cu_tok / lse for the same nq): one flat f32 buffer of ``total_out`` elements,
    sequence b dense at out_off[b] as [H or 1][min(nq, N_b)][N_b] (out_off: B int64 on the device, attention_probs_offsets)."""
    dtype = PA_DTYPE[qkv.dtype]
    total = qkv.shape[0]
    if not _packed_ok(qkv, cu_tok, B, H, max_N) or out_off.dim() != 1 or out_off.numel() != B:
        raise _lib.PasstAmdError(f"attention_probs_varlen: qkv {tuple(qkv.shape)}, cu_tok {tuple(cu_tok.shape)}, out_off "
                                 f"{tuple(out_off.shape)}, B={B}, H={H}, max_N={max_N}")
    nq = _packed_nq("attention_probs_varlen", nq, lse, B, H, max_N, total)
    out = _f32_out("attention_probs_varlen", out, (total_out,), qkv.device)
    _timed("attn_probs", 4.0 * total_out,
           lambda: check(_lib.load().pa_attention_probs(_p(qkv, None, True), qkv.stride(0), _p(lse, torch.float32), _p(out, torch.float32),
                                                        _p(cu_tok, torch.int32), _p(out_off, torch.int64), B, H, max_N, nq,
                                                        int(bool(head_mean)), scale, dtype, flags, _stream()), "pa_attention_probs"))
    return out.view(-1)


ATTN_PGRAD_GRAD, ATTN_PGRAD_CAM = 0, 1      # include/passt_amd.h PA_ATTN_PGRAD_*


def _pgrad_d_o(name, d_o, qkv, H, rows_tok, rows_compact, do_compact):
    rows = rows_compact if do_compact else rows_tok
    if d_o.dim() != 2 or d_o.shape[1] != H * 64 or d_o.shape[0] != rows or d_o.dtype != qkv.dtype or d_o.stride(1) != 1:
        raise _lib.PasstAmdError(f"{name}: d_o {tuple(d_o.shape)} {d_o.dtype} for {rows} rows of {H * 64} ({qkv.dtype}, "
                                 f"do_compact={bool(do_compact)})")


def attention_probs_grad(qkv, lse, d_o, B, H, N, scale, nq=None, head_mean=False, mode=ATTN_PGRAD_GRAD, do_compact=False, flags=0,
                         out=None):
    """The gradient with respect to the attention probabilities of the attention_fwd call on ``qkv``, from ``d_o``, the gradient of
    that call's output (what attention_bwd reads): f32 (B, H, nq, N).  mode=ATTN_PGRAD_GRAD: the gradient itself, ``lse`` may be None.
    mode=ATTN_PGRAD_CAM: max(probability * gradient, 0), with ``head_mean`` its mean over heads (B, 1, nq, N); ``lse`` as for
    attention_probs.  d_o: [B*N][H*64] (token rows; only rows q < nq of a sequence are read), or with ``do_compact`` [B*nq][H*64].
    out: an f32 tensor of that many elements to write instead of a fresh one (tests put guard rows behind it)."""
    dtype = PA_DTYPE[qkv.dtype]
    nq = N if nq is None else nq
    Ho = 1 if head_mean else H
    cam = mode == ATTN_PGRAD_CAM
    if qkv.dim() != 2 or qkv.shape[0] != B * N or qkv.shape[1] != 3 * H * 64 or not 1 <= nq <= N or \
            (lse is None if cam else head_mean) or (lse is not None and lse.numel() != B * H * nq):
        raise _lib.PasstAmdError(f"attention_probs_grad: qkv {tuple(qkv.shape)}, lse {None if lse is None else tuple(lse.shape)}, "
                                 f"B={B}, H={H}, N={N}, nq={nq}, mode={mode}, head_mean={head_mean}")
    _pgrad_d_o("attention_probs_grad", d_o, qkv, H, B * N, B * nq, do_compact)
    out = _f32_out("attention_probs_grad", out, (B, Ho, nq, N), qkv.device)
    _timed("attn_probs_grad", 4.0 * out.numel(),
           lambda: check(_lib.load().pa_attention_probs_grad(_p(qkv, None, True), qkv.stride(0), None if lse is None else _p(lse, torch.float32),
                                                             _p(d_o, qkv.dtype, True), d_o.stride(0), int(bool(do_compact)),
                                                             _p(out, torch.float32), None, None, B, H, N, nq, int(bool(head_mean)),
                                                             int(mode), scale, dtype, flags, _stream()), "pa_attention_probs_grad"))
    return out.view(B, Ho, nq, N)


def attention_probs_grad_varlen(qkv, lse, d_o, cu_tok, out_off, total_out, B, H, max_N, scale, nq=None, head_mean=False,
                                mode=ATTN_PGRAD_GRAD, do_compact=False, flags=0, out=None):
    """attention_probs_grad over packed sequences, in attention_probs_varlen's output layout: one flat f32 buffer of ``total_out``
    elements, sequence b dense at out_off[b] as [H or 1][min(nq, N_b)][N_b].  d_o: [total][H*64] packed like qkv's rows, or with
    ``do_compact`` (nq < max_N) [B*nq][H*64]."""
    dtype = PA_DTYPE[qkv.dtype]
    total = qkv.shape[0]
    cam = mode == ATTN_PGRAD_CAM
    if not _packed_ok(qkv, cu_tok, B, H, max_N) or out_off.dim() != 1 or out_off.numel() != B or (lse is None if cam else head_mean):
        raise _lib.PasstAmdError(f"attention_probs_grad_varlen: qkv {tuple(qkv.shape)}, cu_tok {tuple(cu_tok.shape)}, out_off "
                                 f"{tuple(out_off.shape)}, B={B}, H={H}, max_N={max_N}, mode={mode}, head_mean={head_mean}")
    nq = _packed_nq("attention_probs_grad_varlen", nq, lse, B, H, max_N, total, do_compact, lse_optional=True)
    _pgrad_d_o("attention_probs_grad_varlen", d_o, qkv, H, total, B * nq, do_compact)
    out = _f32_out("attention_probs_grad_varlen", out, (total_out,), qkv.device)
    _timed("attn_probs_grad", 4.0 * total_out,
           lambda: check(_lib.load().pa_attention_probs_grad(_p(qkv, None, True), qkv.stride(0), None if lse is None else _p(lse, torch.float32),
                                                             _p(d_o, qkv.dtype, True), d_o.stride(0), int(bool(do_compact)),
                                                             _p(out, torch.float32), _p(cu_tok, torch.int32), _p(out_off, torch.int64), B, H,
                                                             max_N, nq, int(bool(head_mean)), int(mode), scale, dtype, flags, _stream()),
                         "pa_attention_probs_grad"))
    return out.view(-1)


ATTN_ROLLOUT_ATTN, ATTN_ROLLOUT_CAM = 0, 1     # include/passt_amd.h PA_ATTN_ROLLOUT_*
ATTN_ROLLOUT_MAX_ROWS = 4                       # PA_ATTN_ROLLOUT_MAX_ROWS


def _rollout_launch(name, qkv, lse, d_o, r_in, out, cu_tok, total, B, H, N, nq, nr, mode, slices, a, b, g_scale, scale, do_compact, flags):
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(r_in)
    elif out.shape != r_in.shape or out.dtype != torch.float32 or \
            (out.data_ptr() < r_in.data_ptr() + r_in.numel() * 4 and r_in.data_ptr() < out.data_ptr() + out.numel() * 4):
        raise _lib.PasstAmdError(f"{name}: out must be an f32 tensor of r_in's shape {tuple(r_in.shape)} that shares no byte with it, got "
                                 f"{tuple(out.shape)} {out.dtype}")
    need = lib.pa_attention_rollout_ws_floats(total, B, N, nq, nr, slices)
    if need < 0:
        check(int(need), "pa_attention_rollout_ws_floats")
    ws = torch.empty(need, device=qkv.device, dtype=torch.float32) if need else None
    _timed("attn_rollout", (8.0 if mode == ATTN_ROLLOUT_CAM else 4.0) * min(nq, N) * total * 64 * H,
           lambda: check(lib.pa_attention_rollout(_p(qkv, None, True), qkv.stride(0), _p(lse, torch.float32),
                                                  None if d_o is None else _p(d_o, qkv.dtype, True), 0 if d_o is None else d_o.stride(0),
                                                  int(bool(do_compact)), _p(r_in, torch.float32), _p(out, torch.float32),
                                                  _p(ws, torch.float32), None if cu_tok is None else _p(cu_tok, torch.int32), total, B, H,
                                                  N, nq, nr, int(mode), int(slices), a, b, g_scale, scale, PA_DTYPE[qkv.dtype], flags,
                                                  _stream()), "pa_attention_rollout"))
    return out


def attention_rollout(qkv, lse, r_in, B, H, N, scale, a, b, nq=None, d_o=None, mode=ATTN_ROLLOUT_ATTN, g_scale=1.0, do_compact=False,
                      flags=0, slices=0, out=None):
    """One rollout step on row vectors, without the attention map: out[b, j] = a * r_in[b, j] + b * (r_in[b, j, :nq] @ M_b), f32
    (B, nr, N), with M the mean over heads of the attention probabilities of the attention_fwd call that made ``lse`` (same qkv, nq,
    flags; mode=ATTN_ROLLOUT_ATTN) or of max(probability * g_scale * gradient, 0) (ATTN_ROLLOUT_CAM; ``d_o`` / ``do_compact`` as for
    attention_probs_grad).  Query rows at or behind nq contribute nothing.  slices: 0 = the library cuts the query tiles by B, N and
    the device's CU count, > 0 = that many slices (tests).  out: another f32 tensor of r_in's shape to write instead of a fresh one."""
    nq = N if nq is None else nq
    cam = mode == ATTN_ROLLOUT_CAM
    if qkv.dim() != 2 or qkv.shape[0] != B * N or qkv.shape[1] != 3 * H * 64 or not 1 <= nq <= N or lse.numel() != B * H * nq or \
            r_in.dim() != 3 or r_in.shape[0] != B or r_in.shape[2] != N or not 1 <= r_in.shape[1] <= ATTN_ROLLOUT_MAX_ROWS or \
            (d_o is None) == cam or (do_compact and not cam):
        raise _lib.PasstAmdError(f"attention_rollout: qkv {tuple(qkv.shape)}, lse {tuple(lse.shape)}, r_in {tuple(r_in.shape)}, B={B}, "
                                 f"H={H}, N={N}, nq={nq}, mode={mode}, d_o {'given' if d_o is not None else 'missing'}")
    if cam:
        _pgrad_d_o("attention_rollout", d_o, qkv, H, B * N, B * nq, do_compact)
    return _rollout_launch("attention_rollout", qkv, lse, d_o, r_in, out, None, B * N, B, H, N, nq, r_in.shape[1], mode, slices, a, b,
                           g_scale, scale, do_compact, flags)


def attention_rollout_varlen(qkv, lse, r_in, cu_tok, B, H, max_N, scale, a, b, nq=None, d_o=None, mode=ATTN_ROLLOUT_ATTN, g_scale=1.0,
                             do_compact=False, flags=0, slices=0, out=None):
    """attention_rollout over packed sequences (attention_fwd_varlen's qkv / cu_tok / lse for the same nq): r_in and the result are
    f32 (nr, total) buffers read as one flat array in which sequence b's dense (nr, N_b) block starts at float nr * cu_tok[b] -- NOT
    rows of length total (rollout_views cuts it).  Every sequence gets what attention_rollout gives it alone with the same number of
    query tiles per slice."""
    total = qkv.shape[0]
    cam = mode == ATTN_ROLLOUT_CAM
    if not _packed_ok(qkv, cu_tok, B, H, max_N) or r_in.dim() != 2 or r_in.shape[1] != total or \
            not 1 <= r_in.shape[0] <= ATTN_ROLLOUT_MAX_ROWS or (d_o is None) == cam or (do_compact and not cam):
        raise _lib.PasstAmdError(f"attention_rollout_varlen: qkv {tuple(qkv.shape)}, cu_tok {tuple(cu_tok.shape)}, r_in {tuple(r_in.shape)}, "
                                 f"B={B}, H={H}, max_N={max_N}, mode={mode}, d_o {'given' if d_o is not None else 'missing'}")
    nq = _packed_nq("attention_rollout_varlen", nq, lse, B, H, max_N, total, do_compact)
    if cam:
        _pgrad_d_o("attention_rollout_varlen", d_o, qkv, H, total, B * nq, do_compact)
    return _rollout_launch("attention_rollout_varlen", qkv, lse, d_o, r_in, out, cu_tok, total, B, H, max_N, nq, r_in.shape[0], mode, slices,
                           a, b, g_scale, scale, do_compact, flags)


def rollout_views(r, ntok):
    """The packed rollout buffer (nr, total) -> a list of views: sequence b's (nr, N_b)."""
    nr, flat, out, o = r.shape[0], r.view(-1), [], 0
    for n in ntok:
        n = int(n)
        out.append(flat[o:o + nr * n].view(nr, n))
        o += nr * n
    return out


def attention_bwd(qkv, o, d_o, lse, B, H, N, scale, nq=None, flags=0):
    """dqkv [B*N][3D]; with nq < N (o, d_o, lse compact) the Q third is zero outside the first nq rows."""
    dtype = PA_DTYPE[qkv.dtype]
    nq = N if nq is None else nq
    dqkv = torch.empty_like(qkv)
    lib = _lib.load()
    delta = torch.empty(lib.pa_attention_bwd_ws_floats(B, H, nq), device=lse.device, dtype=torch.float32)
    if nq < N:
        es = qkv.element_size()
        check(lib.pa_zero2d(_p(dqkv), dqkv.stride(0) * es, H * 64 * es, B * N, _stream()), "pa_zero2d")
    _timed("attn_bwd", 10.0 * nq * N * 64 * B * H,      # five N x N x 64 products: S, dP, dV, dK, dQ
           lambda: check(lib.pa_attention_bwd(_p(qkv, None, True), qkv.stride(0), _p(o, qkv.dtype, True), _p(d_o, qkv.dtype, True),
                                              o.stride(0), _p(lse, torch.float32), _p(delta), _p(dqkv), dqkv.stride(0), B, H, N, nq,
                                              scale, dtype, flags | _ATTN_BWD_FORCE, _stream()), "pa_attention_bwd"))
    return dqkv


# ---- attention dropout: the mask is a pure function of (seed, site, sequence x head, query, key), include/passt_amd.h ----------
def attn_drop_t(p):
    """t = round(256 p) of a dropout rate: 0 = no dropout (the plain entries), 1..255 = active with the effective rate t / 256
    (keep = 1 - t / 256; kept probabilities are scaled by 1 / keep, so the expectation is exact for the rate actually applied).
    A rate so large that t > 255 is a ValueError."""
    p = float(p)
    if not (p >= 0.0):
        raise ValueError(f"attention dropout rate {p!r} is negative or not a number")
    t = int(math.floor(256.0 * p + 0.5))
    if t > 255:
        raise ValueError(f"attention dropout rate {p!r} rounds to {t}/256: the largest rate the fused attention applies is 255/256")
    return t


def attn_drop_keep(t):
    return 1.0 - t / 256.0


def _drop_seed(seed, device, what):
    """two words in device memory (int32 storage, read as uint32)"""
    if not torch.is_tensor(seed) or seed.numel() != 2 or seed.dtype not in (torch.int32, torch.uint32) or seed.device != device \
            or not seed.is_contiguous():
        raise _lib.PasstAmdError(f"{what}: seed must be a contiguous (2,) int32 tensor on {device}")
    return seed


def _drop_t(t, what):
    if not isinstance(t, int) or not 1 <= t <= 255:
        raise ValueError(f"{what}: t must be an int in 1..255 (attn_drop_t of the rate), got {t!r}")
    return t


def attention_fwd_dropout(qkv, B, H, N, scale, seed, site, t, nq=None, flags=0):
    """attention_fwd with dropout on the probabilities: seed a (2,) int32 tensor on qkv's device, site the block index, t = attn_drop_t(p)
    in 1..255.  lse is that of the undropped softmax."""
    dtype = PA_DTYPE[qkv.dtype]
    nq = N if nq is None else nq
    _drop_seed(seed, qkv.device, "attention_fwd_dropout")
    _drop_t(t, "attention_fwd_dropout")
    o = torch.empty((B * nq, H * 64), device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty((B * H * nq,), device=qkv.device, dtype=torch.float32)
    _timed("attn_fwd_drop", 4.0 * nq * N * 64 * B * H,
           lambda: check(_lib.load().pa_attention_fwd_dropout(_p(qkv, None, True), qkv.stride(0), _p(o), o.stride(0), _p(lse), B, H, N, nq,
                                                              scale, dtype, flags, _p(seed), int(site), t, _stream()), "pa_attention_fwd_dropout"))
    return o, lse


def attention_bwd_dropout(qkv, o, d_o, lse, B, H, N, scale, seed, site, t, nq=None, flags=0):
    """attention_bwd for attention_fwd_dropout's o / lse under the same seed, site and t: always the dQ + dK/dV kernel pair."""
    dtype = PA_DTYPE[qkv.dtype]
    nq = N if nq is None else nq
    _drop_seed(seed, qkv.device, "attention_bwd_dropout")
    _drop_t(t, "attention_bwd_dropout")
    dqkv = torch.empty_like(qkv)
    lib = _lib.load()
    delta = torch.empty(lib.pa_attention_bwd_ws_floats(B, H, nq), device=lse.device, dtype=torch.float32)
    if nq < N:
        es = qkv.element_size()
        check(lib.pa_zero2d(_p(dqkv), dqkv.stride(0) * es, H * 64 * es, B * N, _stream()), "pa_zero2d")
    _timed("attn_bwd_drop", 14.0 * nq * N * 64 * B * H,     # the kernel pair forms S and dP twice: seven N x N x 64 products
           lambda: check(lib.pa_attention_bwd_dropout(_p(qkv, None, True), qkv.stride(0), _p(o, qkv.dtype, True), _p(d_o, qkv.dtype, True),
                                                      o.stride(0), _p(lse, torch.float32), _p(delta), _p(dqkv), dqkv.stride(0), B, H, N, nq,
                                                      scale, dtype, flags, _p(seed), int(site), t, _stream()), "pa_attention_bwd_dropout"))
    return dqkv


def attn_drop_seed_words(seed):
    """(s0, s1) Python ints < 2^32 from two ints or a (2,) tensor (int32 storage is read as uint32)"""
    if torch.is_tensor(seed):
        if seed.numel() != 2:
            raise ValueError(f"attention dropout seed: a (2,) tensor, got {tuple(seed.shape)}")
        seed = [int(v) for v in seed.detach().cpu().reshape(2).tolist()]
    s = tuple(int(v) & 0xFFFFFFFF if -2 ** 31 <= int(v) < 0 else int(v) for v in seed)
    if len(s) != 2 or not all(0 <= v < 2 ** 32 for v in s):
        raise ValueError(f"attention dropout seed: two ints in [0, 2^32), got {seed!r}")
    return s


def attn_drop_mask(seed, site, B, H, nq, N, p):
    """The keep mask the fused attention applies at dropout site ``site`` (the block index) under ``seed`` (two ints < 2^32 or a (2,)
    tensor) and the rate ``p`` (quantised: attn_drop_t): a CPU bool tensor (B, H, nq, N), True = kept.  Computed on the host from the
    rule the kernels compile (pa_attention_dropout_mask); multiply the probabilities by mask / (1 - attn_drop_t(p) / 256) to replay."""
    t = attn_drop_t(p)
    if t == 0:
        return torch.ones(B, H, nq, N, dtype=torch.bool)
    s0, s1 = attn_drop_seed_words(seed)
    out = torch.empty(B * H * nq * N, dtype=torch.uint8)
    check(_lib.load().pa_attention_dropout_mask(s0, s1, int(site), B * H, nq, N, t, out.data_ptr()), "pa_attention_dropout_mask")
    return out.view(B, H, nq, N).bool()


def attention_bwd_varlen(qkv, o, d_o, lse, cu_tok, B, H, max_N, scale, nq=None, flags=0, ws=None, out=None):
    """dqkv [total][3D] for packed sequences (attention_fwd_varlen's layouts: nq=None -> o / d_o [total][D], lse [H][total]; nq <
    max_N -> compact o / d_o [B*nq][D], lse [B*H*nq]).  Every row of dqkv is written: in the compact form the Q third is zero
    outside each sequence's first nq rows.  Always the dQ + dK/dV kernel pair.  ws / out: an f32 workspace / a [total][3D] tensor of
    qkv's dtype to use instead of fresh ones (tests put guard rows behind them)."""
    return _attention_bwd_varlen("attention_bwd_varlen", qkv, o, d_o, lse, cu_tok, B, H, max_N, scale, nq, flags, ws, out, None)


def _drop_site(site, what):
    if not isinstance(site, int) or isinstance(site, bool) or not 0 <= site < 65536:
        raise ValueError(f"{what}: site must be an int in 0..65535 (the block index), got {site!r}")
    return site


def attention_fwd_varlen_dropout(qkv, cu_tok, B, H, max_N, scale, seed, site, t, nq=None, flags=0):
    """attention_fwd_varlen with dropout on the probabilities (attention_fwd_dropout's seed / site / t).  Sequence b gets the mask the
    fixed entry gives sequence b of a batch: s = b*H + h, q and k the positions inside the sequence."""
    _drop_seed(seed, qkv.device, "attention_fwd_varlen_dropout")
    _drop_t(t, "attention_fwd_varlen_dropout")
    _drop_site(site, "attention_fwd_varlen_dropout")
    return _attention_fwd_varlen("attention_fwd_varlen_dropout", qkv, cu_tok, B, H, max_N, scale, nq, flags, (seed, site, t))


def attention_bwd_varlen_dropout(qkv, o, d_o, lse, cu_tok, B, H, max_N, scale, seed, site, t, nq=None, flags=0, ws=None, out=None):
    """attention_bwd_varlen for attention_fwd_varlen_dropout's o / lse under the same seed, site and t; same layouts, ws / out."""
    _drop_seed(seed, qkv.device, "attention_bwd_varlen_dropout")
    _drop_t(t, "attention_bwd_varlen_dropout")
    _drop_site(site, "attention_bwd_varlen_dropout")
    return _attention_bwd_varlen("attention_bwd_varlen_dropout", qkv, o, d_o, lse, cu_tok, B, H, max_N, scale, nq, flags, ws, out,
                                 (seed, site, t))


def _attention_bwd_varlen(name, qkv, o, d_o, lse, cu_tok, B, H, max_N, scale, nq, flags, ws, out, drop):
    """the packed backward; ``drop``: None (pa_attention_bwd_varlen) or the checked (seed, site, t) of pa_attention_bwd_varlen_dropout"""
    dtype = PA_DTYPE[qkv.dtype]
    total, D = qkv.shape[0], H * 64
    if qkv.dim() != 2 or qkv.shape[1] != 3 * D or cu_tok.dim() != 1 or cu_tok.numel() != B + 1 or not 1 <= max_N <= total:
        raise _lib.PasstAmdError(f"{name}: qkv {tuple(qkv.shape)}, cu_tok {tuple(cu_tok.shape)}, B={B}, H={H}, max_N={max_N}")
    if nq is None or nq >= max_N:
        nq, rows, nlse = max_N, total, H * total
    else:
        if nq < 1:
            raise _lib.PasstAmdError(f"{name}: nq must be >= 1")
        rows, nlse = B * nq, B * H * nq
    if o.shape != (rows, D) or d_o.shape != (rows, D) or lse.numel() != nlse or o.stride(0) != d_o.stride(0):
        raise _lib.PasstAmdError(f"{name}: o {tuple(o.shape)} / d_o {tuple(d_o.shape)} / lse {tuple(lse.shape)} for {rows} query rows")
    lib = _lib.load()
    need = lib.pa_attention_bwd_varlen_ws_floats(total, B, H, nq)
    if ws is None:
        ws = torch.empty(need, device=lse.device, dtype=torch.float32)
    elif ws.numel() < need:
        raise _lib.PasstAmdError(f"{name}: workspace of {ws.numel()} floats, {need} needed")
    dqkv = torch.empty_like(qkv) if out is None else out
    if dqkv.shape != qkv.shape or dqkv.dtype != qkv.dtype:
        raise _lib.PasstAmdError(f"{name}: out is {tuple(dqkv.shape)} {dqkv.dtype}, expected {tuple(qkv.shape)} {qkv.dtype}")
    # executed FLOPs depend on the lengths, which live on the device: the per-launch profile files the upper bound (see attention_fwd_varlen)
    work = nq * (max_N if rows == total else total / B) * 64 * B * H
    if drop is None:
        _timed("attn_bwd", 10.0 * work,
               lambda: check(lib.pa_attention_bwd_varlen(_p(qkv, None, True), qkv.stride(0), _p(o, qkv.dtype, True), _p(d_o, qkv.dtype, True),
                                                         o.stride(0), _p(lse, torch.float32), _p(ws, torch.float32), _p(dqkv, None, True), dqkv.stride(0),
                                                         _p(cu_tok, torch.int32), B, H, max_N, nq, scale, dtype, flags, _stream()),
                             "pa_attention_bwd_varlen"))
    else:
        seed, site, t = drop
        _timed("attn_bwd_drop", 14.0 * work,
               lambda: check(lib.pa_attention_bwd_varlen_dropout(_p(qkv, None, True), qkv.stride(0), _p(o, qkv.dtype, True),
                                                                 _p(d_o, qkv.dtype, True), o.stride(0), _p(lse, torch.float32),
                                                                 _p(ws, torch.float32), _p(dqkv, None, True), dqkv.stride(0),
                                                                 _p(cu_tok, torch.int32), B, H, max_N, nq, scale, dtype, flags, _p(seed), site, t,
                                                                 _stream()),
                             "pa_attention_bwd_varlen_dropout"))
    return dqkv


def gather_rows(x, idx_i32):
    """out[i] = x[idx[i]] for a 2-D (or 1-D) contiguous tensor."""
    n = idx_i32.numel()
    if x.is_cuda and x.is_contiguous() and x.data_ptr() % 4:          # rows move as 4-byte words: a 16-bit view at an odd element gets a copy
        x = x.clone()
    out = torch.empty((n,) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
    row_bytes = x.stride(0) * x.element_size()
    check(_lib.load().pa_gather_rows(_p(x), _p(idx_i32, torch.int32), n, row_bytes, _p(out), _stream()), "pa_gather_rows")
    return out


def scatter_rows_into_zeros(x_rows, idx_i32, n_rows):
    """zeros(n_rows, D) with out[idx[i]] = x_rows[i]"""
    out = torch.empty((n_rows,) + tuple(x_rows.shape[1:]), device=x_rows.device, dtype=x_rows.dtype)
    row_bytes = x_rows.stride(0) * x_rows.element_size()
    if x_rows.is_cuda and x_rows.is_contiguous() and x_rows.data_ptr() % 4:
        x_rows = x_rows.clone()
    lib = _lib.load()
    check(lib.pa_zero2d(_p(out), row_bytes, row_bytes, n_rows, _stream()), "pa_zero2d")
    check(lib.pa_scatter_rows(_p(x_rows), _p(idx_i32, torch.int32), idx_i32.numel(), row_bytes, _p(out), _stream()), "pa_scatter_rows")
    return out


def tail_inject(x_rows, idx_i32, n_rows, add0, add1, dtype):
    """(dx f32 [n_rows][D], its ``dtype`` copy): dx = add0 + add1 + scatter(x_rows at idx) with either addend optional ([n_rows][D]
    f32 or None) -- the gradient of the last block's full-rows output: what a caller injected at the last block's output (add0),
    the final norm's backward over all rows (add1) and the head's gradient on the prefix rows.  idx: strictly ascending.  In f32
    the copy is dx itself."""
    D = x_rows.shape[1]
    for a in (add0, add1):
        if a is not None and a.shape != (n_rows, D):
            raise _lib.PasstAmdError(f"tail_inject: an addend is {tuple(a.shape)}, expected {(n_rows, D)}")
    x_rows, add0, add1 = _aligned16(x_rows), _aligned16(add0), _aligned16(add1)
    dx = torch.empty((n_rows, D), device=x_rows.device, dtype=torch.float32)
    dx_lp = torch.empty((n_rows, D), device=x_rows.device, dtype=TORCH_DTYPE[dtype]) if dtype != PA_F32 else None
    check(_lib.load().pa_tail_inject(_p(x_rows, torch.float32), _p(idx_i32, torch.int32), idx_i32.numel(), _p(add0, torch.float32),
                                     _p(add1, torch.float32), _p(dx), _p(dx_lp), dtype, n_rows, D, _stream()), "pa_tail_inject")
    return dx, (dx if dtype == PA_F32 else dx_lp)


# ---- patch embedding -------------------------------------------------------------------------
def patch_gather(x, patch_f, patch_t, P, fstride, tstride, dtype):
    B, _, F, T = x.shape
    Np = patch_f.numel()
    cols = torch.empty((B * Np, P * P), device=x.device, dtype=TORCH_DTYPE[dtype])
    check(_lib.load().pa_patch_gather(_p(x, torch.float32), B, F, T, _p(patch_f, torch.int32), _p(patch_t, torch.int32), Np, P, fstride, tstride, _p(cols),
                                      dtype, _stream()), "pa_patch_gather")
    return cols


def patch_pos_table(bias, time_pos, freq_pos, patch_f, patch_t, toff, cls, dist, npe, tok):
    B, Ntok, D = tok.shape
    Np = patch_f.numel()
    Tpe, Fpe = time_pos.shape[-1], freq_pos.shape[-2]
    table = torch.empty((Np, D), device=tok.device, dtype=torch.float32)
    check(_lib.load().pa_patch_pos_table(_p(bias), _p(time_pos), Tpe, _p(freq_pos), Fpe, _p(patch_f), _p(patch_t),
                                         Np, toff, D, _p(table), _p(cls), _p(dist), _p(npe), _p(tok), B, Ntok,
                                         _stream()), "pa_patch_pos_table")
    return table


def patch_gather_varlen(x, row_clip, row_f, row_t, P, fstride, tstride, dtype):
    """cols [M][P*P] for the packed token rows of a ragged batch (prefix rows zero); index arrays: (M,) int32 on the device."""
    B, _, F, T = x.shape
    M = row_f.numel()
    if row_clip.numel() != M or row_t.numel() != M or M < 1:
        raise _lib.PasstAmdError("patch_gather_varlen: row_clip / row_f / row_t must have one entry per token row")
    cols = torch.empty((M, P * P), device=x.device, dtype=TORCH_DTYPE[dtype])
    check(_lib.load().pa_patch_gather_varlen(_p(x, torch.float32), B, F, T, _p(row_clip, torch.int32), _p(row_f, torch.int32),
                                             _p(row_t, torch.int32), M, P, fstride, tstride, _p(cols), dtype, _stream()),
          "pa_patch_gather_varlen")
    return cols


def patch_gather_windows(x, win_src, win_t0, win_len, row_win, row_f, row_t, P, fstride, tstride, dtype):
    """cols [M][P*P] for the packed token rows of sliding windows over the recordings x (B, 1, F, T): row r is the patch (row_f, row_t)
    of window row_win[r] = (recording win_src, first frame win_t0, win_len frames), read in place; prefix rows zero.  All index arrays:
    int32 on the device, (W,) per window and (M,) per token row."""
    B, _, F, T = x.shape
    W, M = win_src.numel(), row_f.numel()
    if win_t0.numel() != W or win_len.numel() != W or W < 1:
        raise _lib.PasstAmdError("patch_gather_windows: win_src / win_t0 / win_len must have one entry per window")
    if row_win.numel() != M or row_t.numel() != M or M < 1:
        raise _lib.PasstAmdError("patch_gather_windows: row_win / row_f / row_t must have one entry per token row")
    cols = torch.empty((M, P * P), device=x.device, dtype=TORCH_DTYPE[dtype])
    check(_lib.load().pa_patch_gather_windows(_p(x, torch.float32), B, F, T, _p(win_src, torch.int32), _p(win_t0, torch.int32),
                                              _p(win_len, torch.int32), W, _p(row_win, torch.int32), _p(row_f, torch.int32),
                                              _p(row_t, torch.int32), M, P, fstride, tstride, _p(cols), dtype, _stream()),
          "pa_patch_gather_windows")
    return cols


def window_pool(rows, offsets, mode="mean", act=None):
    """(W, C) f32 per-window rows -> (B, C): recording b pools its own rows offsets[b]:offsets[b + 1] (pa_window_pool: rows added in
    row order in f32, the mean divided by the recording's own count, the max started from its first row).  ``offsets``: B + 1 HOST
    integers (sequence / numpy / CPU tensor), checked here -- they start at 0, end at W and leave no recording empty (ValueError,
    nothing launched).  ``mode``: "mean" / "max"; ``act``: None or "sigmoid" (pool the sigmoid of the rows)."""
    if mode not in ("mean", "max"):
        raise ValueError(f"window_pool: mode must be 'mean' or 'max', got {mode!r}")
    if act not in (None, "sigmoid"):
        raise ValueError(f"window_pool: act must be None or 'sigmoid', got {act!r}")
    if torch.is_tensor(offsets) and offsets.is_cuda:
        raise ValueError("window_pool: offsets are host integers (they are checked before the launch)")
    off = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if rows.dim() != 2:
        raise ValueError(f"window_pool: expected (windows, columns) rows, got {tuple(rows.shape)}")
    W, Cc = rows.shape
    if off.size < 2 or off[0] != 0 or off[-1] != W or (np.diff(off) < 1).any():
        raise ValueError(f"window_pool: offsets must rise from 0 to the {W} rows with at least one row per recording, got {off.tolist()}")
    B = off.size - 1
    out = torch.empty((B, Cc), device=rows.device, dtype=torch.float32)
    off_dev = upload_small(off.astype(np.int32), rows.device)
    check(_lib.load().pa_window_pool(_p(rows, torch.float32), W, Cc, _p(off_dev, torch.int32), B,
                                     _lib.POOL_MAX if mode == "max" else _lib.POOL_MEAN,
                                     _lib.POOL_ACT_SIGMOID if act == "sigmoid" else _lib.POOL_ACT_NONE, _p(out), _stream()), "pa_window_pool")
    return out


def patch_pos_table_varlen(bias, time_pos, freq_pos, row_f, row_t, cls, dist, npe):
    """table [M][D] f32: positional rows + conv bias under the patch rows, cls / dist + their position rows under the prefix rows."""
    M, D = row_f.numel(), bias.numel()
    Tpe, Fpe = time_pos.shape[-1], freq_pos.shape[-2]
    if row_t.numel() != M or M < 1 or time_pos.numel() != D * Tpe or freq_pos.numel() != D * Fpe or npe.numel() != 2 * D:
        raise _lib.PasstAmdError("patch_pos_table_varlen: inconsistent shapes")
    table = torch.empty((M, D), device=bias.device, dtype=torch.float32)
    check(_lib.load().pa_patch_pos_table_varlen(_p(bias, torch.float32), _p(time_pos, torch.float32), Tpe, _p(freq_pos, torch.float32), Fpe,
                                                _p(row_f, torch.int32), _p(row_t, torch.int32), M, D, _p(table), _p(cls, torch.float32),
                                                _p(dist, torch.float32), _p(npe, torch.float32), _stream()), "pa_patch_pos_table_varlen")
    return table


def patch_bwd(dtok, patch_f, patch_t, toff, Tpe, Fpe, d_cls, d_dist, d_npe, d_bias, d_tpos, d_fpos, dtype,
              accumulate=False):
    B, Ntok, D = dtok.shape
    Np = patch_f.numel()
    dtok = _aligned16(dtok)
    gsum = torch.empty((Ntok, D), device=dtok.device, dtype=torch.float32) if d_cls is not None else None   # all d_* None: dpatch only
    dpatch = torch.empty((B * Np, D), device=dtok.device, dtype=TORCH_DTYPE[dtype])
    check(_lib.load().pa_patch_bwd(_p(dtok), B, Ntok, D, _p(patch_f), _p(patch_t), Np, toff, Tpe, Fpe, _p(gsum),
                                   _p(d_cls), _p(d_dist), _p(d_npe), _p(d_bias), _p(d_tpos), _p(d_fpos),
                                   int(accumulate), _p(dpatch), dtype, _stream()), "pa_patch_bwd")
    return dpatch


def patch_input_bwd(dcols, patch_f, patch_t, B, F, T, P, fstride, tstride, out=None):
    """dx [B][1][F][T] f32 = fold (col2im) of dcols [B*Np][P*P] (f32 or bf16) over the kept patches: the gradient w.r.t. the input
    spectrogram of patch_gather.  Every element is written (0 where no kept patch covers the pixel); deterministic (no atomics).
    out: an existing (B, 1, F, T) f32 tensor to overwrite."""
    Np = patch_f.numel()
    if dcols.dim() != 2 or dcols.shape[0] != B * Np or dcols.shape[1] != P * P or patch_t.numel() != Np or F < P or T < P:
        raise _lib.PasstAmdError(f"patch_input_bwd: dcols {tuple(dcols.shape)} for B={B}, Np={Np}, P={P}, F={F}, T={T}")
    lib = _lib.load()
    dx = torch.empty((B, 1, F, T), device=dcols.device, dtype=torch.float32) if out is None else out
    if dx.shape != (B, 1, F, T):
        raise _lib.PasstAmdError(f"patch_input_bwd: out is {tuple(dx.shape)}, expected {(B, 1, F, T)}")
    grid = torch.empty(lib.pa_patch_input_bwd_ws_ints(F, T, P, fstride, tstride), device=dcols.device, dtype=torch.int32)
    dcols = _aligned16(dcols)
    return _into_aligned16(dx, lambda: torch.empty_like(dx), lambda o: check(
        lib.pa_patch_input_bwd(_p(dcols), PA_DTYPE[dcols.dtype], B, Np, _p(patch_f, torch.int32), _p(patch_t, torch.int32), P, fstride, tstride,
                               F, T, _p(grid, torch.int32), _p(o, torch.float32), _stream()), "pa_patch_input_bwd"))


def patch_input_bwd_varlen(dcols, cu_tok, B, F, T_max, P, fstride, tstride, out=None):
    """dx [B][1][F][T_max] f32 = fold of the packed dcols [M][P*P] (f32 or bf16; the rows under the prefix tokens are not read) over
    every clip's own patches: the gradient w.r.t. the input of patch_gather_varlen.  Every element is written, 0 behind a clip's last
    patch column; deterministic.  out: an existing (B, 1, F, T_max) f32 tensor to overwrite."""
    if dcols.dim() != 2 or dcols.shape[1] != P * P or cu_tok.dim() != 1 or cu_tok.numel() != B + 1 or F < P or T_max < P:
        raise _lib.PasstAmdError(f"patch_input_bwd_varlen: dcols {tuple(dcols.shape)}, cu_tok {tuple(cu_tok.shape)} for B={B}, P={P}, F={F}, T={T_max}")
    dx = torch.empty((B, 1, F, T_max), device=dcols.device, dtype=torch.float32) if out is None else out
    if dx.shape != (B, 1, F, T_max):
        raise _lib.PasstAmdError(f"patch_input_bwd_varlen: out is {tuple(dx.shape)}, expected {(B, 1, F, T_max)}")
    dcols = _aligned16(dcols)
    return _into_aligned16(dx, lambda: torch.empty_like(dx), lambda o: check(
        _lib.load().pa_patch_input_bwd_varlen(_p(dcols), PA_DTYPE[dcols.dtype], _p(cu_tok, torch.int32), B, P, fstride, tstride, F, T_max,
                                              _p(o, torch.float32), _stream()), "pa_patch_input_bwd_varlen"))


def patch_bwd_varlen(dtok, cu_tok, B, Tpe, Fpe, d_cls, d_dist, d_npe, d_bias, d_tpos, d_fpos, accumulate=False):
    """Positional / prefix-token / conv-bias gradients from the packed dtok [M][D] f32 (overwritten or accumulated); deterministic."""
    if dtok.dim() != 2 or cu_tok.dim() != 1 or cu_tok.numel() != B + 1:
        raise _lib.PasstAmdError(f"patch_bwd_varlen: dtok {tuple(dtok.shape)}, cu_tok {tuple(cu_tok.shape)} for B={B}")
    M, D = dtok.shape
    check(_lib.load().pa_patch_bwd_varlen(_p(dtok, torch.float32), M, D, _p(cu_tok, torch.int32), B, Tpe, Fpe, _p(d_cls), _p(d_dist), _p(d_npe),
                                          _p(d_bias), _p(d_tpos), _p(d_fpos), int(accumulate), _stream()), "pa_patch_bwd_varlen")


def patch_input_bwd_rows(dcols, slot, F, T_max, P, fstride, tstride, out=None):
    """patch_input_bwd_varlen for a packed batch with Patchout: the kept patches that cover a pixel are found through ``slot``, the
    (B, Fg, Tg) int32 device table of their packed rows (-1: no kept patch there).  dx [B][1][F][T_max] f32, every element written,
    exactly 0 where no kept patch covers it; deterministic.  out: an existing (B, 1, F, T_max) f32 tensor to overwrite."""
    if dcols.dim() != 2 or dcols.shape[1] != P * P or slot.dim() != 3 or F < P or T_max < P or slot.shape[1] != (F - P) // fstride + 1 \
            or slot.shape[2] < 1:
        raise _lib.PasstAmdError(f"patch_input_bwd_rows: dcols {tuple(dcols.shape)}, slot {tuple(slot.shape)} for P={P}, F={F}, T={T_max}")
    B, _, Tg = slot.shape
    dx = torch.empty((B, 1, F, T_max), device=dcols.device, dtype=torch.float32) if out is None else out
    if dx.shape != (B, 1, F, T_max):
        raise _lib.PasstAmdError(f"patch_input_bwd_rows: out is {tuple(dx.shape)}, expected {(B, 1, F, T_max)}")
    dcols = _aligned16(dcols)
    return _into_aligned16(dx, lambda: torch.empty_like(dx), lambda o: check(
        _lib.load().pa_patch_input_bwd_rows(_p(dcols), PA_DTYPE[dcols.dtype], dcols.shape[0], _p(slot, torch.int32), B, Tg, P, fstride, tstride,
                                            F, T_max, _p(o, torch.float32), _stream()), "pa_patch_input_bwd_rows"))


def patch_bwd_rows(dtok, slot, cu_tok, toff, Tpe, Fpe, d_cls, d_dist, d_npe, d_bias, d_tpos, d_fpos, accumulate=False):
    """patch_bwd_varlen for a packed batch with Patchout: ``slot`` as in patch_input_bwd_rows, ``toff`` the (B,) int32 device array of
    the clips' offsets into the time embedding.  Overwritten or accumulated; deterministic."""
    if dtok.dim() != 2 or slot.dim() != 3 or slot.shape[1] != Fpe or slot.shape[2] < 1 or cu_tok.dim() != 1 \
            or cu_tok.numel() != slot.shape[0] + 1 or toff.dim() != 1 or toff.numel() != slot.shape[0]:
        raise _lib.PasstAmdError(f"patch_bwd_rows: dtok {tuple(dtok.shape)}, slot {tuple(slot.shape)}, cu_tok {tuple(cu_tok.shape)}, "
                                 f"toff {tuple(toff.shape)} for Fpe={Fpe}")
    M, D = dtok.shape
    B, _, Tg = slot.shape
    check(_lib.load().pa_patch_bwd_rows(_p(dtok, torch.float32), M, D, _p(slot, torch.int32), _p(cu_tok, torch.int32), _p(toff, torch.int32), B, Tg,
                                        Tpe, Fpe, _p(d_cls), _p(d_dist), _p(d_npe), _p(d_bias), _p(d_tpos), _p(d_fpos), int(accumulate), _stream()),
          "pa_patch_bwd_rows")


# ---- head / loss -----------------------------------------------------------------------------
def head_pre_fwd(x, norm_g, norm_b, eps_norm, hg, hb, eps_head):
    B, Ntok, D = x.shape
    feat = torch.empty((B, D), device=x.device, dtype=torch.float32)
    hn = torch.empty((B, D), device=x.device, dtype=torch.float32)
    stats = torch.empty((B, 6), device=x.device, dtype=torch.float32)
    check(_lib.load().pa_head_pre_fwd(_p(x), B, Ntok, D, _p(norm_g), _p(norm_b), eps_norm, _p(hg), _p(hb), eps_head,
                                      _p(feat), _p(hn), _p(stats), _stream()), "pa_head_pre_fwd")
    return feat, hn, stats


def head_pre_bwd(dhn, dfeat, x, feat, norm_g, hg, stats):
    B, Ntok, D = x.shape
    dx = torch.empty((B, Ntok, D), device=x.device, dtype=torch.float32)
    part = torch.empty((B, 4 * D), device=x.device, dtype=torch.float32)
    check(_lib.load().pa_head_pre_bwd(_p(dhn), _p(dfeat), _p(x), _p(feat), B, Ntok, D, _p(norm_g), _p(hg), _p(stats),
                                      _p(dx), _p(part), _stream()), "pa_head_pre_bwd")
    return dx, part


def linear_f32_fwd(x, W, b):
    B, D = x.shape
    Cc = W.shape[0]
    y = torch.empty((B, Cc), device=x.device, dtype=torch.float32)
    check(_lib.load().pa_linear_f32_fwd(_p(x, torch.float32), _p(W, torch.float32), _p(b, torch.float32), _p(y), B, Cc, D, _stream()), "pa_linear_f32_fwd")
    return y


def linear_f32_bwd(dy, x, W, dW, db, accumulate=False):
    B, Cc = dy.shape
    D = x.shape[1]
    dx = torch.empty((B, D), device=x.device, dtype=torch.float32)
    check(_lib.load().pa_linear_f32_bwd(_p(dy, torch.float32), _p(x, torch.float32), _p(W, torch.float32), _p(dx), _p(dW, torch.float32), _p(db, torch.float32), int(accumulate), B, Cc, D,
                                        _stream()), "pa_linear_f32_bwd")
    return dx


def bce_fwd_bwd(logits, target, grad_scale=1.0, out=None):
    """out: (loss [1], dlogits [>= B * C], ws [>= 1 + ceil(B * C / 256)]) f32 buffers to reuse instead of allocating"""
    B, Cc = logits.shape
    if out is not None:
        loss, dlogits, ws = out
        if loss.numel() < 1 or dlogits.numel() < B * Cc or ws.numel() < 1 + (B * Cc + 255) // 256:
            raise _lib.PasstAmdError("bce_fwd_bwd: the buffers in `out` are too small")
    else:
        loss = torch.empty(1, device=logits.device, dtype=torch.float32)
        dlogits = torch.empty_like(logits)
        ws = torch.empty(1 + (B * Cc + 255) // 256, device=logits.device, dtype=torch.float32)
    check(_lib.load().pa_bce_fwd_bwd(_p(logits, torch.float32), _p(target, torch.float32), B, Cc, grad_scale, _p(loss), _p(dlogits), _p(ws),
                                     _stream()), "pa_bce_fwd_bwd")
    return loss, dlogits


def ce_mixup_fwd_bwd(logits, target_i32, target2_i32=None, lam=None, grad_scale=1.0):
    """ESC-50 loss (ex_esc50.py:159-165); targets are int32 class indices."""
    B, Cc = logits.shape
    loss = torch.empty(1, device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits)
    ws = torch.empty(max(B, 1), device=logits.device, dtype=torch.float32)
    check(_lib.load().pa_ce_mixup_fwd_bwd(_p(logits, torch.float32), _p(target_i32, torch.int32), _p(target2_i32, torch.int32), _p(lam, torch.float32), B, Cc, grad_scale,
                                          _p(loss), _p(dlogits), _p(ws), _stream()), "pa_ce_mixup_fwd_bwd")
    return loss, dlogits


# ---- caller glue -----------------------------------------------------------------------------
def mixup(x, perm_i32, lam):
    B = x.shape[0]
    out = torch.empty_like(x)
    check(_lib.load().pa_mixup(_p(x, torch.float32), _p(perm_i32, torch.int32), _p(lam, torch.float32), _p(out), B, x[0].numel(), _stream()), "pa_mixup")
    return out


def mixup_varlen(x, lens_dev, perm_i32, lam, pad, out=None):
    """Spectrogram mixup of a ragged batch (pa_mixup_varlen).  x (B, 1, F, T) or (B, F, T) dense f32, clip b valid in its first
    lens_dev[b] frames; lens_dev / perm_i32 int32 and lam f32 device tensors of B entries.  Returns a new tensor of x's shape: clip b
    mixed with clip perm[b] cut to its length or continued with ``pad``, exactly 0 behind lens_dev[b].  ``out`` (a dense f32 tensor of
    x's shape that is not x): written and returned instead of a new one."""
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
        raise _lib.PasstAmdError(f"mixup_varlen: expected a (B, 1, F, T) or (B, F, T) spectrogram batch, got shape {tuple(x.shape)}")
    B, rows, ldt = x.shape[0], x.shape[-2], x.shape[-1]
    for name, t in (("lens_dev", lens_dev), ("perm_i32", perm_i32), ("lam", lam)):
        if t.numel() != B:
            raise _lib.PasstAmdError(f"mixup_varlen: {name} has {t.numel()} entries for a batch of {B} clips")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape:
        raise _lib.PasstAmdError(f"mixup_varlen: out has shape {tuple(out.shape)}, x {tuple(x.shape)}")
    check(_lib.load().pa_mixup_varlen(_p(x, torch.float32), _p(lens_dev, torch.int32), _p(perm_i32, torch.int32), _p(lam, torch.float32),
                                      float(pad), _p(out, torch.float32), B, rows, ldt, _stream()), "pa_mixup_varlen")
    return out


def wave_augment(x, L, lengths=None, amp=None, shift=None, partner=None, lam=None):
    """x [B][ldx] f32 raw clips -> [B][L]: gain, pad/truncate, roll, waveform mixup (pa_wave_augment)."""
    B, ldx = x.shape
    out = torch.empty((B, L), device=x.device, dtype=torch.float32)
    ws = torch.empty(B, device=x.device, dtype=torch.float32) if partner is not None else None
    check(_lib.load().pa_wave_augment(_p(x, torch.float32, True), B, x.stride(0), _p(lengths, torch.int32), _p(amp, torch.float32), _p(shift, torch.int32), _p(partner, torch.int32), _p(lam, torch.float32), _p(ws),
                                      _p(out), L, _stream()), "pa_wave_augment")
    return out


def wave_augment_varlen(x, L, lengths=None, out_lengths=None, amp=None, shift=None, partner=None, lam=None):
    """x [B][ldx] f32 raw clips -> [B][L]: row b is clip b after gain, pad/truncate, roll and waveform mixup AT ITS OWN LENGTH
    out_lengths[b] (<= L), exactly 0 behind it (pa_wave_augment_varlen).  lengths (valid samples per row of x; None: ldx),
    out_lengths, shift, partner int32 and amp, lam f32 are device tensors of B entries."""
    if x.dim() != 2:
        raise _lib.PasstAmdError(f"wave_augment_varlen: expected raw clips [B][ldx], got shape {tuple(x.shape)}")
    B = x.shape[0]
    if out_lengths is None:
        raise _lib.PasstAmdError("wave_augment_varlen needs out_lengths (int32, one per clip)")
    for name, t in (("lengths", lengths), ("out_lengths", out_lengths), ("amp", amp), ("shift", shift), ("partner", partner), ("lam", lam)):
        if t is not None and t.numel() != B:
            raise _lib.PasstAmdError(f"wave_augment_varlen: {name} has {t.numel()} entries for a batch of {B} clips")
    if partner is not None and lam is None:
        raise _lib.PasstAmdError("wave_augment_varlen: partner needs lam")
    out = torch.empty((B, L), device=x.device, dtype=torch.float32)
    ws = torch.empty(2 * B, device=x.device, dtype=torch.float32) if partner is not None else None
    check(_lib.load().pa_wave_augment_varlen(_p(x, torch.float32, True), B, max(x.stride(0), x.shape[1]), _p(lengths, torch.int32),
                                             _p(out_lengths, torch.int32), _p(amp, torch.float32), _p(shift, torch.int32),
                                             _p(partner, torch.int32), _p(lam, torch.float32), _p(ws), _p(out), L, L, _stream()),
          "pa_wave_augment_varlen")
    return out


IR_MAX_TAPS = 8192            # PA_IR_MAX_TAPS
IRSpectra = collections.namedtuple("IRSpectra", "spectra ir_len n_ir max_taps")      # what ir_bank_prepare returns


def ir_conv_plan(max_taps):
    """(fft_n, hop) of the overlap-save tiles used for a bank whose longest IR has ``max_taps`` taps (host only)."""
    n, hop = C.c_int32(0), C.c_int32(0)
    check(_lib.load().pa_ir_conv_plan(int(max_taps), C.byref(n), C.byref(hop)), "pa_ir_conv_plan")
    return n.value, hop.value


def ir_bank_prepare(irs, ir_len=None):
    """irs [n_ir][max_taps] f32 (row i valid for ir_len[i] taps; the row length is the bank's max_taps) -> IRSpectra: the
    opaque spectra buffer of pa_ir_bank_prepare together with ir_len (int32, on the device) and the bank's geometry."""
    if irs.dim() != 2 or irs.shape[0] < 1 or not 1 <= irs.shape[1] <= IR_MAX_TAPS:
        raise _lib.PasstAmdError(f"ir_bank_prepare: irs must be [n_ir >= 1][1..{IR_MAX_TAPS} taps], got {tuple(irs.shape)}")
    n_ir, max_taps = irs.shape
    if ir_len is None:
        ir_len = torch.full((n_ir,), max_taps, device=irs.device, dtype=torch.int32)
    if ir_len.numel() != n_ir:
        raise _lib.PasstAmdError(f"ir_bank_prepare: ir_len holds {ir_len.numel()} entries for {n_ir} IRs")
    lib = _lib.load()
    spectra = torch.empty(lib.pa_ir_bank_floats(n_ir, max_taps), device=irs.device, dtype=torch.float32)
    check(lib.pa_ir_bank_prepare(_p(irs, torch.float32), n_ir, max_taps, _p(ir_len, torch.int32), _p(spectra), _stream()), "pa_ir_bank_prepare")
    return IRSpectra(spectra, ir_len, n_ir, max_taps)


def wave_ir_convolve(x, L, lengths=None, ir_idx=None, bank=None, out=None):
    """x [B][ldx] f32 raw clips -> (out [B][L], len_out int32 [B]): clip b convolved ('full') with IR ir_idx[b] of ``bank`` (an
    IRSpectra), cut or zero padded to L; ir_idx[b] < 0 copies the clip (pa_wave_ir_convolve).  ``out``: an optional [B][L] f32
    destination whose rows may be further apart than L."""
    if bank is None:
        raise _lib.PasstAmdError("wave_ir_convolve needs the IRSpectra of ir_bank_prepare")
    B = x.shape[0]
    if out is None:
        out = torch.empty((B, L), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, L):
        raise _lib.PasstAmdError(f"wave_ir_convolve: out must be [{B}][{L}], got {tuple(out.shape)}")
    if ir_idx is not None and ir_idx.numel() != B or lengths is not None and lengths.numel() != B:
        raise _lib.PasstAmdError(f"wave_ir_convolve: lengths / ir_idx must hold {B} entries")
    len_out = torch.empty(B, device=x.device, dtype=torch.int32)
    check(_lib.load().pa_wave_ir_convolve(_p(x, torch.float32, True), B, max(x.stride(0), x.shape[1]), _p(lengths, torch.int32),
                                          _p(ir_idx, torch.int32), _p(bank.spectra, torch.float32), _p(bank.ir_len, torch.int32),
                                          bank.n_ir, bank.max_taps, _p(out, torch.float32, True), max(out.stride(0), L),
                                          L, _p(len_out), _stream()), "pa_wave_ir_convolve")
    return out, len_out


def grad_norm_partials(n):
    """how many f32 partial sums pa_grad_accum_sumsq writes for a span of n elements (host only: a function of n alone)"""
    return int(_lib.load().pa_grad_norm_partials(int(n)))


def grad_accum_sumsq(g, acc=None, first=False, partials=None):
    """One pass over the flat f32 gradients ``g``: ``acc = g if first else acc + g`` (when given) and/or ``partials[k]`` = the sum of
    squares of chunk k of the result (acc, or g without acc); deterministic, see pa_grad_accum_sumsq."""
    n = g.numel()
    if acc is not None and acc.numel() != n:
        raise _lib.PasstAmdError(f"grad_accum_sumsq: acc holds {acc.numel()} elements, g {n}")
    if partials is not None and partials.numel() != grad_norm_partials(n):
        raise _lib.PasstAmdError(f"grad_accum_sumsq: {partials.numel()} partial slots for {n} elements, {grad_norm_partials(n)} needed")
    check(_lib.load().pa_grad_accum_sumsq(_p(g, torch.float32), _p(acc, torch.float32), int(bool(first)), n, _p(partials, torch.float32),
                                          _stream()), "pa_grad_accum_sumsq")


def clip_coef(partials, max_norm, out):
    """out[0] = the total L2 norm behind ``partials``, out[1] = clip_grad_norm_'s factor for ``max_norm`` (2 device floats, no sync)"""
    if out.numel() != 2:
        raise _lib.PasstAmdError("clip_coef: out holds 2 floats (norm, factor)")
    check(_lib.load().pa_clip_coef(_p(partials, torch.float32), partials.numel(), float(max_norm), _p(out, torch.float32), _stream()),
          "pa_clip_coef")


def adamw_hyper(lr, beta1, beta2, eps, wd, step, out_host):
    """fill the 7-float HOST tensor `out_host` with [lr, beta1, beta2, eps, wd, 1 - beta1^step, sqrt(1 - beta2^step)]"""
    assert out_host.dtype == torch.float32 and out_host.numel() == 7 and not out_host.is_cuda
    _lib.load().pa_adamw_hyper(lr, beta1, beta2, eps, wd, int(step), C.cast(out_host.data_ptr(), C.POINTER(C.c_float)))


def swa_update(avg, p, num_averaged):
    """avg = p if num_averaged == 0 else avg + (p - avg) / (num_averaged + 1), flat f32 buffers."""
    check(_lib.load().pa_swa_update(_p(avg, torch.float32), _p(p, torch.float32), p.numel(), int(num_averaged), _stream()), "pa_swa_update")


def sgd(p, g, lr):
    check(_lib.load().pa_sgd(_p(p, torch.float32), _p(g, torch.float32), p.numel(), lr, _stream()), "pa_sgd")


# ---- validation metrics ----------------------------------------------------------------------
def eval_append(scores, target, keys, state, n0, mask=None, mode=_lib.EVAL_SIGMOID):
    """One validation batch [B][C] (f32 logits or scores, targets, optional 0/1 mask) into columns n0 .. n0 + B of the
    class-major buffers keys [C][capacity] int32 (the u32 rank keys) and state [C][capacity] uint8 (pa_eval_append)."""
    B, Cc = scores.shape
    if target.shape != scores.shape or (mask is not None and mask.shape != scores.shape):
        raise _lib.PasstAmdError(f"eval_append: scores {tuple(scores.shape)}, target {tuple(target.shape)}"
                                 f"{'' if mask is None else f', mask {tuple(mask.shape)}'} must have one shape")
    if keys.dim() != 2 or keys.shape[0] != Cc or state.shape != keys.shape:
        raise _lib.PasstAmdError(f"eval_append: keys {tuple(keys.shape)} / state {tuple(state.shape)} are not [{Cc}][capacity]")
    check(_lib.load().pa_eval_append(_p(scores, torch.float32), _p(target, torch.float32), _p(mask, torch.float32), B, Cc, int(n0),
                                     keys.shape[1], int(mode), _p(keys, torch.int32), _p(state, torch.uint8), _stream()), "pa_eval_append")


def eval_rank(keys, state, n, ws=None):
    """Per-class metrics of the first n columns: (n_pos, n_neg, auc_num) int64 [C] and (ap, auc) float64 [C] (pa_eval_rank).
    ws: a uint8 workspace of at least pa_eval_ws_bytes(C, capacity) bytes to reuse, else one is allocated."""
    if keys.dim() != 2 or state.shape != keys.shape:
        raise _lib.PasstAmdError(f"eval_rank: keys {tuple(keys.shape)} / state {tuple(state.shape)} are not [C][capacity]")
    Cc, cap = keys.shape
    lib = _lib.load()
    need = lib.pa_eval_ws_bytes(Cc, cap)
    if need <= 0:
        raise _lib.PasstAmdError(f"eval_rank: unsupported shape [{Cc}][{cap}]")
    if ws is None:
        ws = torch.empty(need, device=keys.device, dtype=torch.uint8)
    elif ws.numel() < need:
        raise _lib.PasstAmdError(f"eval_rank: workspace of {ws.numel()} bytes, {need} needed")
    ints = torch.empty((3, Cc), device=keys.device, dtype=torch.int64)
    flt = torch.empty((2, Cc), device=keys.device, dtype=torch.float64)
    check(lib.pa_eval_rank(_p(keys, torch.int32), _p(state, torch.uint8), Cc, int(n), cap, _p(ws, torch.uint8), _p(ints[0]), _p(ints[1]),
                           _p(ints[2]), _p(flt[0]), _p(flt[1]), _stream()), "pa_eval_rank")
    return ints[0], ints[1], ints[2], flt[0], flt[1]

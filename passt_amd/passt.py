"""PaSST on MI355X: drop-in for the reference's ``models/passt.py``.

Same public surface as the reference (kkoutini/PaSST, file:line below are the reference's):
``PaSST`` (models/passt.py:383) with identical constructor kwargs, ``state_dict`` keys/shapes
(SURVEY.md App. D), parameter order and ``forward(x) -> (logits, features)`` (:576-595);
``get_model`` (:957-1018) / ``get_model_passt`` (hear21passt alias), ``get_ensemble_model``
(:1039-1045), ``EnsembelerModel`` (:1021-1037), ``fix_embedding_layer``/``lighten_model``
(:924-954) and a ``model_ing`` ingredient when ``ba3l`` is importable.

Underneath, nothing of torch's operator library is used on the hot path: ``forward`` /
``backward`` sequence the hand-written gfx950 kernels of libpasst_amd.so (include/passt_amd.h)
through one ``torch.autograd.Function``; the sub-modules below (``nn.Linear`` ...) are
*parameter containers only*, kept so that ``state_dict()``, ``.parameters()`` order,
``deepcopy`` (SWA), ``print(model)`` and checkpoint loading behave exactly like the reference.

Precision: plain call = exact-f32 MFMA path (matches the reference's fp32 forward/backward
<= 1e-3 rel); inside ``torch.autocast("cuda")`` or with ``model.precision = "bf16"`` = bf16 MFMA
with f32 accumulation, f32 residual stream / LayerNorm / softmax (the reference's AMP regime).
Patchout indices are drawn with the reference's own torch CPU RNG calls in the reference's order
(:513-553), hence bit-exact.
"""
import contextlib
import copy
import math
import os
import warnings
import weakref
from collections import OrderedDict
from functools import partial
from itertools import islice
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn
from torch.optim.optimizer import register_optimizer_step_post_hook

from . import ops
from ._lib import EPI_DGELU, EPI_RESID, EPI_STORE, PA_BF16, PA_F32, PasstAmdError, compile_opaque


def to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


# --------------------------------------------------------------------------------------------
# parameter containers (never executed on the product path)
# --------------------------------------------------------------------------------------------
class PatchEmbed(nn.Module):
    """Parameter container mirroring models/passt.py:298-328 (Conv2d 1->D, k=patch, stride)."""

    def __init__(self, img_size=224, patch_size=16, stride=16, in_chans=3, embed_dim=768, norm_layer=None,
                 flatten=True):
        super().__init__()
        self.img_size = to_2tuple(img_size)
        self.patch_size = to_2tuple(patch_size)
        self.stride = to_2tuple(stride)
        self.grid_size = (self.img_size[0] // self.stride[0], self.img_size[1] // self.stride[1])
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.flatten = flatten
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.stride)
        self.norm = norm_layer(embed_dim) if norm_layer else nn.Identity()


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)


class DropPath(nn.Module):
    """Stochastic depth per sample (models/helpers/vit_helpers.py:203-233): holds the rate.  The kernel sequence reads ``drop_prob`` and
    never calls ``forward`` -- the factor rides in the residual GEMM's epilogue (drop_path_draws, _forward_trunk); ``forward`` is the
    reference's own arithmetic in plain torch, for hooks and CPU use.  No parameters, no buffers."""

    def __init__(self, drop_prob=None):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if not self.drop_prob or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = (keep + torch.rand((x.shape[0],) + (1,) * (x.ndim - 1), dtype=x.dtype, device=x.device)).floor_()
        return x.div(keep) * mask

    def extra_repr(self):
        return f"drop_prob={self.drop_prob}"


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()      # one module for both branches (:372)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)


def _init_vit_weights(module):
    """models/passt.py:598-629 as reached through ``self.apply`` (no name => generic branch)."""
    if isinstance(module, nn.Linear):
        nn.init.trunc_normal_(module.weight, std=.02)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, (nn.LayerNorm, nn.GroupNorm, nn.BatchNorm2d)):
        nn.init.zeros_(module.bias)
        nn.init.ones_(module.weight)


# --------------------------------------------------------------------------------------------
# host-side index logic (bit-exact with the reference: same torch CPU RNG calls, same order)
# --------------------------------------------------------------------------------------------
def draw_patchout(model, F_dim, T_dim):
    """models/passt.py:513-553.  Returns (toff, T_eff, idx_t, idx_f, idx_u) (numpy / None)."""
    Tpe = model.time_new_pos_embed.shape[-1]
    toff, T_eff = 0, T_dim
    if T_dim < Tpe:
        if model.training:
            toff = torch.randint(1 + Tpe - T_dim, (1,)).item()                         # :516
    else:
        warnings.warn(f"the patches shape:{(F_dim, T_dim)} are larger than the expected time encodings "
                      f"{tuple(model.time_new_pos_embed.shape)}, x will be cut")         # :524-526
        T_eff = Tpe
    idx_t = idx_f = idx_u = None
    T_cur, F_cur = T_eff, F_dim
    if model.training and model.s_patchout_t:
        idx_t = torch.randperm(T_dim)[:T_dim - model.s_patchout_t].sort().values.numpy()   # :535
        if idx_t.size and idx_t.max() >= T_eff:
            raise IndexError("time patchout index out of range (reference would fail at models/passt.py:536)")
        T_cur = idx_t.size
    if model.training and model.s_patchout_f:
        idx_f = torch.randperm(F_dim)[:F_dim - model.s_patchout_f].sort().values.numpy()   # :541
        F_cur = idx_f.size
    if model.training and model.u_patchout:
        S = F_cur * T_cur
        idx_u = torch.randperm(S)[:S - model.u_patchout].sort().values.numpy()             # :551
    return toff, T_eff, idx_t, idx_f, idx_u


def kept_patches(F_dim, T_eff, idx_t, idx_f, idx_u):
    """Grid coordinates of the surviving patches in sequence order (frequency-major flatten, :546)."""
    ts = np.arange(T_eff, dtype=np.int32) if idx_t is None else idx_t
    fs = np.arange(F_dim, dtype=np.int32) if idx_f is None else idx_f
    pf = np.repeat(fs, ts.size)
    pt = np.tile(ts, fs.size)
    if idx_u is not None:
        pf, pt = pf[idx_u], pt[idx_u]
    return pf.astype(np.int32, copy=False), pt.astype(np.int32, copy=False)


# --------------------------------------------------------------------------------------------
# the kernel sequence
# --------------------------------------------------------------------------------------------
class _Staged:
    """Per-dtype GEMM-ready copies of the weights (bf16 cast and/or transposes), re-made only when a
    parameter changed (``_version`` bump by the optimizer / load_state_dict).  The first time a copy is
    asked for it is made on its own; from then on a stale copy triggers ONE batched launch
    (pa_stage_weights) that refreshes every known copy of that dtype in place -- after an optimizer step
    all of them are stale together."""

    def __init__(self):
        self.cache = {}     # (id(p), dtype, transposed) -> [version, tensor, p]
        self.tables = {}    # dtype -> (signature, device table, n, tiles, keys)
        self.epoch = 0      # bumped by optimizers that update parameters through raw pointers
        self.gen = 0        # bumped whenever a copy tensor is created: fused optimizer tables (adamw_table) are keyed on it
        self.fused = {}     # (span key, dtype) -> (gen, device table, n, items, cache keys covered)

    def _version(self, p):
        return (p._version, p.data_ptr(), self.epoch)

    def _refresh_all(self, dtype):
        if os.environ.get("PASST_AMD_NO_BATCH_STAGE"):          # A/B knob: one launch per copy, as on first use
            return False
        tab = self.stage_table(dtype)
        if tab is None:
            return False
        ops.stage_weights(tab[1], tab[2], tab[3], dtype)
        for key, ent in self.cache.items():
            if key[1] == dtype:
                ent[0] = self._version(ent[2])
        return True

    def stage_table(self, dtype):
        """(signature, device table, n, tiles) of the batched refresh of every known copy of ``dtype``; (re)built -- one small
        host-to-device copy -- when the set of copies changed.  TrainStep's graph mode calls this BEFORE it starts capturing: with
        the optimizer rewriting the copies itself (pa_adamw_stage) the eager warm-up steps never need the refresh launch, and a
        copy is not allowed inside a stream capture."""
        groups = {}
        for key, (ver, out, p) in self.cache.items():
            if key[1] == dtype:
                groups.setdefault(key[0], [p, None, None])[2 if key[2] else 1] = out
        if not groups:
            return None
        sig = tuple((pid, g[0].data_ptr(), None if g[1] is None else g[1].data_ptr(),
                     None if g[2] is None else g[2].data_ptr()) for pid, g in groups.items())
        tab = self.tables.get(dtype)
        if tab is None or tab[0] != sig:
            entries = []
            for p, dst, dst_t in groups.values():
                w2 = p.detach().reshape(p.shape[0], -1)
                if not w2.is_contiguous():
                    return None
                entries.append((w2, dst, dst_t))
            tab = self.tables[dtype] = (sig,) + ops.make_stage_table(entries, next(iter(groups.values()))[0].device)
        return tab

    def get(self, p, dtype, transposed):
        if dtype == PA_F32 and not transposed:                  # used in place
            w2 = p.detach().reshape(p.shape[0], -1)
            return w2 if w2.is_contiguous() else w2.contiguous()
        key = (id(p), dtype, transposed)
        ver = self._version(p)
        hit = self.cache.get(key)
        if hit is not None:
            if hit[0] == ver:
                return hit[1]
            if hit[0][1] == ver[1] and self._refresh_all(dtype):     # same storage, new values: batched refresh
                return hit[1]
        w = p.detach()
        w2 = w.reshape(w.shape[0], -1)
        if not w2.is_contiguous():
            w2 = w2.contiguous()
        if transposed:
            out = ops.transpose(w2, dtype)
        else:
            out = ops.convert(w2, dtype)
        self.cache[key] = [ver, out, p]
        self.tables.pop(dtype, None)
        self.gen += 1
        return out

    def adamw_table(self, span_key, params, dtype):
        """The pa_adamw_stage descriptor table of one optimizer launch: ``params`` = [(parameter, element offset in the launch's
        flat buffers)], every parameter of the launch in buffer order.  A parameter with GEMM-ready copies of ``dtype`` in the
        cache gets them rewritten by the optimizer launch itself (no separate pa_stage_weights pass reads the updated values
        back); returns (device table, n, work items, covered cache keys) -- mark_fresh(keys) once the parameters' epoch was bumped."""
        hit = self.fused.get((span_key, dtype))
        if hit is not None and hit[0] == self.gen:
            return hit[1:]
        entries, keys = [], []
        for p, off in params:
            kd, kt = (id(p), dtype, False), (id(p), dtype, True)
            d, t = self.cache.get(kd), self.cache.get(kt)
            ok = (d is not None or t is not None) and p.dim() >= 2 and p.is_contiguous()
            if ok and d is not None and d[2] is not p or ok and t is not None and t[2] is not p:
                ok = False                                      # an id re-used by another tensor: leave it to get()
            if not ok:
                entries.append((off, 1, p.numel(), None, None))
                continue
            rows = p.shape[0]
            entries.append((off, rows, p.numel() // rows, None if d is None else d[1], None if t is None else t[1]))
            keys += [k for k, e in ((kd, d), (kt, t)) if e is not None]
        tab = ops.make_adamw_stage_table(entries, params[0][0].device)
        self.fused[(span_key, dtype)] = (self.gen,) + tab + (keys,)
        return tab + (keys,)

    def mark_fresh(self, keys):
        """The copies under ``keys`` were just rewritten from the current parameter values (fused optimizer launch)."""
        for k in keys:
            ent = self.cache.get(k)
            if ent is not None:
                ent[0] = self._version(ent[2])


def _prefix_rows(model, B, Ntok, device):
    """int32 row indices of the cls / dist tokens in the [B*Ntok] token matrix (cached per shape)."""
    key = ("pidx", B, Ntok, str(device))
    t = model._scratch.get(key)
    if t is None:
        idx = (np.arange(B, dtype=np.int32)[:, None] * Ntok + np.arange(2, dtype=np.int32)[None, :]).reshape(-1)
        t = model._scratch[key] = torch.from_numpy(idx).to(device)
    return t


def _precision(model):
    if model.precision is not None:
        return {"fp32": PA_F32, "f32": PA_F32, "bf16": PA_BF16}[model.precision]
    return PA_BF16 if torch.is_autocast_enabled() else PA_F32


def _checked_input(model, x, bind_dt):
    """What every forward checks first: a HIP tensor, the precision of this call, a dense f32 (B, 1, n_mels, frames) spectrogram.
    ``bind_dt``: remember the precision as the one whose weight copies a bound optimizer refreshes (it steps outside torch.autocast)."""
    if not x.is_cuda:
        raise PasstAmdError("passt_amd.PaSST runs on a HIP device only (no CPU fallback); got a CPU tensor")
    dt = _precision(model)
    if bind_dt:
        object.__setattr__(model, "_last_dt", dt)
    x = x.contiguous().float()
    if x.dim() != 4 or x.shape[1] != 1:
        raise ValueError(f"PaSST expects a (B, 1, n_mels, frames) spectrogram, got {tuple(x.shape)} "
                         "(in_chans = 1 in every reference arch, models/passt.py:961)")
    return x, dt


def _freq_rows(model, F):
    """Frequency rows of the patch grid of an F-bin spectrogram; they must be the frequency embedding's."""
    F_dim = (F - model.patch_embed.patch_size[0]) // model.patch_embed.stride[0] + 1
    Fpe = model.freq_new_pos_embed.shape[-2]
    if F_dim != Fpe:
        raise RuntimeError(f"patch grid has {F_dim} frequency rows but freq_new_pos_embed has {Fpe}")
    return F_dim


# The two token layouts.  The shared kernel sequence below (_forward_trunk / _backward_trunk) runs on a token matrix [M][D] and
# asks the layout for what it cannot know: B, M, the rows of the cls / dist tokens, the attention entries of this layout, and
# whether the stage in front of block 0 wants block 0's input gradient in 16 bits as well.
class _FixedLayout:
    """B clips of Ntok token rows each (every clip keeps the same patches)."""
    dx0_lp = False                  # the patch stage starts from the f32 dx (pa_patch_bwd makes its own compact 16-bit dpatch)

    def __init__(self, model, B, Ntok):
        self.model, self.B, self.Ntok, self.M = model, B, Ntok, B * Ntok

    def prefix_rows(self, device):
        return _prefix_rows(self.model, self.B, self.Ntok, device)

    def hidden_view(self, h):
        return h.view(self.B, self.Ntok, -1)

    def attention_fwd(self, qkv, H, scale, drop=None, **kw):
        """``drop``: (seed, site, t) of a block with an active attention dropout -- the dropout entry; None: the plain one"""
        if drop is not None:
            return ops.attention_fwd_dropout(qkv, self.B, H, self.Ntok, scale, *drop, **kw)
        return ops.attention_fwd(qkv, self.B, H, self.Ntok, scale, **kw)

    def attention_bwd(self, qkv, att, d_att, lse, H, scale, drop=None, **kw):
        if drop is not None:
            return ops.attention_bwd_dropout(qkv, att, d_att, lse, self.B, H, self.Ntok, scale, *drop, **kw)
        return ops.attention_bwd(qkv, att, d_att, lse, self.B, H, self.Ntok, scale, **kw)

    def prefix_lse(self, lse, H):
        """The all-queries lse [(b*H + h)*Ntok + q] cut to its cls / dist rows, compact as attention_fwd(nq=2) leaves it."""
        return lse.view(self.B * H, self.Ntok)[:, :2].contiguous().view(-1)

    def attention_probs(self, qkv, lse, H, scale, nq, head_mean, flags):
        """One attention map in the shape PaSST.forward hands out: (B, H, Nq, Ntok), or (B, Nq, Ntok) for the mean over heads."""
        p = ops.attention_probs(qkv, lse, self.B, H, self.Ntok, scale, nq=nq, head_mean=head_mean, flags=flags)
        return p.view(self.B, -1, self.Ntok) if head_mean else p

    def attention_probs_grad(self, qkv, lse, d_att, H, scale, nq, head_mean, flags, mode, do_compact):
        """The gradient of one attention map (ops.attention_probs_grad), in the map's own shape."""
        p = ops.attention_probs_grad(qkv, lse, d_att, self.B, H, self.Ntok, scale, nq=nq, head_mean=head_mean, mode=mode,
                                     do_compact=do_compact, flags=flags)
        return p.view(self.B, -1, self.Ntok) if head_mean else p

    def rollout_start(self, device):
        """The one-hot start rows of a rollout, (B, 2, Ntok) f32: row 0 = cls, row 1 = dist."""
        r = torch.zeros((self.B, 2, self.Ntok), device=device, dtype=torch.float32)
        r[:, 0, 0] = 1.0
        r[:, 1, 1] = 1.0
        return r

    def attention_rollout(self, qkv, lse, r_in, H, scale, a, b, nq, flags, **kw):
        """One rollout step on the (B, 2, Ntok) rows (ops.attention_rollout): no map is formed."""
        return ops.attention_rollout(qkv, lse, r_in, self.B, H, self.Ntok, scale, a, b, nq=nq, flags=flags, **kw)


class _PackedLayout:
    """B clips of different token counts back to back: clip b owns rows cu_tok[b] .. cu_tok[b + 1] (device int32), none longer
    than max_N; ``pidx``: the rows of the cls / dist tokens (device int32).  The attention backward is always the kernel pair."""
    dx0_lp = True                   # block 0's 16-bit dx feeds the patch stage's two GEMMs as it is

    def __init__(self, B, M, max_N, cu_tok, pidx, ntok=None):
        self.B, self.M, self.max_N, self.cu_tok, self.pidx = B, M, max_N, cu_tok, pidx
        self.ntok, self._map_off = ntok, {}      # host token counts per clip (attention maps only); their uploaded output offsets

    def prefix_rows(self, device):
        return self.pidx

    def hidden_view(self, h):
        return h.view(self.M, -1)       # a view, not h itself: what the autograd node hands out must not be what its context keeps

    def attention_fwd(self, qkv, H, scale, drop=None, **kw):
        """``drop``: as in _FixedLayout.attention_fwd; clip b gets the mask of sequence b of a fixed batch (s = b*H + h, local q / k)"""
        if drop is not None:
            return ops.attention_fwd_varlen_dropout(qkv, self.cu_tok, self.B, H, self.max_N, scale, *drop, **kw)
        return ops.attention_fwd_varlen(qkv, self.cu_tok, self.B, H, self.max_N, scale, **kw)

    def attention_bwd(self, qkv, att, d_att, lse, H, scale, drop=None, **kw):
        if drop is not None:
            return ops.attention_bwd_varlen_dropout(qkv, att, d_att, lse, self.cu_tok, self.B, H, self.max_N, scale, *drop, **kw)
        return ops.attention_bwd_varlen(qkv, att, d_att, lse, self.cu_tok, self.B, H, self.max_N, scale, **kw)

    def prefix_lse(self, lse, H):
        """The all-queries lse [h][total tokens] cut to every clip's cls / dist rows, compact [(b*H + h)*2 + q] as
        attention_fwd_varlen(nq=2) leaves it."""
        return lse.view(H, self.M).index_select(1, self.pidx).view(H, self.B, 2).permute(1, 0, 2).contiguous().view(-1)

    def _map_offsets(self, Ho, nq, device):
        key = (Ho, nq)
        if key not in self._map_off:
            off, total = ops.attention_probs_offsets(self.ntok, Ho, nq)
            self._map_off[key] = (ops.upload_small(off, device), total)
        return self._map_off[key]

    def attention_probs_grad(self, qkv, lse, d_att, H, scale, nq, head_mean, flags, mode, do_compact):
        """The gradient of one attention map of the packed batch as ONE flat f32 buffer, cut like the map (attn_views); the offsets
        are the ones the map's own launch uploaded."""
        off_dev, total = self._map_offsets(1 if head_mean else H, nq, qkv.device)
        return ops.attention_probs_grad_varlen(qkv, lse, d_att, self.cu_tok, off_dev, total, self.B, H, self.max_N, scale, nq=nq,
                                               head_mean=head_mean, mode=mode, do_compact=do_compact, flags=flags)

    def attention_probs(self, qkv, lse, H, scale, nq, head_mean, flags):
        """One attention map of the packed batch as ONE flat f32 buffer (attn_views cuts it into the clips' tensors)."""
        off_dev, total = self._map_offsets(1 if head_mean else H, nq, qkv.device)
        return ops.attention_probs_varlen(qkv, lse, self.cu_tok, off_dev, total, self.B, H, self.max_N, scale, nq=nq,
                                          head_mean=head_mean, flags=flags)

    def rollout_start(self, device):
        """The one-hot start rows of a rollout as ONE f32 buffer (2, M): clip b's dense (2, N_b) block starts at float 2 * cu_tok[b]
        (rollout_views cuts it); row 0 = cls, row 1 = dist."""
        n = np.asarray(self.ntok, dtype=np.int64)
        base = 2 * (np.cumsum(n) - n)
        r = np.zeros((2, self.M), dtype=np.float32)
        r.reshape(-1)[np.concatenate([base, base + n + 1])] = 1.0
        return ops.upload_small(r, device)

    def attention_rollout(self, qkv, lse, r_in, H, scale, a, b, nq, flags, **kw):
        """One rollout step on the packed (2, M) buffer (ops.attention_rollout_varlen)."""
        return ops.attention_rollout_varlen(qkv, lse, r_in, self.cu_tok, self.B, H, self.max_N, scale, a, b, nq=nq, flags=flags, **kw)

    @staticmethod
    def rollout_views(r, tok_offsets):
        """The packed rollout buffer -> a list of B views: clip i's (2, N_i)."""
        return ops.rollout_views(r, (tok_offsets[1:] - tok_offsets[:-1]).tolist())

    @staticmethod
    def attn_views(p, tok_offsets, H, prefix, head_mean):
        """The flat buffer of a packed map -> a list of B views: clip i's (H, Nq_i, N_i), or (Nq_i, N_i) for the mean over heads."""
        ntok = (tok_offsets[1:] - tok_offsets[:-1]).tolist()
        off, _ = ops.attention_probs_offsets(ntok, 1 if head_mean else H, 2 if prefix else None)
        out = []
        for o, n in zip(off.tolist(), ntok):
            nq = min(2, n) if prefix else n
            out.append(p[o:o + nq * n].view(nq, n) if head_mean else p[o:o + H * nq * n].view(H, nq, n))
        return out


def parse_hidden(hidden, nblk):
    """``hidden=`` of PaSST.forward -> a tuple of block indices in [0, nblk) and / or "norm", in the order asked.  ValueError for
    anything else: a bare int or string, an empty sequence, an index out of range, an entry named twice (also as k and k - nblk)."""
    if isinstance(hidden, (str, bytes)) or not isinstance(hidden, (list, tuple)):
        raise ValueError(f"hidden must be a sequence of block indices and/or \"norm\", e.g. hidden=(3, 7, -1, \"norm\"); got {hidden!r}")
    if not hidden:
        raise ValueError("hidden is empty: name at least one block index or \"norm\" (hidden=None asks for no token outputs)")
    out = []
    for h in hidden:
        if isinstance(h, str):
            if h != "norm":
                raise ValueError(f"hidden: unknown entry {h!r} (the only name is \"norm\")")
            k = h
        elif isinstance(h, (int, np.integer)) and not isinstance(h, (bool, np.bool_)):
            k = int(h)
            if not -nblk <= k < nblk:
                raise ValueError(f"hidden: block index {k} is out of range for {nblk} blocks")
            k %= nblk
        else:
            raise ValueError(f"hidden: entries are ints or \"norm\", got {h!r}")
        if k in out:
            raise ValueError(f"hidden: {h!r} is named twice")
        out.append(k)
    return tuple(out)


def parse_attn(attn, nblk, attn_rows="all", attn_heads="each"):
    """``attn=`` / ``attn_rows=`` / ``attn_heads=`` of PaSST.forward -> (block indices in [0, nblk) in the order asked, prefix rows
    only?, mean over heads?).  parse_hidden's rules without "norm": ValueError for a bare int or string, an empty sequence, an index
    out of range, an index named twice (also as k and k - nblk), and for any other value of the two modes."""
    if attn_rows not in ("all", "prefix"):
        raise ValueError(f"attn_rows must be \"all\" or \"prefix\" (the cls and dist query rows), got {attn_rows!r}")
    if attn_heads not in ("each", "mean"):
        raise ValueError(f"attn_heads must be \"each\" or \"mean\", got {attn_heads!r}")
    if isinstance(attn, (str, bytes)) or not isinstance(attn, (list, tuple, range)):
        raise ValueError(f"attn must be a sequence of block indices, e.g. attn=(0, -1); got {attn!r}")
    if not attn:
        raise ValueError("attn is empty: name at least one block index (attn=None asks for no attention maps)")
    out = []
    for a in attn:
        if not isinstance(a, (int, np.integer)) or isinstance(a, (bool, np.bool_)):
            raise ValueError(f"attn: entries are block indices (ints), got {a!r}")
        k = int(a)
        if not -nblk <= k < nblk:
            raise ValueError(f"attn: block index {k} is out of range for {nblk} blocks")
        k %= nblk
        if k in out:
            raise ValueError(f"attn: block {a!r} is named twice")
        out.append(k)
    return tuple(out), attn_rows == "prefix", attn_heads == "mean"


def parse_attn_grad(attn_grad, attn, attn_heads="each"):
    """``attn_grad=`` of PaSST.forward -> None, "grad" or "cam" (True means "grad").  ValueError for any other value, for a request
    without ``attn=`` and for "grad" with ``attn_heads="mean"`` (the network never forms a mean over heads of the probabilities, so
    there is no gradient with respect to one)."""
    if attn_grad is None or attn_grad is False:
        return None
    mode = "grad" if attn_grad is True else attn_grad
    if not isinstance(mode, str) or mode not in ("grad", "cam"):
        raise ValueError(f"attn_grad must be None, \"grad\" (or True) or \"cam\", got {attn_grad!r}")
    if attn is None:
        raise ValueError("attn_grad needs attn=: it fills .grad of the attention maps that attn= returns")
    if mode == "grad" and attn_heads == "mean":
        raise ValueError("attn_grad=\"grad\" needs attn_heads=\"each\": the network forms no mean over heads, so nothing is the "
                         "gradient with respect to one (attn_grad=\"cam\" gives the head mean of relu(map * gradient))")
    return mode


def parse_rollout(rollout, rollout_from, nblk):
    """``rollout=`` / ``rollout_from=`` of PaSST.forward -> None or (mode, first block in [0, nblk)).  ValueError for any value other
    than None, "attn", "cam", for a ``rollout_from`` that is no int or out of range, and for one without ``rollout``."""
    if rollout is not None and (not isinstance(rollout, str) or rollout not in ("attn", "cam")):
        raise ValueError(f"rollout must be None, \"attn\" or \"cam\", got {rollout!r}")
    if not isinstance(rollout_from, (int, np.integer)) or isinstance(rollout_from, (bool, np.bool_)):
        raise ValueError(f"rollout_from must be a block index (an int), got {rollout_from!r}")
    k = int(rollout_from)
    if not -nblk <= k < nblk:
        raise ValueError(f"rollout_from: block index {k} is out of range for {nblk} blocks")
    if rollout is None:
        if k != 0:
            raise ValueError("rollout_from needs rollout=: it names the first block of the rollout that rollout= asks for")
        return None
    return rollout, k % nblk


class _RolloutRequest:
    """What a call with ``rollout="cam"`` hands the autograd node in the place of parse_rollout's pair.  ``first``: the first block of
    the product; ``start``: the one-hot start rows the forward made (the node's own tensor); ``target``: the tensor forward() returned
    for them (packed: the list of the clips' views), put there by forward(): the backward fills its .grad with the rolled-out rows;
    ``g_scale``: what the backward multiplies the maps' gradients by (the world size under an attached reducer, whose node divides
    dlogits by it: the product of (I + C_l) is not linear in that factor, so it cannot be repaired afterwards)."""
    __slots__ = ("first", "start", "target", "g_scale", "result")

    def __init__(self, first):
        self.first, self.start, self.target, self.g_scale, self.result = first, None, None, 1.0, None


class _AttnGradRequest:
    """What a call with ``attn_grad=`` hands the autograd node in the place of parse_attn's triple.  ``triple``: that triple (blocks,
    prefix rows only?, mean over heads?); ``mode``: "grad" / "cam"; ``targets``: per requested block the tensor forward() returned
    for it (packed: the list of the clips' tensors), put there by forward() once it has cut them; the backward fills their .grad
    (_map_grad).  The maps have no grad_fn, so holding them makes no cycle."""
    __slots__ = ("triple", "mode", "targets")

    def __init__(self, triple, mode):
        self.triple, self.mode, self.targets = triple, mode, None


class _Fwd(NamedTuple):
    """What ONE forward produces, on every entry path.  ``ctx``: what the backward needs (None for a forward that saves nothing, and
    on a record rebuilt from the autograd node's outputs); ``hidden``: the token outputs asked for, in the order asked -- (B, Ntok, D)
    views, packed: (M, D); ``maps``: the attention maps asked for, in the order asked -- shaped tensors, packed: one flat buffer per
    map (_PackedLayout.attn_views cuts it); both empty when not asked for.  ``tok_offsets``: None on the fixed path; on the packed path
    the int64 CPU tensor of B + 1 row offsets whenever token outputs or maps were asked for."""
    logits: torch.Tensor
    feat: torch.Tensor
    ctx: Optional[dict]
    hidden: tuple = ()
    maps: tuple = ()
    tok_offsets: Optional[torch.Tensor] = None
    roll: Optional[torch.Tensor] = None      # rollout=: the cls / dist rows, (B, 2, Ntok); packed: one (2, M) buffer (rollout_views cuts it)

    def flat(self):
        """The tensors in the order the autograd node hands them out (and from_flat reads them back)."""
        return (self.logits, self.feat) + self.hidden + self.maps + (() if self.roll is None else (self.roll,)) + \
            (() if self.tok_offsets is None else (self.tok_offsets,))

    @classmethod
    def from_flat(cls, out, n_hidden, n_maps, has_roll=False):
        it = iter(out)
        logits, feat, hidden, maps = next(it), next(it), tuple(islice(it, n_hidden)), tuple(islice(it, n_maps))
        roll = next(it) if has_roll else None
        return cls(logits, feat, None, hidden, maps, next(it, None), roll)


# --------------------------------------------------------------------------------------------
# stochastic depth (DropPath, models/helpers/vit_helpers.py:203-233; models/passt.py:372, 378-379, 444-448)
# --------------------------------------------------------------------------------------------
def param_stage(name, depth):
    """The stage a parameter belongs to: -1 the patch embedding, cls / dist tokens and position tables, 0 .. depth-1 the blocks,
    ``depth`` the final norm + head (the buckets of ddp.bucket_layout and of passt_backward's ``on_block_done``)."""
    if name.startswith("blocks."):
        return int(name.split(".")[1])
    return depth if name.startswith(("norm.", "head.")) else -1


# the weights whose gradient is a weight-gradient GEMM of its own: frozen, the problem is left out of the launch.  Every other
# gradient falls out of a kernel that runs anyway (head.1.weight leaves pa_linear_f32_bwd together with its bias)
_WGRAD_MATRICES = ("attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight", "patch_embed.proj.weight")


class _Plan(NamedTuple):
    """What one forward / backward pair of a partly frozen network does, decided when the forward starts (trainable_plan)."""
    stop: int               # the lowest stage the backward reaches; the forward keeps nothing of the blocks below it
    wanted: frozenset       # names of the parameters that get a gradient
    live: frozenset         # stages holding one
    mats: frozenset         # stages holding a wanted weight-gradient GEMM
    dump: tuple             # (name, numel) of the unwanted small parameters of live stages: their reductions land in a scratch buffer
    idx: tuple              # positions of the wanted parameters in the list the plan was made from
    total: int              # their element count


def trainable_plan(model, want_dx=False, low_block=None, named=None, flags=None):
    """The _Plan of ``model`` as its ``requires_grad`` flags stand (``flags``: one bool per entry of ``named``, in place of them).
    ``stop`` is the lowest stage with a trainable parameter (``depth`` when there is none), -1 when the input's gradient is wanted
    (``want_dx``), and at most ``low_block`` when the backward has other work at that block (``attn_grad=``, ``rollout="cam"``)."""
    if named is None:
        named = model._graph_params()[0]
    if flags is None:
        flags = tuple(p.requires_grad for _, p in named)
    key = (flags, bool(want_dx), low_block)
    plans = model._scratch.get("plans")
    if plans is None or plans[0] is not named:
        plans = model._scratch["plans"] = (named, {})
    plan = plans[1].get(key)
    if plan is None:
        depth = len(model.blocks)
        idx = tuple(i for i, f in enumerate(flags) if f)
        wanted = frozenset(named[i][0] for i in idx)
        live = frozenset(param_stage(n, depth) for n in wanted)
        mats = frozenset(param_stage(n, depth) for n in wanted if n.endswith(_WGRAD_MATRICES))
        dump = tuple((n, p.numel()) for n, p in named
                     if n not in wanted and param_stage(n, depth) in live and not n.endswith(_WGRAD_MATRICES))
        stop = -1 if want_dx else min(live, default=depth)
        if low_block is not None:
            stop = min(stop, low_block)
        plan = plans[1][key] = _Plan(stop, wanted, live, mats, dump, idx, sum(named[i][1].numel() for i in idx))
    return plan


def drop_path_rates(model):
    """Per block: the drop probability of its DropPath in training mode, 0.0 for an Identity, a rate of 0 and in eval mode."""
    if not model.training:
        return [0.0] * len(model.blocks)
    return [float(getattr(blk.drop_path, "drop_prob", 0.0) or 0.0) for blk in model.blocks]


def drop_path_draws(model, B, device):
    """The factors of one training forward, (depth, 2, B) f32 on ``device``: [i, 0] the attention branch of block i, [i, 1] its MLP
    branch, entry b = floor(keep + u) / keep of clip b -- 1 / keep (kept) or 0 (dropped) -- and 1 for a block without an active
    DropPath.  u is drawn as the reference's modules draw it: one ``torch.rand((B, 1, 1), dtype=torch.float32, device=device)`` call
    per active module call, blocks ascending, attention branch then MLP branch, so ``device``'s generator is consumed exactly as the
    reference consumes it in fp32.  (Under autocast the reference's branch output is 16-bit and it draws in that type; this path
    always draws f32: the masks then differ from the reference's under the same seed, their distribution does not.)  Eval mode or
    no active module: all ones, nothing drawn."""
    rates = drop_path_rates(model)
    out = torch.ones((len(rates), 2, B), dtype=torch.float32, device=device)
    for i, p in enumerate(rates):
        if p > 0.0:
            keep = 1 - p
            for j in range(2):
                u = torch.rand((B, 1, 1), dtype=torch.float32, device=device)
                out[i, j] = ((keep + u).floor_() / keep).view(B)
    return out


def drop_path_scales(model, masks, B, device):
    """``drop_path_masks`` -- (depth, 2, B) keep flags, 1 keep / 0 drop, any dtype or device -- as drop_path_draws' factors: flag / keep
    for an active module, 1 elsewhere (entries of inactive modules are ignored).  Nothing is drawn."""
    rates = drop_path_rates(model)
    m = torch.as_tensor(masks)
    if tuple(m.shape) != (len(rates), 2, B):
        raise ValueError(f"drop_path_masks must have shape (depth, 2, B) = {(len(rates), 2, B)}, got {tuple(m.shape)}")
    m = m.to(device=device, dtype=torch.float32)
    active = torch.tensor([p > 0.0 for p in rates], device=device).view(-1, 1, 1)
    keep = torch.tensor([1 - p for p in rates], dtype=torch.float32, device=device).view(-1, 1, 1)
    return torch.where(active, m, torch.ones_like(m)) / keep


def attn_drop_rates(model):
    """Per block: t = round(256 p) of its ``attn.attn_drop.p`` (ops.attn_drop_t: the fused attention applies the rate t / 256) in
    training mode; 0 in eval mode, for p == 0 and for a module without ``p`` (an Identity).  A p that rounds past 255 / 256 raises
    ValueError."""
    if not model.training:
        return [0] * len(model.blocks)
    out = []
    for blk in model.blocks:
        p = getattr(getattr(blk.attn, "attn_drop", None), "p", None)
        out.append(ops.attn_drop_t(p) if p else 0)
    return out


class _AttnDrop:
    """A forward's attention dropout: ``seed`` (2,) int32 on the device (read as two uint32 words), ``t`` per block (attn_drop_rates)."""

    def __init__(self, seed, t):
        self.seed, self.t = seed, t

    def kw(self, i):
        """the keyword goes only to the attention launches of a block with an active dropout; site = the block index"""
        return dict(drop=(self.seed, i, self.t[i])) if self.t[i] else {}


def attn_drop_seed_tensor(seed, device):
    """``attn_drop_seed`` -- two Python ints < 2^32 or a (2,) tensor -- as the (2,) int32 device tensor the kernels read."""
    if torch.is_tensor(seed) and seed.dtype == torch.int32 and tuple(seed.shape) == (2,):
        return seed.to(device).contiguous()
    s0, s1 = ops.attn_drop_seed_words(seed)
    return torch.tensor([v - 2 ** 32 if v >= 2 ** 31 else v for v in (s0, s1)], dtype=torch.int32).to(device)


def attn_drop_draw(device):
    """The seed of one training forward: ONE (2,) int32 tensor from ``device``'s default generator (full 32-bit range per word)."""
    return torch.randint(-2 ** 31, 2 ** 31, (2,), dtype=torch.int32, device=device)


def refuse_varlen_attn_drop(model):
    """The refusal of a ragged batch by a model with an active attention dropout (training mode, attn_drop.p > 0), before any draw:
    the packed attention entries have no dropout form."""
    if any(attn_drop_rates(model)):
        raise NotImplementedError("PaSST.forward(x, lengths=...) in training mode with an active attention dropout "
                                  "(blocks[i].attn.attn_drop.p > 0) is not supported: the packed attention kernels have no dropout "
                                  "form (train with equal-length batches, or with attn_drop.p = 0 on ragged ones)")


class _DropRows:
    """A forward's drop-path factors per ROW, expanded once: ``full`` (depth, 2, M) for launches over all token rows (``ntok`` rows per
    clip), ``tail`` (2, 2 B) for the last block on the compact prefix rows (2 per clip); ``active``: the blocks with a factor.
    ``ntok``: the clips' token counts -- one int (the fixed layout: every clip the same), or a (B,) integer tensor on the factors'
    device with ``M``, their sum, known to the host (the packed layout: clip b's factor on all of its rows; no device read)."""

    def __init__(self, scales, rates, ntok, M=None):
        self.active = [p > 0.0 for p in rates]
        if torch.is_tensor(ntok):
            self.full = scales.repeat_interleave(ntok, dim=2, output_size=M).contiguous()
        else:
            self.full = scales.repeat_interleave(ntok, dim=2).contiguous()
        self.tail = scales[-1].repeat_interleave(2, dim=1).contiguous()

    def rows(self, i, branch, compact=False):
        """block i's factor rows for its attention (0) / MLP (1) branch, or None when the block has none"""
        if i < 0 or not self.active[i]:
            return None
        return self.tail[branch] if compact else self.full[i, branch]


def _drop_rows(model, lay, scales):
    """_DropRows of a fixed-layout forward from its (depth, 2, B) factors, or None when no DropPath is active (rate 0, eval)."""
    rates = drop_path_rates(model)
    if scales is None or not any(p > 0.0 for p in rates):
        return None
    return _DropRows(scales, rates, lay.Ntok)


def _forward_trunk(model, lay, xs, dt, save, patch, hidden=None, attn=None, rollout=None, drop=None, adrop=None):
    """Token matrix xs [M][D] f32 in layout ``lay`` -> blocks -> tail -> head.  Returns a _Fwd (tok_offsets left to the caller); ctx
    (``save`` only) is what _backward_trunk needs plus ``patch``, the entry path's own state for its patch-stage backward.
    ``hidden`` (parse_hidden's tuple or None): the token outputs to hand out, in that order -- a block's output is the f32
    residual stream the block wrote (its own fresh buffer, no copy), "norm" the final norm of every row of the last block's output.
    The last block or "norm" among them makes the last block run on all rows (FULL TAIL) instead of the prefix-only tail.
    ``attn`` (parse_attn's triple or None): the attention maps to hand out, in the order asked (layout's
    attention_probs: a shaped tensor, or the packed batch's flat buffer) -- made right behind the block's attention launch from the
    qkv and lse it used.  All rows of the last block's map need the FULL TAIL too; its prefix rows come from the prefix-only tail's
    own compact lse, and the tail is unchanged.
    ``rollout`` (parse_rollout's pair, a _RolloutRequest, or None): "attn" keeps (qkv, lse) of the blocks from its first one on for the
    duration of the call and, behind the last block, runs the chain r <- 0.5 r + 0.5 r A_l from the one-hot cls / dist rows, last block
    first, one pa_attention_rollout step per block; the prefix-only tail's block enters with its two query rows and its own two-row
    lse, which is exact because the start rows are one-hot in the prefix.  A _RolloutRequest ("cam") only gets its start rows here: the
    chain rides with the backward (_backward_trunk).
    ``drop`` (a _DropRows or None): stochastic depth -- both residual GEMMs of a block with a factor add rowscale[m] * branch[m]; a
    block without one, and every block when ``drop`` is None, makes exactly the calls it always made.
    ``adrop`` (an _AttnDrop or None): attention dropout -- the attention launch of a block with t > 0 is the dropout entry with site =
    the block index; every other block, and every block when ``adrop`` is None, launches what it always launched.  Maps and the
    "attn" rollout stay the undropped softmax (they are formed from qkv and lse, which carry no mask).
    ``save``: False, True (keep what a backward down to the patch stage needs) or a _Plan: the blocks below ``plan.stop`` launch what
    they always launch and keep nothing -- their entry of ``ctx["saved"]`` is None and their LayerNorms write no row statistics."""
    st = model._staged
    plan = save if isinstance(save, _Plan) else None
    D, H = model.embed_dim, model.num_heads
    scale = (D // H) ** -0.5
    aflags = ops.ATTN_Q_PRESCALED
    saved = []
    nblk = len(model.blocks)
    want = hidden or ()
    amaps, aprefix, amean = attn or ((), False, False)
    full_tail = (nblk - 1) in want or "norm" in want or ((nblk - 1) in amaps and not aprefix)
    outs, maps = {}, {}
    roll_first = nblk if rollout is None or isinstance(rollout, _RolloutRequest) else rollout[1]
    roll_keep = []                          # (qkv, lse, query rows) of the blocks an "attn" rollout multiplies through
    for bi, blk in enumerate(model.blocks):
        last = bi == nblk - 1
        keep = bool(save) and (plan is None or bi >= plan.stop)
        ln1, mean1, rstd1 = ops.layernorm_fwd(xs, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps, dt, keep)
        # the q third leaves the GEMM as q * scale * log2(e) (one rounding): attention takes "score - row reference"
        # straight from the matrix pipe (ATTN_Q_PRESCALED); every gradient stays the gradient of the unscaled Linear
        qkv = ops.linear(ln1, st.get(blk.attn.qkv.weight, dt, False), blk.attn.qkv.bias, dt,
                         colscale_n=D, colscale=scale * ops.LOG2E)
        kw_d = {} if adrop is None else adrop.kw(bi)
        if not last or full_tail:
            att, lse = lay.attention_fwd(qkv, H, scale, flags=aflags, **kw_d)
            x_res = xs
            if bi in amaps:
                maps[bi] = lay.attention_probs(qkv, lay.prefix_lse(lse, H) if aprefix else lse, H, scale, 2 if aprefix else None,
                                               amean, aflags)
        else:
            # PREFIX-ONLY TAIL.  The network output reads the last block at the cls/dist rows only
            # (models/passt.py:570-574, 583), so from here on just those 2 rows per clip are computed: attention for
            # 2 queries (keys/values still span every token), then proj / LN2 / MLP on [2B, D].  Exact, not an
            # approximation: the reference computes the other N-2 rows and discards them.
            pidx = lay.prefix_rows(xs.device)
            att, lse = lay.attention_fwd(qkv, H, scale, nq=2, flags=aflags, **kw_d)
            x_res = ops.gather_rows(xs, pidx)
            if bi in amaps:                 # aprefix: the two rows this launch produced
                maps[bi] = lay.attention_probs(qkv, lse, H, scale, 2, amean, aflags)
        if bi >= roll_first:
            roll_keep.append((qkv, lse, None if (not last or full_tail) else 2))
        compact = last and not full_tail
        # stochastic depth: the keyword goes only to a block that has a factor
        kw_a = {} if drop is None or drop.rows(bi, 0) is None else dict(rowscale=drop.rows(bi, 0, compact))
        kw_m = {} if drop is None or drop.rows(bi, 1) is None else dict(rowscale=drop.rows(bi, 1, compact))
        x_mid = ops.linear_resid(att, st.get(blk.attn.proj.weight, dt, False), blk.attn.proj.bias, x_res, dt, **kw_a)
        ln2, mean2, rstd2 = ops.layernorm_fwd(x_mid, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps, dt, keep)
        h_pre, h_act = ops.linear_gelu(ln2, st.get(blk.mlp.fc1.weight, dt, False), blk.mlp.fc1.bias, dt)
        x_out = ops.linear_resid(h_act, st.get(blk.mlp.fc2.weight, dt, False), blk.mlp.fc2.bias, x_mid, dt, **kw_m)
        if save:
            saved.append((xs, ln1, mean1, rstd1, qkv, att, lse, x_mid, ln2, mean2, rstd2, h_pre, h_act) if keep else None)
        if bi in want:
            outs[bi] = x_out
        xs = x_out
    tail = None
    if full_tail:
        # FULL TAIL: the last block ran like every other one; the head reads its cls / dist rows
        xl = ops.gather_rows(xs, lay.prefix_rows(xs.device)).view(lay.B, 2, D)
        stats_n = None
        if "norm" in want:
            outs["norm"], mean_n, rstd_n = ops.layernorm_fwd(xs, model.norm.weight, model.norm.bias, model.norm.eps, PA_F32, bool(save))
            stats_n = (mean_n, rstd_n)
        tail = dict(x_last=xs, norm=stats_n)
    else:
        xl = xs.view(lay.B, 2, D)          # compact: the two prefix tokens of every clip
    feat, hn, stats = ops.head_pre_fwd(xl, model.norm.weight, model.norm.bias, model.norm.eps, model.head[0].weight,
                                       model.head[0].bias, model.head[0].eps)
    logits = ops.linear_f32_fwd(hn, model.head[1].weight, model.head[1].bias)
    roll = None
    if rollout is not None:
        roll = lay.rollout_start(xs.device)
        if isinstance(rollout, _RolloutRequest):
            rollout.start = roll
        while roll_keep:                    # later blocks on the left: the row vectors meet the last block first
            qkv, lse, nq = roll_keep.pop()
            roll = lay.attention_rollout(qkv, lse, roll, H, scale, 0.5, 0.5, nq, aflags)
    # tail: None = the prefix-only tail; else the full tail's own state (the last block's output, the final norm's row statistics)
    ctx = dict(dt=dt, lay=lay, scale=scale, saved=saved, xl=xl, feat=feat, hn=hn, stats=stats, patch=patch, tail=tail) if save else None
    if save and drop is not None:
        ctx["drop"] = drop
    if save and adrop is not None:
        ctx["adrop"] = adrop
    if plan is not None:
        ctx["plan"] = plan
    return _Fwd(logits, feat, ctx, tuple(lay.hidden_view(outs[k]) for k in want), tuple(maps[k] for k in amaps), roll=roll)


def _saves_patch(save):
    """Does a forward called with ``save`` (False / True / a _Plan) keep the patch stage's state?  Only a backward that reaches it needs it."""
    return bool(save) and (not isinstance(save, _Plan) or save.stop < 0)


def patchout_draws(model, x_shape):
    """The host part of a forward: geometry checks and the reference's Patchout draws (models/passt.py:513-553, same torch CPU
    RNG calls in the same order), as numpy arrays: the grid coordinates of the kept patches (pf, pt) and the time-positional
    offset.  passt_forward() calls this itself; TrainStep's captured-graph mode calls it ahead of the replay and hands the
    result over in device buffers of fixed address."""
    B, Cin, F, T = x_shape
    P, (fs, ts) = model.patch_embed.patch_size[0], model.patch_embed.stride
    if not (F == model.patch_embed.img_size[0] and T == model.patch_embed.img_size[1]):
        warnings.warn(f"Input image size ({F}*{T}) doesn't match model "
                      f"({model.patch_embed.img_size[0]}*{model.patch_embed.img_size[1]}).")   # :320-321
    F_dim, T_dim = _freq_rows(model, F), (T - P) // ts + 1
    toff, T_eff, idx_t, idx_f, idx_u = draw_patchout(model, F_dim, T_dim)
    pf_np, pt_np = kept_patches(F_dim, T_eff, idx_t, idx_f, idx_u)
    return dict(pf=pf_np, pt=pt_np, toff=toff, Np=pf_np.size)


def passt_forward(model, x, save, draws=None, hidden=None, attn=None, drop_path_masks=None, attn_drop_seed=None):
    """Kernel sequence of PaSST.forward (:576-595).  Returns (logits, features, ctx).  ``save``: False, True (everything a full
    backward needs) or a trainable_plan (what the backward of a partly frozen network needs, see _forward_trunk).  ``draws``: device-resident Patchout
    draws {pf, pt, pt_pos (= pt + time offset), Np} prepared by the caller (captured-graph mode) -- with an active DropPath also
    ``dp``, drop_path_draws' (depth, 2, B) factors; None = draw here.
    ``hidden`` (parse_hidden's tuple): returns (logits, features, ctx, hs), hs = the (B, Ntok, D) f32 token outputs asked for.
    ``attn`` (parse_attn's triple): returns (logits, features, ctx, hs, maps), maps = the attention maps asked for.
    ``drop_path_masks`` ((depth, 2, B) keep flags): used in place of the stochastic-depth draws (PaSST.forward).
    ``attn_drop_seed`` (two ints < 2^32 or a (2,) tensor): used in place of the attention-dropout seed draw (PaSST.forward); with
    ``draws``, an active attention dropout reads its seed from ``draws["ad"]``, a (2,) int32 device tensor."""
    r = _run_forward(model, x, None, save, draws, hidden, attn, drop_path_masks=drop_path_masks,
                     **({} if attn_drop_seed is None else dict(attn_drop_seed=attn_drop_seed)))
    out = (r.logits, r.feat, r.ctx)
    if hidden is not None or attn is not None:
        out += (list(r.hidden),)
    return out if attn is None else out + (list(r.maps),)


def varlen_regularized(model):
    """Does a ragged batch of this model run with its regularisers (``net.varlen_regularize = True`` on a model in training mode with
    an active DropPath or attention dropout)?  False: the packed path is the one without them and the two refusals below hold."""
    return bool(getattr(model, "varlen_regularize", False)) and (any(p > 0.0 for p in drop_path_rates(model))
                                                                   or any(attn_drop_rates(model)))


def refuse_varlen_drop_path(model):
    """The refusal of a ragged batch by a model with an active DropPath (training mode, rate > 0): net(x, lengths=) and
    TrainStep.step(lengths=) raise the same NotImplementedError, the step before any of its draws."""
    if any(p > 0.0 for p in drop_path_rates(model)):
        raise NotImplementedError("PaSST.forward(x, lengths=...) in training mode with drop_path_rate > 0 is not supported: the draw "
                                  "order that gives every clip the masks it would get alone at batch size 1 is not decided yet "
                                  "(train with equal-length batches, or with drop_path_rate = 0 on ragged ones)")


def _run_forward(model, x, lengths=None, save=False, draws=None, hidden=None, attn=None, rollout=None, drop_path_masks=None,
                 attn_drop_seed=None):
    """The one way into the kernel sequence of a forward: the fixed path, or with ``lengths`` the packed one, under this model's GEMM
    flags.  Returns the _Fwd."""
    reg = lengths is not None and varlen_regularized(model)
    if lengths is not None and not reg:
        refuse_varlen_drop_path(model)
        refuse_varlen_attn_drop(model)
    with ops.gemm_flags(getattr(model, "_gemm_flags", 0)):
        if lengths is None:
            if attn_drop_seed is not None:
                return _passt_forward(model, x, save, draws, hidden, attn, rollout, drop_path_masks, attn_drop_seed)
            return _passt_forward(model, x, save, draws, hidden, attn, rollout, drop_path_masks)
        if reg:
            return _passt_forward_varlen(model, x, lengths, save, hidden, attn, rollout, drop_path_masks, attn_drop_seed, True)
        return _passt_forward_varlen(model, x, lengths, save, hidden, attn, rollout)


def _passt_forward(model, x, save, draws=None, hidden=None, attn=None, rollout=None, drop_path_masks=None, attn_drop_seed=None):
    x, dt = _checked_input(model, x, True)
    B, Cin, F, T = x.shape
    P, (fs, ts) = model.patch_embed.patch_size[0], model.patch_embed.stride
    if draws is None:
        d = patchout_draws(model, x.shape)
        pf = ops.upload_small(d["pf"], x.device)         # page-locked staging: asynchronous H2D
        pt = ops.upload_small(d["pt"], x.device)
        pt_pos, toff, Np = pt, d["toff"], d["Np"]        # the positional kernels add the offset themselves
    else:
        pf, pt, pt_pos, toff, Np = draws["pf"], draws["pt"], draws["pt_pos"], 0, draws["Np"]
    D, Ntok = model.embed_dim, Np + 2
    # stochastic depth: behind the Patchout draws, as the reference's blocks run behind its patch stage
    scales = None
    if any(p > 0.0 for p in drop_path_rates(model)):
        if drop_path_masks is not None:
            scales = drop_path_scales(model, drop_path_masks, B, x.device)
        elif draws is not None and draws.get("dp") is not None:
            scales = draws["dp"]
        else:
            scales = drop_path_draws(model, B, x.device)
    # attention dropout: one seed per forward, behind the Patchout and the drop-path draws
    adrop, ad_t = None, attn_drop_rates(model)
    if any(ad_t):
        if attn_drop_seed is not None:
            adrop = _AttnDrop(attn_drop_seed_tensor(attn_drop_seed, x.device), ad_t)
        elif draws is not None and draws.get("ad") is not None:
            adrop = _AttnDrop(draws["ad"], ad_t)
        else:
            adrop = _AttnDrop(attn_drop_draw(x.device), ad_t)

    # patch embedding: gather-first im2col GEMM, epilogue adds bias + time/freq positional rows and
    # scatters to token rows 2.. ; rows 0,1 = cls/dist + new_pos_embed                 (:323,:527-564)
    cols = ops.patch_gather(x, pf, pt, P, fs, ts, dt)
    tok = torch.empty((B, Ntok, D), device=x.device, dtype=torch.float32)
    table = ops.patch_pos_table(model.patch_embed.proj.bias, model.time_new_pos_embed, model.freq_new_pos_embed,
                                pf, pt_pos, toff, model.cls_token, model.dist_token, model.new_pos_embed, tok)
    ops.gemm_nt(cols, model._staged.get(model.patch_embed.proj.weight, dt, False), dt, EPI_RESID, resid=table, out_f32=tok,
                row_mod=Np, out_batch_rows=Ntok, out_row_off=2)
    # pt_grid: the kept patches' own grid columns (pt may carry the time-positional offset); F, T: the input gradient's shape
    patch = dict(Np=Np, pf=pf, pt=pt_pos, pt_grid=pt, toff=toff, F=F, T=T, cols=cols) if _saves_patch(save) else None
    lay = _FixedLayout(model, B, Ntok)
    drop = _drop_rows(model, lay, scales)
    kw = {} if adrop is None else dict(adrop=adrop)
    if drop is None:
        return _forward_trunk(model, lay, tok.view(B * Ntok, D), dt, save, patch, hidden, attn, rollout, **kw)
    return _forward_trunk(model, lay, tok.view(B * Ntok, D), dt, save, patch, hidden, attn, rollout, drop=drop, **kw)


# --------------------------------------------------------------------------------------------
# packed forward for clips of different lengths
# --------------------------------------------------------------------------------------------
def _clip_columns(lengths, P, tstride, T_max):
    """What both ragged geometries check first, clip after clip: yields (clip index, frames, patch columns (len_i - P) // tstride + 1).
    ValueError for an empty batch and for the first clip shorter than one patch or longer than ``T_max``."""
    lens = [int(v) for v in lengths]
    if not lens:
        raise ValueError("lengths is empty")
    for i, n in enumerate(lens):
        if n < P:
            raise ValueError(f"clip {i}: {n} frames are shorter than one patch ({P} frames): no patch column")
        if T_max is not None and n > T_max:
            raise ValueError(f"clip {i}: length {n} exceeds the input's {T_max} frames")
        yield i, n, (n - P) // tstride + 1


def _pack_clips(F_dim, T_eff, clips, slot=False):
    """The token rows of a packed batch.  ``clips``: per clip (pf, pt, toff) -- the grid coordinates of its patches in sequence order
    (kept_patches) and its offset into the time embedding; ``T_eff``: its patch columns.  Clip i owns cls, dist and its patches, the
    clips back to back.  Returns int32 numpy arrays per token row -- ``row_clip`` / ``row_f`` / ``row_t`` (row_f = -1 on the prefix
    rows, row_t = 0 cls / 1 dist there) / ``row_tpos`` (row_t + the clip's offset on the patch rows) -- ``cu_tok`` (B + 1 row offsets),
    ``toff`` (one per clip), plus ``max_N``, ``Tg`` (patch columns of the widest clip) and, asked for with ``slot``, ``slot`` (int32
    [B][F_dim][Tg]: the packed row of patch (f, t) of clip b, -1 where there is none)."""
    B = len(clips)
    ntok = np.array([2 + pf.size for pf, _, _ in clips], dtype=np.int64)
    cu = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(ntok, out=cu[1:])
    M = int(cu[-1])
    if M >= 2 ** 31:
        raise ValueError("packed batch has too many tokens")
    row_clip = np.repeat(np.arange(B, dtype=np.int32), ntok)
    row_f, row_t = np.empty(M, dtype=np.int32), np.empty(M, dtype=np.int32)
    toff = np.array([toff for _, _, toff in clips], dtype=np.int32)
    g = dict(row_clip=row_clip, row_f=row_f, row_t=row_t, cu_tok=cu.astype(np.int32), max_N=int(ntok.max()), toff=toff, Tg=max(T_eff))
    if slot:
        g["slot"] = np.full((B, F_dim, g["Tg"]), -1, dtype=np.int32)
    for i, (pf, pt, _) in enumerate(clips):
        o = int(cu[i])
        row_f[o:o + 2], row_t[o:o + 2] = -1, (0, 1)
        row_f[o + 2:o + 2 + pf.size], row_t[o + 2:o + 2 + pf.size] = pf, pt
        if slot:
            g["slot"][i, pf, pt] = o + 2 + np.arange(pf.size, dtype=np.int32)
    g["row_tpos"] = row_t + toff[row_clip] * (row_f >= 0) if toff.any() else row_t       # without offsets: row_t itself, not a copy
    return g


def varlen_geometry(lengths, P, tstride, F_dim, Tpe, T_max=None):
    """Host geometry of a packed ragged batch (models/passt.py:513-526 per clip, eval mode).  ``lengths``: valid frames per clip.
    Clip i has T_i = (len_i - P) // tstride + 1 patch columns, cut to the time embedding's ``Tpe``; its tokens are cls, dist and
    the F_dim x T_i patches in frequency-major order (:546), and the clips lie back to back.  Returns a dict of int32 numpy arrays
    -- per token row ``row_clip`` / ``row_f`` / ``row_t`` (row_f = -1 on the prefix rows, row_t = 0 cls / 1 dist there), ``cu_tok``
    (B + 1 row offsets) -- plus ``T_eff`` (patch columns kept per clip), ``cut`` (clips whose columns reach or exceed Tpe: the
    reference warns for them) and ``max_N`` (and _pack_clips' other keys: ``row_tpos`` = row_t, ``toff`` = 0, ``Tg``).  ValueError names
    the first clip shorter than one patch or longer than ``T_max``."""
    T_eff, cut = [], []
    for i, n, T_dim in _clip_columns(lengths, P, tstride, T_max):
        if T_dim >= Tpe:
            cut.append(i)
        T_eff.append(min(T_dim, Tpe))
    return dict(_pack_clips(F_dim, T_eff, [kept_patches(F_dim, t, None, None, None) + (0,) for t in T_eff]), T_eff=T_eff, cut=cut)


def varlen_geometry_train(model, lengths, F_dim=None, T_max=None):
    """varlen_geometry for a packed batch in training mode: every clip gets the Patchout it would get alone at batch size 1.  The
    draws are made clip after clip, i = 0 .. B - 1, each with the reference's own torch CPU RNG calls in the reference's order
    (draw_patchout: randint for the time-positional offset when the clip has fewer patch columns than the time embedding, then
    randperm for s_patchout_t, s_patchout_f, u_patchout), so after torch.manual_seed(s) one call leaves the CPU generator where
    the loop ``for i: net(x[i:i+1, :, :, :lengths[i]])`` leaves it, with the same kept patches and offsets.  ``F_dim``: frequency
    rows of the patch grid (default: the frequency embedding's).  Returns varlen_geometry's dict -- ``row_clip`` / ``row_f`` /
    ``row_t`` / ``cu_tok`` / ``T_eff`` / ``cut`` / ``max_N``, the patch rows of a clip being its KEPT patches in sequence order -- plus
    ``row_tpos`` (= row_t + the clip's offset on the patch rows: the column of the time embedding; row_t on the prefix rows),
    ``toff`` (int32, one per clip), ``Tg`` (patch columns of the widest clip) and ``slot`` (int32 [B][F_dim][Tg]: the packed row of the
    kept patch (f, t) of clip b, -1 where there is none).
    ValueError -- BEFORE any RNG call, so a rejected batch consumes nothing -- names the first clip that is shorter than one patch or
    longer than ``T_max``, or that cannot satisfy the configured counts: no more patch columns than s_patchout_t, no more frequency
    rows than s_patchout_f, no more patches left than u_patchout, or structured time Patchout on a clip with more patch columns than
    the time embedding (the reference indexes the cut grid with indices of the uncut one and fails, models/passt.py:536)."""
    if F_dim is None:
        F_dim = model.freq_new_pos_embed.shape[-2]
    T_dims, cut = check_patchout_varlen(model, lengths, F_dim, T_max)
    clips, T_eff = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # draw_patchout's "x will be cut", per clip: the caller warns once, from ``cut``
        for T_dim in T_dims:
            toff, Te, idx_t, idx_f, idx_u = draw_patchout(model, F_dim, T_dim)
            clips.append(kept_patches(F_dim, Te, idx_t, idx_f, idx_u) + (toff,))
            T_eff.append(Te)
    return dict(_pack_clips(F_dim, T_eff, clips, slot=True), T_eff=T_eff, cut=cut)


def check_patchout_varlen(model, lengths, F_dim=None, T_max=None):
    """Every check varlen_geometry_train makes, and nothing else: no RNG call, no launch.  ``lengths``: valid frames per clip.  Returns
    (patch columns per clip, the clips whose columns reach the time embedding's length); raises varlen_geometry_train's ValueErrors,
    clip after clip.  A caller that has more to draw ahead of the Patchout draws (TrainStep.step(lengths=): the front end's, mixup's)
    calls this first, so that a rejected batch consumes no random number."""
    P, ts = model.patch_embed.patch_size[0], model.patch_embed.stride[1]
    Tpe = model.time_new_pos_embed.shape[-1]
    if F_dim is None:
        F_dim = model.freq_new_pos_embed.shape[-2]
    s_t, s_f, u = (int(model.s_patchout_t or 0), int(model.s_patchout_f or 0), int(model.u_patchout or 0)) if model.training else (0, 0, 0)
    T_dims, cut = [], []
    for i, n, T_dim in _clip_columns(lengths, P, ts, T_max):
        if s_t and T_dim <= s_t:
            raise ValueError(f"clip {i}: {T_dim} patch columns ({n} frames) leave nothing after s_patchout_t={s_t}")
        if s_t and T_dim > Tpe:
            raise ValueError(f"clip {i}: {T_dim} patch columns ({n} frames) exceed the time embedding's {Tpe}; structured time Patchout "
                             "cannot be drawn for a clip that is cut (the reference fails at models/passt.py:536)")
        if s_f and F_dim <= s_f:
            raise ValueError(f"clip {i}: {F_dim} frequency rows leave nothing after s_patchout_f={s_f}")
        left = (F_dim - s_f) * ((T_dim - s_t) if s_t else min(T_dim, Tpe))
        if u and u >= left:
            raise ValueError(f"clip {i}: u_patchout={u} needs more than the {left} patches the clip has left ({n} frames)")
        if T_dim >= Tpe:
            cut.append(i)
        T_dims.append(T_dim)
    return T_dims, cut


def passt_forward_varlen(model, x, lengths, save=False):
    """Kernel sequence of the packed forward: every clip gets what it would get alone at batch size 1.  Returns (logits, features);
    ``save=True``: (logits, features, ctx) with what passt_backward_varlen needs.  Without it nothing is kept and the launch sequence is
    the same.  Eval geometry (no Patchout) -- except for a model in training mode with ``varlen_train`` set: then every clip gets its own
    Patchout draws (varlen_geometry_train) and the context carries the slot table the packed patch-stage backward walks.  A model with
    ``varlen_regularize`` set and an active rate draws its stochastic-depth factors and its attention-dropout seed here
    (passt_forward_varlen_replay takes them from the caller)."""
    return passt_forward_varlen_replay(model, x, lengths, save)


def passt_forward_varlen_replay(model, x, lengths, save=False, drop_path_masks=None, attn_drop_seed=None):
    """passt_forward_varlen with passt_forward's two replay keywords, for a model with ``varlen_regularize`` set (PaSST.forward):
    ``drop_path_masks`` ((depth, 2, B) keep flags) in place of the stochastic-depth draws, ``attn_drop_seed`` (two ints < 2^32 or a
    (2,) tensor) in place of the seed draw; None: drawn.  Both are ignored without the switch or without an active rate."""
    r = _run_forward(model, x, lengths, save, drop_path_masks=drop_path_masks, attn_drop_seed=attn_drop_seed)
    return (r.logits, r.feat, r.ctx) if save else (r.logits, r.feat)


def _upload_parts(parts, device):
    """ONE upload of the int32 host arrays ``parts`` (name -> array) laid back to back in the order given; returns name -> the device
    view of that part, in the array's own shape."""
    buf = ops.upload_small(np.concatenate([a.reshape(-1) for a in parts.values()]), device)
    views = buf.split([a.size for a in parts.values()])
    return {name: v.view(a.shape) for (name, a), v in zip(parts.items(), views)}


def _passt_forward_varlen(model, x, lengths, save=False, hidden=None, attn=None, rollout=None, drop_path_masks=None,
                          attn_drop_seed=None, regularize=False):
    """``regularize`` (_run_forward: the model's ``varlen_regularize`` with an active rate): stochastic depth and attention dropout as
    the fixed path applies them to a batch of B clips -- the draws of _passt_forward in its order, behind the per-clip Patchout draws;
    clip b's factor on all of its rows, clip b's attention mask that of sequence b.  False: neither is looked at."""
    x, dt = _checked_input(model, x, save)
    if torch.is_tensor(lengths):
        if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError("lengths must be a sequence of ints or a 1-D integer tensor")
        lengths = lengths.tolist()                   # a device tensor costs one host read here: the geometry is decided on the host
    lengths = [int(v) for v in lengths]
    B, Cin, F, T = x.shape
    if len(lengths) != B:
        raise ValueError(f"lengths has {len(lengths)} entries for a batch of {B} clips")
    P, (fs, ts) = model.patch_embed.patch_size[0], model.patch_embed.stride
    train = model.training and getattr(model, "varlen_train", False)       # Patchout per clip (PaSST.forward lets no other training call in)
    dp_rates = drop_path_rates(model) if regularize else ()
    ad_t = attn_drop_rates(model) if regularize else ()
    dp_on, ad_on = any(p > 0.0 for p in dp_rates), any(ad_t)
    # what the caller handed over for a replay is checked before the first draw (the Patchout draws of the geometry below)
    scales = drop_path_scales(model, drop_path_masks, B, x.device) if dp_on and drop_path_masks is not None else None
    ad_seed = attn_drop_seed_tensor(attn_drop_seed, x.device) if ad_on and attn_drop_seed is not None else None
    if train:
        g = varlen_geometry_train(model, lengths, _freq_rows(model, F), T_max=T)
    else:
        g = varlen_geometry(lengths, P, ts, _freq_rows(model, F), model.time_new_pos_embed.shape[-1], T_max=T)
    if g["cut"]:
        warnings.warn(f"the patches shape of clips {g['cut']} are larger than the expected time encodings "
                      f"{tuple(model.time_new_pos_embed.shape)}, x will be cut")              # :524-526, once per call
    M, cu = g["row_f"].size, g["cu_tok"]
    # one upload: [row_clip | row_f | row_t | cu_tok | prefix rows], in training mode followed by [row_tpos | clip offsets | slot table]
    parts = {k: g[k] for k in ("row_clip", "row_f", "row_t", "cu_tok")}
    parts["pidx"] = (cu[:-1, None] + np.arange(2, dtype=np.int32)[None, :]).reshape(-1).astype(np.int32)
    if train:
        parts.update((k, g[k]) for k in ("row_tpos", "toff", "slot"))
    if dp_on:
        parts["ntok"] = np.diff(cu).astype(np.int32)     # the clips' token counts: the drop-path factors are expanded on the device
    d = _upload_parts(parts, x.device)
    # stochastic depth, then the attention-dropout seed: _passt_forward's draws in its order, behind the Patchout draws
    if dp_on and scales is None:
        scales = drop_path_draws(model, B, x.device)
    adrop = None
    if ad_on:
        adrop = _AttnDrop(attn_drop_draw(x.device) if ad_seed is None else ad_seed, ad_t)

    # patch embedding: the packed im2col has a zero row under every prefix token and the table holds the token there, so the one
    # GEMM with the residual epilogue writes the whole token matrix (no scatter pass)
    cols = ops.patch_gather_varlen(x, d["row_clip"], d["row_f"], d["row_t"], P, fs, ts, dt)
    # eval: the time embedding is read from offset 0, row_t is the column
    table = ops.patch_pos_table_varlen(model.patch_embed.proj.bias, model.time_new_pos_embed, model.freq_new_pos_embed, d["row_f"],
                                       d["row_tpos" if train else "row_t"], model.cls_token, model.dist_token, model.new_pos_embed)
    xs = torch.empty((M, model.embed_dim), device=x.device, dtype=torch.float32)
    ops.gemm_nt(cols, model._staged.get(model.patch_embed.proj.weight, dt, False), dt, EPI_RESID, resid=table, out_f32=xs)
    patch = dict(F=F, T=T, cols=cols) if _saves_patch(save) else None
    if patch is not None and train:
        patch.update(slot=d["slot"], toff=d["toff"])   # Patchout: the patch-stage backward finds a row's grid position through the table
    tok_offsets = torch.from_numpy(cu.astype(np.int64)) if (hidden is not None or attn is not None or rollout is not None) else None
    lay = _PackedLayout(B, M, g["max_N"], d["cu_tok"], d["pidx"], ntok=np.diff(cu))
    kw = {} if adrop is None else dict(adrop=adrop)
    if dp_on:
        kw["drop"] = _DropRows(scales, dp_rates, d["ntok"], M)
    return _forward_trunk(model, lay, xs, dt, save, patch, hidden, attn, rollout, **kw)._replace(tok_offsets=tok_offsets)


# --------------------------------------------------------------------------------------------
# sliding windows over recordings longer than the time embedding (PaSST.forward_windows)
# --------------------------------------------------------------------------------------------
class Windows(NamedTuple):
    """What forward_windows reports per window.  ``logits`` (W, C) / ``features`` (W, D): window w's outputs; ``offsets``: int64 CPU
    tensor of B + 1 entries, recording b owns windows offsets[b]:offsets[b + 1]; ``start`` / ``length``: int64 CPU tensors of W
    entries (frames); ``dropped``: list of (recording, start, length) -- the tail="short" windows shorter than one patch."""
    logits: torch.Tensor
    features: torch.Tensor
    offsets: torch.Tensor
    start: torch.Tensor
    length: torch.Tensor
    dropped: list


def check_window_rule(window, hop, tail, P):
    """The window rule's own refusals (ValueError): ``window`` >= one patch, 1 <= ``hop`` <= ``window``, ``tail`` "align" or "short"."""
    if tail not in ("align", "short"):
        raise ValueError(f"tail must be 'align' or 'short', got {tail!r}")
    if isinstance(window, bool) or isinstance(hop, bool) or int(window) != window or int(hop) != hop:
        raise ValueError(f"window and hop are whole numbers of frames, got window={window!r}, hop={hop!r}")
    if window < P:
        raise ValueError(f"window={window} frames is shorter than one patch ({P} frames)")
    if hop < 1 or hop > window:
        raise ValueError(f"hop={hop} must lie in 1 .. window={window} (a larger hop would skip frames)")


def window_spans(n, window, hop, tail, P):
    """The windows of ONE recording of ``n`` >= P frames: ([(start, length)], [(start, length) dropped]).  n <= window: the one
    window [0, n).  Otherwise K = ceil((n - window) / hop) + 1 windows; "align": starts k * hop for k < K - 1 and the last at
    n - window (every window full, every frame covered); "short": starts k * hop, lengths min(window, n - start), a last window
    shorter than one patch dropped."""
    if n <= window:
        return [(0, n)], []
    K = -(-(n - window) // hop) + 1
    if tail == "align":
        return [(k * hop, window) for k in range(K - 1)] + [(n - window, window)], []
    spans = [(k * hop, min(window, n - k * hop)) for k in range(K)]
    if spans[-1][1] < P:
        return spans[:-1], spans[-1:]
    return spans, []


def _pack_windows(F_dim, P, tstride, win_src, win_t0, win_len):
    """_pack_clips over windows: every window is a sequence of its own (cls, dist, F_dim x ((len - P) // tstride + 1) patches, the time
    embedding from offset 0); ``row_clip`` is the window index.  Adds ``win_src`` / ``win_t0`` / ``win_len`` (int32)."""
    T_eff = [(int(n) - P) // tstride + 1 for n in win_len]
    grids = {t: kept_patches(F_dim, t, None, None, None) + (0,) for t in set(T_eff)}
    g = _pack_clips(F_dim, T_eff, [grids[t] for t in T_eff])
    g.update(T_eff=T_eff, win_src=np.asarray(win_src, dtype=np.int32), win_t0=np.asarray(win_t0, dtype=np.int32),
             win_len=np.asarray(win_len, dtype=np.int32))
    return g


def window_geometry(lengths, window, hop, tail, P, tstride, F_dim):
    """Host geometry of forward_windows: the windows of every recording (window_spans), recording after recording, as ONE packed
    batch.  ``lengths``: valid frames per recording.  Returns _pack_clips' dictionary over the windows (``row_clip`` = the window of
    a token row, ``row_f`` / ``row_t`` / ``cu_tok`` / ``max_N`` / ...) plus, per window, ``win_src`` (recording), ``win_t0`` (first frame),
    ``win_len`` (frames) as int32 arrays, ``T_eff`` (patch columns), ``offsets`` (int64, B + 1: recording b owns windows
    offsets[b]:offsets[b + 1]) and ``dropped`` ([(recording, start, length)], tail="short" only).  ValueError for a bad window rule
    (check_window_rule), an empty batch, and the first recording shorter than one patch."""
    check_window_rule(window, hop, tail, P)
    window, hop = int(window), int(hop)
    lens = [int(v) for v in lengths]
    if not lens:
        raise ValueError("lengths is empty")
    src, t0, ln, dropped, offsets = [], [], [], [], [0]
    for b, n in enumerate(lens):
        if n < P:
            raise ValueError(f"recording {b}: {n} frames are shorter than one patch ({P} frames): no window")
        spans, gone = window_spans(n, window, hop, tail, P)
        src += [b] * len(spans)
        t0 += [s for s, _ in spans]
        ln += [m for _, m in spans]
        dropped += [(b, s, m) for s, m in gone]
        offsets.append(len(src))
    g = _pack_windows(F_dim, P, tstride, src, t0, ln)
    g.update(offsets=np.asarray(offsets, dtype=np.int64), dropped=dropped)
    return g


def window_chunks(ntok, max_tokens):
    """Windows in order into chunks of at most ``max_tokens`` packed tokens (None: one chunk); a single larger window is a chunk of
    its own.  ``ntok``: tokens per window.  Returns [(first window, one past the last)]."""
    if max_tokens is None:
        return [(0, len(ntok))]
    chunks, lo, used = [], 0, 0
    for w, n in enumerate(ntok):
        if w > lo and used + n > max_tokens:
            chunks.append((lo, w))
            lo, used = w, 0
        used += n
    chunks.append((lo, len(ntok)))
    return chunks


def check_window_call(model, x, lengths, window, hop, tail, pool, pool_of, max_tokens):
    """Every refusal of forward_windows, on the host, before anything is launched or uploaded.  Returns (lengths as ints, window,
    hop) with the defaults filled in: window = the model's img_size[1], hop = window // 2."""
    if model.training:
        raise NotImplementedError("PaSST.forward_windows: eval mode only (sliding windows are an inference entry; call net.eval())")
    if pool not in ("mean", "max", None):
        raise ValueError(f"pool must be 'mean', 'max' or None, got {pool!r}")
    if pool_of not in ("logits", "sigmoid"):
        raise ValueError(f"pool_of must be 'logits' or 'sigmoid', got {pool_of!r}")
    if max_tokens is not None and (isinstance(max_tokens, bool) or int(max_tokens) != max_tokens or max_tokens < 1):
        raise ValueError(f"max_tokens must be a positive int or None, got {max_tokens!r}")
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 1:
        raise ValueError(f"PaSST.forward_windows expects (B, 1, n_mels, frames) recordings, got {tuple(getattr(x, 'shape', ()))}")
    B, _, F, T = x.shape
    P, ts = model.patch_embed.patch_size[0], model.patch_embed.stride[1]
    if window is None:
        window = model.patch_embed.img_size[1]
    if hop is None:
        hop = window // 2
    check_window_rule(window, hop, tail, P)
    Tpe = model.time_new_pos_embed.shape[-1]
    if (window - P) // ts + 1 > Tpe:
        raise ValueError(f"window={window} frames has {(window - P) // ts + 1} patch columns, more than the time embedding's {Tpe}: "
                         "windows are never cut")
    if lengths is None:
        lengths = [T] * B
    elif torch.is_tensor(lengths):
        if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
            raise ValueError("lengths must be a sequence of ints or a 1-D integer tensor")
        lengths = lengths.tolist()
    lengths = [int(v) for v in lengths]
    if len(lengths) != B:
        raise ValueError(f"lengths has {len(lengths)} entries for a batch of {B} recordings")
    for b, n in enumerate(lengths):
        if n > T:
            raise ValueError(f"recording {b}: length {n} exceeds the input's {T} frames")
    return lengths, int(window), int(hop)


def pool_windows(logits, features, offsets, pool, pool_of):
    """Per-window (W, C) logits and (W, D) features -> per-recording (B, C), (B, D): one pa_window_pool launch each.  ``pool_of`` =
    "sigmoid" pools sigmoid(logits); the features are always pooled raw.  ``pool`` None: the per-window tensors themselves."""
    if pool is None:
        return logits, features
    return (ops.window_pool(logits, offsets, pool, "sigmoid" if pool_of == "sigmoid" else None),
            ops.window_pool(features, offsets, pool, None))


def _passt_forward_windows(model, x, lengths, window, hop, tail, max_tokens):
    """Kernel sequence of forward_windows behind check_window_call: per chunk one upload of the index arrays, the window gather, the
    packed positional table, the patch GEMM and _forward_trunk on a _PackedLayout whose sequences are the windows.  Returns a
    Windows with the per-window outputs."""
    P, (fs, ts) = model.patch_embed.patch_size[0], model.patch_embed.stride
    F_dim = _freq_rows(model, x.shape[2])
    g = window_geometry(lengths, window, hop, tail, P, ts, F_dim)
    ntok = np.diff(g["cu_tok"].astype(np.int64))
    chunks = window_chunks(ntok.tolist(), max_tokens)
    x, dt = _checked_input(model, x, False)
    lo_parts, fe_parts = [], []
    with torch.no_grad(), ops.gemm_flags(getattr(model, "_gemm_flags", 0)):
        for lo, hi in chunks:
            c = g if len(chunks) == 1 else _pack_windows(F_dim, P, ts, g["win_src"][lo:hi], g["win_t0"][lo:hi], g["win_len"][lo:hi].tolist())
            cu, M = c["cu_tok"], c["row_f"].size
            # one upload: [row_win | row_f | row_t | cu_tok | prefix rows | win_src | win_t0 | win_len]
            parts = {k: c[k] for k in ("row_clip", "row_f", "row_t", "cu_tok")}
            parts["pidx"] = (cu[:-1, None] + np.arange(2, dtype=np.int32)[None, :]).reshape(-1).astype(np.int32)
            parts.update((k, c[k]) for k in ("win_src", "win_t0", "win_len"))
            d = _upload_parts(parts, x.device)
            # the packed path of _passt_forward_varlen from here on: only the gather knows that a sequence is a window
            cols = ops.patch_gather_windows(x, d["win_src"], d["win_t0"], d["win_len"], d["row_clip"], d["row_f"], d["row_t"], P, fs, ts, dt)
            table = ops.patch_pos_table_varlen(model.patch_embed.proj.bias, model.time_new_pos_embed, model.freq_new_pos_embed, d["row_f"],
                                               d["row_t"], model.cls_token, model.dist_token, model.new_pos_embed)
            xs = torch.empty((M, model.embed_dim), device=x.device, dtype=torch.float32)
            ops.gemm_nt(cols, model._staged.get(model.patch_embed.proj.weight, dt, False), dt, EPI_RESID, resid=table, out_f32=xs)
            lay = _PackedLayout(hi - lo, M, c["max_N"], d["cu_tok"], d["pidx"], ntok=ntok[lo:hi])
            r = _forward_trunk(model, lay, xs, dt, False, None)
            lo_parts.append(r.logits)
            fe_parts.append(r.feat)
    logits = lo_parts[0] if len(lo_parts) == 1 else torch.cat(lo_parts)
    feat = fe_parts[0] if len(fe_parts) == 1 else torch.cat(fe_parts)
    return Windows(logits, feat, torch.from_numpy(g["offsets"].copy()), torch.from_numpy(g["win_t0"].astype(np.int64)),
                   torch.from_numpy(g["win_len"].astype(np.int64)), list(g["dropped"]))


class _NoRowJobs(list):
    """``defer`` sink of the no-weight-gradients backward: deferred row reductions are dropped, nothing finishes them."""

    def append(self, job):
        pass


class _SideStream:
    """Weight-gradient GEMMs and bias-gradient reductions are off the input-gradient critical path: they run
    on a second HIP stream so their workgroups interleave with the dgrad / LayerNorm / attention kernels
    (fills tile-quantisation tails, overlaps epilogue write bursts with compute).  ``fork(*tensors)`` orders the
    side stream after everything enqueued so far on the main stream; ``join()`` makes the main stream wait."""

    def __init__(self, device, enabled=True):
        self.enabled = enabled and torch.cuda.is_available()
        self.stream = torch.cuda.Stream(device=device) if self.enabled else None

    def fork(self, *tensors):
        if not self.enabled:
            return torch.cuda.stream(None)
        self.stream.wait_stream(torch.cuda.current_stream())
        for t in tensors:
            if t is not None:
                t.record_stream(self.stream)          # caching-allocator safety across streams
        return torch.cuda.stream(self.stream)

    def join(self):
        if self.enabled:
            torch.cuda.current_stream().wait_stream(self.stream)


class _NoGrads(dict):
    """``grads`` of the no-weight-gradients backward: every parameter's output buffer is None."""

    def __missing__(self, name):
        return None


class _PlanGrads(dict):
    """``grads`` of a partly frozen backward: a wanted parameter's output buffer; for an unwanted small parameter of a live stage a
    piece of a scratch buffer (its reduction falls out of a kernel that runs anyway, and those kernels take all their outputs or
    none); None for everything else -- the frozen weight matrices, and every parameter of a stage without a trainable one."""

    def __init__(self, grads, dump):
        super().__init__(grads)
        self.dump = dump

    def __missing__(self, name):
        return self.dump.get(name)


def _dump_views(model, plan, device):
    """name -> f32 view for ``plan.dump``, cut from one scratch buffer (kept per model and plan)."""
    hit = model._scratch.get("grad_dump")
    if hit is None or hit[0] is not plan or hit[1].device != device:
        buf = torch.empty(sum(n for _, n in plan.dump), device=device, dtype=torch.float32)
        views = dict(zip((name for name, _ in plan.dump), buf.split([n for _, n in plan.dump]))) if plan.dump else {}
        hit = model._scratch["grad_dump"] = (plan, buf, views)
    return hit[2]


class _WgradSchedule:
    """Where and when the parameter gradients of ONE backward go out -- the side stream, the per-block batching, the deferred row
    reductions, who produces which bias gradient, the ``on_block_done`` reports -- decided here, once per call, for both token
    layouts.  Every A/B switch of the backward is read here, per call (a test toggles one between two models of one process).
    ``g``: the parameter-name -> output-buffer dict, all None when ``grads`` is None (frozen: no weight-gradient work at all).
    ``plan`` (the forward's _Plan, or None: every stage as ``grads`` says): the backward ends behind stage ``stop``, and ``enter(s)``
    makes stage s the current one -- ``frozen`` (no weight-gradient work, deferred reductions dropped, no report) when it holds no
    trainable parameter."""

    def __init__(self, model, dt, grads, on_block_done, device, plan=None):
        self.dt, self.scratch = dt, model._scratch
        self.frozen = frozen = grads is None
        self.plan, self.stop = plan, -1 if plan is None else plan.stop
        if frozen:
            self.g = _NoGrads()
        else:
            self.g = grads if plan is None else _PlanGrads(grads, _dump_views(model, plan, device))
        self.on_block_done = None if frozen else on_block_done
        overlap = getattr(model, "overlap_wgrad", False)
        side = self.scratch.get("side")
        if side is None or side.enabled != bool(overlap):
            side = self.scratch["side"] = _SideStream(device, enabled=overlap)
        self.side = side
        env = os.environ.get
        self.fused_bias = not env("PASST_AMD_NO_FUSED_BIAS")
        # bf16, single stream: the four weight gradients of a block wait until the block's last operand exists and go out as
        # ONE batched launch (+ one batched split-K reduction): no drain / prologue between them, equal-sized work items
        self.pending = [] if (dt == PA_BF16 and not side.enabled and not frozen and not env("PASST_AMD_NO_BATCH_WGRAD")) else None
        # ... and so do the block's small finishing reductions: the two LayerNorms' dgamma | dbeta (+ the bias gradient each carries)
        # and the GELU' epilogue's fc1.bias rows stay as partial rows and are reduced by the SAME finishing launch as the split-K
        # slabs (three launches per block less; PASST_AMD_NO_DEFER_ROWS=1: A/B, every reduction right behind its producer)
        self.rowjobs = [] if (self.pending is not None and not env("PASST_AMD_NO_DEFER_ROWS")) else None
        if frozen:
            self.rowjobs = _NoRowJobs()     # the LayerNorm backward leaves its parameter-gradient partial rows unreduced
        # PASST_AMD_BIAS_FROM_WGRAD=1 (A/B; required by PA_EPILOGUE_V3=1): fc1.bias out of the weight-gradient launch instead of the
        # GELU' epilogue's lane-local column sums
        self.bias_from_wgrad = (dt == PA_BF16 and ops.wgrad_tn_fuses_bias(dt) and self.fused_bias
                                and (env("PASST_AMD_BIAS_FROM_WGRAD") == "1" or env("PA_EPILOGUE_V3") == "1"))
        self._all_frozen, self._rowjobs = frozen, self.rowjobs

    def is_frozen(self, s):
        """does stage s run without any parameter-gradient work?"""
        return self._all_frozen or (self.plan is not None and s not in self.plan.live)

    def wants(self, name):
        """does parameter ``name`` get a gradient from this backward?"""
        return not self._all_frozen and (self.plan is None or name in self.plan.wanted)

    def enter(self, s):
        """Stage s begins.  A stage whose weight matrices are all frozen has no finishing launch for deferred rows to ride in:
        its small reductions go out right behind their producers."""
        self.frozen = self.is_frozen(s)
        if self.frozen:
            self.rowjobs = _NoRowJobs()
        elif self.plan is not None and s not in self.plan.mats:
            self.rowjobs = None
        else:
            self.rowjobs = self._rowjobs

    def report(self, i):
        if self.on_block_done and not self.frozen:
            self.on_block_done(i)

    def launch_async(self, dY, X, dW, db, done=None):
        """dW[N][K] = dY^T X, db[N] = colsum(dY) from row-major dY[M][N], X[M][K], both read in place (pa_gemm_tn: transpose-read
        MFMA operands, deterministic split-K over tokens), on the side stream; optionally report block completion from there
        (DDP bucket launch)."""
        if self.frozen:
            return
        with self.side.fork(dY, X):
            fused = dW is not None and db is not None and ops.wgrad_tn_fuses_bias(self.dt) and self.fused_bias
            if dW is not None:          # None: a frozen matrix in a stage that has trainable parameters
                self.scratch["part"] = ops.wgrad_tn(dY, X, dW.view(dY.shape[1], -1), self.dt, False, self.scratch.get("part"),
                                                    db=db if fused else None)
            if db is not None and not fused:
                ops.colsum(dY, db, accumulate=False)
            if done is not None:
                self.report(done)

    def launch(self, dY, X, dW, db, done=None, fuse=False):
        """A block's weight gradient: into the block's batched launch where there is one (``done`` = block index: this is the
        block's last, send the batch), else launch_async."""
        if self.frozen:
            return
        pending = self.pending
        if pending is None:
            return self.launch_async(dY, X, dW, db, done)
        # the block's last problem (qkv) -- and fc1, `fuse` -- get their bias gradient out of the batched launch itself (a
        # ninth MFMA per phase in the tiles of the first X-column block); the compact fc2 of the last block uses the
        # column-sum kernel right away
        # a frozen matrix (dW None) is no problem of the launch; a bias gradient it would have carried is summed on its own
        fused_bias = dW is not None and (done is not None or fuse) and db is not None and self.fused_bias
        if dW is not None:
            pending.append((dY, X, dW.view(dY.shape[1], -1), False, db if fused_bias else None))
        if db is not None and not fused_bias:
            ops.colsum(dY, db)
        if done is not None:
            if pending:
                self.scratch["part"] = ops.wgrad_tn_batched(pending, self.dt, self.scratch.get("part"), row_jobs=self.rowjobs)
            pending.clear()
            if self.rowjobs is not None:
                self.rowjobs.clear()
            self.report(done)


def _backward_trunk(model, ctx, dlogits, dfeat, wg):
    """Head stage, then blocks depth-1 .. 0 of either token layout.  Returns the gradient of the token matrix [M][D] f32 and its
    16-bit copy (None where the layout's patch stage does not ask for one: ``lay.dx0_lp``).
    ``ctx["dhidden"]`` (optional, put there by the caller): {block index or "norm": gradient [M][D] f32} of the token outputs the
    forward handed out that fed the loss; an output that did not is simply absent.  A
    block's enters the residual stream where that block's output gradient is formed: inside the next block's norm1 backward (its
    second addend; the 16-bit copy and the column sums = this block's fc2.bias gradient see it), or, for the last block of a full
    tail, in pa_tail_inject together with the final norm's backward and the head's prefix-row gradient.
    ``ctx["drop"]`` (a _DropRows, put there by a forward with an active DropPath): the gradient that enters a branch carries that
    branch's row factor -- block i's norm2 backward scales its copy and column sums (proj) by block i's attention factor, block i's
    norm1 backward by block i - 1's MLP factor (fc2 of block i - 1), the head's gradient enters the last block's MLP branch through a
    scaled copy; dx, the residual gradient, is never scaled.  Everything downstream of a copy (d_pre, d_att, the attention backward,
    the maps' gradients, the weight and bias gradients) sees the scaled gradient by construction."""
    dt, lay, st, scratch = ctx["dt"], ctx["lay"], model._staged, model._scratch
    drop = ctx.get("drop")
    adrop = ctx.get("adrop")                # a forward with an active attention dropout: the same seed, site and t go to the backward

    def factor(i, branch, compact=False):       # the keyword goes only to a launch whose branch has a factor
        rows = None if drop is None else drop.rows(i, branch, compact)
        return {} if rows is None else dict(rowscale=rows)
    B, D, H = lay.B, model.embed_dim, model.num_heads
    nblk = len(model.blocks)
    g = wg.g
    wg.enter(nblk)
    rowjobs = wg.rowjobs
    # head: logits = hn W^T + b ; hn = LN_1e-5(feat) ; feat = mean of the two normed prefix tokens
    dhn = ops.linear_f32_bwd(dlogits.contiguous(), ctx["hn"], model.head[1].weight, g["head.1.weight"],
                             g["head.1.bias"])
    dxl, part = ops.head_pre_bwd(dhn, dfeat, ctx["xl"], ctx["feat"], model.norm.weight, model.head[0].weight,
                                 ctx["stats"])
    part4 = part.view(B, 4, D)
    for j, name in enumerate(("head.0.weight", "head.0.bias", "norm.weight", "norm.bias")):
        if not wg.frozen:
            ops.colsum_f32(part4[:, j, :], g[name])
    dh, tail = ctx.get("dhidden") or {}, ctx["tail"]
    ag = ctx.get("attn_grad")               # the _AttnGradRequest of a forward run with attn_grad=, put there by the caller
    rr = ctx.get("rollout")                 # the _RolloutRequest of a forward run with rollout="cam", put there by the caller
    roll = None if rr is None else rr.start
    d_norm = None
    if "norm" in dh:
        # the final norm over ALL rows: its dgamma / dbeta add to what the head's own two rows per clip just gave norm.weight / norm.bias
        mean_n, rstd_n = tail["norm"]
        d_norm, _ = ops.layernorm_bwd(dh["norm"], tail["x_last"], model.norm.weight, mean_n, rstd_n, None, g["norm.weight"],
                                      g["norm.bias"], False, **(dict(defer=rowjobs) if wg.frozen else dict(accumulate=True)))
    wg.report(nblk)
    stop = wg.stop
    if stop >= nblk:                        # only the final norm and the head are trainable: the backward ends here
        return None, None
    if tail is None:
        dx = dxl.view(2 * B, D)             # gradient w.r.t. the compact (prefix-rows) output of the last block
        dx_lp = ops.convert(dx, dt, **factor(nblk - 1, 1, True))
    else:
        # FULL TAIL: gradient w.r.t. all M rows of the last block's output, f32 and 16-bit, in one pass
        dx, dx_lp = ops.tail_inject(dxl.view(2 * B, D), lay.prefix_rows(dxl.device), lay.M, dh.get(nblk - 1), d_norm, dt)
        if factor(nblk - 1, 1):             # the copy that enters the last block's MLP branch carries that branch's factor
            dx_lp = ops.convert(dx, dt, **factor(nblk - 1, 1))
    for i in range(nblk - 1, max(stop, 0) - 1, -1):
        blk = model.blocks[i]
        last = i == nblk - 1
        prefix_tail = last and tail is None
        pfx = f"blocks.{i}."
        wg.enter(i)
        rowjobs = wg.rowjobs
        xs, ln1, mean1, rstd1, qkv, att, lse, x_mid, ln2, mean2, rstd2, h_pre, h_act = ctx["saved"][i]
        # ---- MLP:  x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))      (on [2B, D] rows for the last block of a prefix-only tail)
        # fc2.bias gradient = column sums of dx: already produced by the LayerNorm backward that made dx (the next
        # block's norm1) -- except for the last block, whose dx comes from the head
        # (or the block above is frozen while this one wants it: a frozen stage reduces nothing)
        fc2_bias_here = last or (wg.is_frozen(i + 1) and wg.wants(pfx + "mlp.fc2.bias"))
        wg.launch(dx_lp, h_act, g[pfx + "mlp.fc2.weight"], g[pfx + "mlp.fc2.bias"] if fc2_bias_here else None)
        # the fc1.bias gradient (column sums of d_pre) comes out of the GELU' epilogue -- unless it rides in the weight-gradient
        # launch, like qkv.bias (the LDS-free GELU' epilogue -- transposed accumulators, lane = token -- has no lane-local column
        # sums to offer), or nobody wants it
        from_epilogue, colsum_args = not (wg.bias_from_wgrad or wg.frozen), {}
        if from_epilogue:
            cws = scratch["colsum_ws"] = ops.gemm_colsum_ws(h_pre.shape[0], h_pre.shape[1], dx_lp.device, scratch.get("colsum_ws"))
            colsum_args = dict(colsum_out=g[pfx + "mlp.fc1.bias"], colsum_ws=cws, defer=rowjobs)
        d_pre = ops.dgelu_gemm(dx_lp, st.get(blk.mlp.fc2.weight, dt, True), h_pre, dt, **colsum_args)
        wg.launch(d_pre, ln2, g[pfx + "mlp.fc1.weight"], None if from_epilogue else g[pfx + "mlp.fc1.bias"], fuse=not from_epilogue)
        d_ln2 = torch.empty_like(ln2)
        ops.gemm_nt(d_pre, st.get(blk.mlp.fc1.weight, dt, True), dt, EPI_STORE, out_lp=d_ln2)
        del d_pre
        dx, dx_lp = ops.layernorm_bwd(d_ln2, x_mid, blk.norm2.weight, mean2, rstd2, dx, g[pfx + "norm2.weight"],
                                      g[pfx + "norm2.bias"], True, dcolsum=g[pfx + "attn.proj.bias"], defer=rowjobs,
                                      **factor(i, 0, prefix_tail))
        # ---- attention:  x_mid = x_in + proj(attn(qkv(LN1(x_in))))      (proj.bias gradient came out of LN2' above)
        wg.launch(dx_lp, att, g[pfx + "attn.proj.weight"], None)
        d_att = torch.empty_like(att)
        ops.gemm_nt(dx_lp, st.get(blk.attn.proj.weight, dt, True), dt, EPI_STORE, out_lp=d_att)
        kw_d = {} if adrop is None else adrop.kw(i)
        want_map_grad = ag is not None and i in ag.triple[0]       # the map's gradient: right behind the attention backward, from what it read
        if not prefix_tail:
            d_qkv = lay.attention_bwd(qkv, att, d_att, lse, H, ctx["scale"], flags=ops.ATTN_Q_PRESCALED, **kw_d)
            if want_map_grad:
                _map_grad(lay, ag, ag.triple[0].index(i), qkv, lse, d_att, H, ctx["scale"], False)
            if rr is not None and i >= rr.first:
                roll = _rollout_cam_step(lay, rr, roll, qkv, lse, d_att, H, ctx["scale"], False)
        else:
            # only 2 queries per sequence carry a gradient (the Q third of d_qkv is zero elsewhere); the residual gradient lives
            # on the prefix rows only
            d_qkv = lay.attention_bwd(qkv, att, d_att, lse, H, ctx["scale"], nq=2, flags=ops.ATTN_Q_PRESCALED, **kw_d)
            if want_map_grad:
                _map_grad(lay, ag, ag.triple[0].index(i), qkv, lse, d_att, H, ctx["scale"], True)
            if rr is not None and i >= rr.first:
                roll = _rollout_cam_step(lay, rr, roll, qkv, lse, d_att, H, ctx["scale"], True)
        if i == stop and not (wg.wants(pfx + "norm1.weight") or wg.wants(pfx + "norm1.bias")):
            # the backward ends behind this block and its norm1 is frozen: nobody reads the gradient of the block's input
            wg.launch(d_qkv, ln1, g[pfx + "attn.qkv.weight"], g[pfx + "attn.qkv.bias"], done=i)
            break
        dres = dx if not prefix_tail else ops.scatter_rows_into_zeros(dx, lay.prefix_rows(dx.device), lay.M)
        d_ln1 = torch.empty_like(ln1)
        ops.gemm_nt(d_qkv, st.get(blk.attn.qkv.weight, dt, True), dt, EPI_STORE, out_lp=d_ln1)
        # a loss on the previous block's output: this LayerNorm's input (dropped where the backward ends: it reaches nothing trainable)
        inject = dh.get(i - 1) if i > max(stop, 0) else None
        if inject is None:
            dx, dx_lp = ops.layernorm_bwd(d_ln1, xs, blk.norm1.weight, mean1, rstd1, dres, g[pfx + "norm1.weight"],
                                          g[pfx + "norm1.bias"], i > 0 or lay.dx0_lp,
                                          dcolsum=g[f"blocks.{i - 1}.mlp.fc2.bias"] if i > 0 else None, defer=rowjobs,
                                          **factor(i - 1, 1))
        else:
            dx, dx_lp = ops.layernorm_bwd2(d_ln1, xs, blk.norm1.weight, mean1, rstd1, dres, inject, g[pfx + "norm1.weight"],
                                           g[pfx + "norm1.bias"], True, dcolsum=g[f"blocks.{i - 1}.mlp.fc2.bias"], defer=rowjobs,
                                           **factor(i - 1, 1))
        # last weight gradient of the block; the side stream (ordered after the LayerNorm gradients above)
        # then reports the block complete, so its all-reduce bucket starts without stalling the main stream
        wg.launch(d_qkv, ln1, g[pfx + "attn.qkv.weight"], g[pfx + "attn.qkv.bias"], done=i)
    if rr is not None:
        rr.result = roll
    return dx, dx_lp


def _rollout_cam_step(lay, rr, roll, qkv, lse, d_att, H, scale, prefix_tail):
    """One step r <- r + r mean_h relu(A_l * dA_l) of the gradient-weighted rollout, from what the block's attention backward just
    read (one pa_attention_rollout launch in CAM mode; no map and no gradient of one is formed).  The prefix-only tail hands over its
    compact d_att and two-row lse with nq = 2: only its cls / dist query rows carry a gradient, and the rows are one-hot there."""
    return lay.attention_rollout(qkv, lse, roll, H, scale, 1.0, 1.0, 2 if prefix_tail else None, ops.ATTN_Q_PRESCALED, d_o=d_att,
                                 mode=ops.ATTN_ROLLOUT_CAM, g_scale=rr.g_scale, do_compact=prefix_tail)


def _map_grad(lay, ag, j, qkv, lse, d_att, H, scale, prefix_tail):
    """.grad of the j-th requested attention map, from what its block's attention backward just read: the gradient with respect to
    the probabilities ("grad") or relu(map * gradient) ("cam", with the head mean where the map has it), one pa_attention_probs_grad
    launch.  Prefix rows below a prefix-only tail read the first two rows per clip of the token-row d_att and, for "cam", the lse cut
    to those rows as the map's own launch had it; the prefix-only tail hands over its compact d_att and two-row lse as they are."""
    _, aprefix, amean = ag.triple
    cam = ag.mode == "cam"
    if not cam:
        lse = None
    elif aprefix and not prefix_tail:
        lse = lay.prefix_lse(lse, H)
    g = lay.attention_probs_grad(qkv, lse, d_att, H, scale, 2 if aprefix else None, amean, ops.ATTN_Q_PRESCALED,
                                 ops.ATTN_PGRAD_CAM if cam else ops.ATTN_PGRAD_GRAD, prefix_tail)
    target = ag.targets[j]
    if isinstance(target, list):            # packed: one flat buffer, cut like the map
        tok = torch.tensor([0] + [t.shape[-1] for t in target]).cumsum(0)
        for t, v in zip(target, _PackedLayout.attn_views(g, tok, H, aprefix, amean)):
            t.grad = v
    else:
        target.grad = g


def _patch_backward(model, ctx, wg, dx, dx_lp, want_dx):
    """Patch embedding / positional parameters / prefix tokens of the fixed layout (also when frozen: pa_patch_bwd makes the
    compact dpatch the input gradient starts from), then the input spectrogram's gradient."""
    dt, lay, p, g, st = ctx["dt"], ctx["lay"], ctx["patch"], wg.g, model._staged
    Tpe, Fpe = model.time_new_pos_embed.shape[-1], model.freq_new_pos_embed.shape[-2]
    dpatch = ops.patch_bwd(dx.view(lay.B, lay.Ntok, -1), p["pf"], p["pt"], p["toff"], Tpe, Fpe, g["cls_token"],
                           g["dist_token"], g["new_pos_embed"], g["patch_embed.proj.bias"],
                           g["time_new_pos_embed"], g["freq_new_pos_embed"], dt)
    wg.launch_async(dpatch, p["cols"], g["patch_embed.proj.weight"], None, done=-1)
    if not want_dx:
        return None
    # dcols = dpatch W (the im2col GEMM mirrored), then the fold of the kept patches
    P, (fs, ts) = model.patch_embed.patch_size[0], model.patch_embed.stride
    dcols = torch.empty((lay.B * p["Np"], P * P), device=dpatch.device, dtype=dpatch.dtype)
    ops.gemm_nt(dpatch, st.get(model.patch_embed.proj.weight, dt, True), dt, EPI_STORE, out_lp=dcols)
    return ops.patch_input_bwd(dcols, p["pf"], p["pt_grid"], lay.B, p["F"], p["T"], P, fs, ts)


def _patch_backward_varlen(model, ctx, wg, dx, dx_lp, want_dx):
    """The packed layout's patch stage: dx is the packed dtok [M][D].  The packed im2col has a zero row under every prefix token, so
    both GEMMs run over all M rows of dx_lp: no compaction pass."""
    dt, lay, p, g, st = ctx["dt"], ctx["lay"], ctx["patch"], wg.g, model._staged
    Tpe, Fpe = model.time_new_pos_embed.shape[-1], model.freq_new_pos_embed.shape[-2]
    slot = p.get("slot")                             # training mode (Patchout): the rows of a clip are not a regular grid
    if not wg.frozen:
        d_pos = (g["cls_token"], g["dist_token"], g["new_pos_embed"], g["patch_embed.proj.bias"], g["time_new_pos_embed"],
                 g["freq_new_pos_embed"])
        if slot is None:
            ops.patch_bwd_varlen(dx, lay.cu_tok, lay.B, Tpe, Fpe, *d_pos)
        else:
            ops.patch_bwd_rows(dx, slot, lay.cu_tok, p["toff"], Tpe, Fpe, *d_pos)
    wg.launch_async(dx_lp, p["cols"], g["patch_embed.proj.weight"], None, done=-1)
    if not want_dx:
        return None
    P, (fs, ts) = model.patch_embed.patch_size[0], model.patch_embed.stride
    dcols = torch.empty((lay.M, P * P), device=dx_lp.device, dtype=dx_lp.dtype)
    ops.gemm_nt(dx_lp, st.get(model.patch_embed.proj.weight, dt, True), dt, EPI_STORE, out_lp=dcols)
    if slot is not None:
        return ops.patch_input_bwd_rows(dcols, slot, p["F"], p["T"], P, fs, ts)
    return ops.patch_input_bwd_varlen(dcols, lay.cu_tok, lay.B, p["F"], p["T"], P, fs, ts)


def _backward(model, ctx, dlogits, dfeat, grads, on_block_done, want_dx, patch_stage):
    with ops.gemm_flags(getattr(model, "_gemm_flags", 0)):
        wg = _WgradSchedule(model, ctx["dt"], grads, on_block_done, dlogits.device, ctx.get("plan"))
        if want_dx and wg.stop >= 0:
            raise ValueError("passt_backward(want_dx=True): this forward's plan ends the backward at stage "
                             f"{wg.stop} (make the plan with want_dx=True)")
        dx, dx_lp = _backward_trunk(model, ctx, dlogits, dfeat, wg)
        dx_in = None
        if wg.stop < 0:
            wg.enter(-1)
            dx_in = patch_stage(model, ctx, wg, dx, dx_lp, want_dx)
        wg.side.join()
    return dx_in


def passt_backward(model, ctx, dlogits, dfeat, grads, on_block_done=None, want_dx=False):
    """Backward of passt_forward.  ``grads``: dict param-name -> f32 tensor to OVERWRITE -- of a forward run with ``save=`` a
    trainable_plan: the plan's wanted parameters only; the backward then ends behind the plan's lowest stage, a stage without a
    trainable parameter runs its activation gradients only, and ``on_block_done`` fires for the stages that have one.
    ``on_block_done(i)`` is called after block i's parameter gradients are enqueued (i = depth for the
    head, then depth-1 .. 0, then -1 for the patch embedding) -- the hook the data-parallel reducer
    uses to start all-reducing finished buckets while the rest of the backward runs.

    ``want_dx``: also return the gradient w.r.t. the input spectrogram, (B, 1, F, T) f32 -- one more N = P*P GEMM with the
    transposed patch-embedding weight and the fold of the kept patches (pa_patch_input_bwd); otherwise returns None.
    ``grads=None``: the no-weight-gradients mode of a fully frozen network (a loss network): no weight-gradient GEMM, no bias /
    positional / head parameter reduction and no ``on_block_done``.  What the activation-gradient kernels produce anyway stays
    where it falls and is never reduced: the LayerNorm backward's dgamma / dbeta partial rows (in that call's own workspace) and
    the head's per-clip LayerNorm partials (pa_head_pre_bwd's ``part``).
    Gradients of the token outputs of a forward run with ``hidden=`` travel in the context: ``ctx["dhidden"] = {block index (>= 0)
    or "norm": (B * Ntok, D) f32}`` before this call (see _backward_trunk)."""
    return _backward(model, ctx, dlogits, dfeat, grads, on_block_done, want_dx, _patch_backward)


def passt_backward_varlen(model, ctx, dlogits, dfeat, grads, on_block_done=None, want_dx=False):
    """Backward of passt_forward_varlen(save=True): passt_backward's contract (``grads`` dict to OVERWRITE or None = the
    no-weight-gradients mode of a frozen network, ``on_block_done``, ``want_dx`` -> (B, 1, F, T_max) f32 or None) on the packed rows.
    Everything runs on M = sum of the clips' tokens: the same head / block sequence and weight-gradient scheduling as the fixed path
    (_backward_trunk, _WgradSchedule), the packed attention backward (pa_attention_bwd_varlen: always the kernel pair) and the packed
    patch stage (pa_patch_bwd_varlen, pa_patch_input_bwd_varlen).  A parameter gradient is the sum over the clips of their batch-1
    gradients; dx of clip i is what the clip alone gives in its own frames and exactly 0 behind them."""
    return _backward(model, ctx, dlogits, dfeat, grads, on_block_done, want_dx, _patch_backward_varlen)


_NLEAD = 7          # arguments of _PasstFunction.forward in front of x (none of them carries a gradient)


class _PasstFunction(torch.autograd.Function):
    """One autograd node for the whole network: forward/backward are kernel sequences, torch only sees
    (x, *parameters) -> (logits, features).  ``lengths``: None = the fixed path, else the packed ragged-batch forward
    (``net.varlen_grad = True``) with the packed backward; same ``grads`` / ``on_block_done`` contract, same flat-buffer and reducer
    routes.  ``hidden`` (parse_hidden's tuple or None): the token outputs asked for are further outputs of this node, behind
    (logits, features) and in the order asked (then, on the packed path, the int64 row offsets, which carry no gradient).
    ``attn`` (parse_attn's triple or None): the attention maps asked for follow the token outputs as outputs marked
    non-differentiable (on the packed path one flat buffer per map); the backward ignores their (None) gradients."""

    @staticmethod
    def forward(ctx, model, lengths, hidden, attn, rollout, drop_path_masks, attn_drop_seed, x, *params):
        req = attn if isinstance(attn, _AttnGradRequest) else None        # the maps' gradients were asked for as well
        named, total = model._graph_params(validate=False)            # the list forward() just handed to apply()
        flat = model._flat if (len(params) == 1 and model._flat is not None and params[0] is model._flat["token"]) else None
        # what the backward will have to reach is known now: the parameters and the input that ask for a gradient, and the lowest
        # block whose map gradient or rollout step rides with it.  The forward keeps nothing below that
        low = [min(req.triple[0])] if req is not None else []
        if isinstance(rollout, _RolloutRequest):
            low.append(rollout.first)
        # (under ddp.attach on several ranks the reducer's buckets are laid out over every parameter: all of them are produced)
        red = getattr(model, "_ddp", None)
        every = flat is not None or (red is not None and red.world > 1)
        plan = trainable_plan(model, bool(ctx.needs_input_grad[_NLEAD]), min(low) if low else None, named,
                              (True,) * len(named) if every else tuple(ctx.needs_input_grad[_NLEAD + 1:]))
        r = _run_forward(model, x, lengths, plan, hidden=hidden, attn=attn if req is None else req.triple, rollout=rollout,
                         drop_path_masks=drop_path_masks, **({} if attn_drop_seed is None else dict(attn_drop_seed=attn_drop_seed)))
        # the integer row offsets of the packed path are non-differentiable as they are
        ctx.mark_non_differentiable(*r.maps, *(() if r.roll is None else (r.roll,)))
        ctx.rollout = rollout if isinstance(rollout, _RolloutRequest) else None   # "cam": the backward runs the chain
        ctx.model, ctx.c, ctx.varlen, ctx.hidden = model, r.ctx, lengths is not None, hidden
        ctx.attn_grad = req
        # the input spectrogram's gradient is computed only when asked for; a graph none of whose parameters requires a gradient
        # (a frozen loss network) runs the backward without any weight-gradient work
        ctx.want_dx = bool(ctx.needs_input_grad[_NLEAD])
        ctx.frozen = not any(ctx.needs_input_grad[_NLEAD + 1:])
        ctx.named, ctx.total, ctx.plan = named, total, plan
        # bound to a passt_amd.optim.AdamW (PaSST.bind_flat_grads): the only input is a token; the backward writes the gradients
        # straight into the optimizer's persistent flat buffer -- p.grad are views of it -- and hands autograd nothing
        ctx.flat = flat
        ctx.set_materialize_grads(False)        # an unused `features` output arrives as None, not as a zero tensor
        return r.flat()

    @staticmethod
    def backward(ctx, dlogits, dfeat, *dhs):
        model, c = ctx.model, ctx.c
        if c is None:
            raise RuntimeError("passt_amd.PaSST: the saved activations of this forward were already consumed by a backward "
                               "pass (retain_graph / double backward are not supported: run the forward again)")
        run_backward = passt_backward_varlen if ctx.varlen else passt_backward
        # the model, the lengths, the hidden request, the attention-map request, the rollout request, the drop-path masks, the
        # attention-dropout seed
        lead = (None,) * _NLEAD
        dev = c["feat"].device
        # gradients of the token outputs that fed the loss, as [M][D] rows (an unused one arrives as None and costs nothing)
        dhidden = {k: d.contiguous().view(c["lay"].M, -1) for k, d in zip(ctx.hidden or (), dhs) if d is not None}
        if dhidden:
            c["dhidden"] = dhidden
        ag, ctx.attn_grad = ctx.attn_grad, None
        if ag is not None and ag.targets is not None:
            c["attn_grad"] = ag
        rr, ctx.rollout = ctx.rollout, None
        if rr is not None and rr.target is not None:
            red = getattr(model, "_ddp", None)
            rr.g_scale = float(red.world) if (red is not None and red.world > 1 and not ctx.frozen) else 1.0
            c["rollout"] = rr
        # gradient buffers for the parameters that asked for one (ctx.plan; head_dist.* is never among them): a frozen
        # parameter has no buffer and its gradient is not computed where that is a launch of its own (frozen backbone, ...)
        named, plan = ctx.named, ctx.plan
        fl = ctx.flat
        B = c["lay"].B
        if dlogits is not None:
            dlogits = dlogits.contiguous()
        if ctx.frozen:
            # nothing but the input asked for a gradient: no flat buffer, no weight-gradient launch, no reducer (dx is a local quantity)
            if dlogits is None:
                dlogits = torch.zeros((B, model.num_classes), device=dev, dtype=torch.float32)
            dx = run_backward(model, c, dlogits, None if dfeat is None else dfeat.contiguous(), None, want_dx=ctx.want_dx)
            ctx.c = None
            _fill_rollout_grad(rr)
            return lead + (dx,) + (None,) * (len(named) if fl is None else 1)
        if fl is not None and fl["fresh"]:
            flat, grads = fl["flat_g"], fl["grads"]     # overwritten in place: the caller zeroed (optimizer.zero_grad()) since the last backward
        else:
            flat = torch.empty(plan.total, device=dev, dtype=torch.float32)
            # one C++ call makes the 159 views (a Python loop of slice + view costs 1.3 ms of host time in front of the first
            # backward kernel: exposed whenever the caller synchronised in this step, and the reference's mixup does)
            wanted = [named[i] for i in plan.idx]
            views = torch._C._nn.unflatten_dense_tensors(flat, [p for _, p in wanted])
            grads = {n: v for (n, _), v in zip(wanted, views)}
        # a fresh flat buffer per backward: autograd may keep (not copy) the views as .grad
        if dlogits is None:                     # only `features` fed the loss
            dlogits = torch.zeros((B, model.num_classes), device=flat.device, dtype=torch.float32)
        dlogits = dlogits.contiguous()
        dfeat = None if dfeat is None else dfeat.contiguous()
        red = getattr(model, "_ddp", None)
        if red is not None and red.world > 1:
            # passt_amd.ddp.attach(net): this node reduces its own gradients.  `flat` is laid out like the reducer's buckets
            # (named_parameters() order without head_dist.*); every bucket's all-reduce starts from on_block_done while the
            # rest of the backward runs, and the node returns once the current stream is ordered behind the last bucket.
            # Mean over ranks (DDP's semantics) = sum of gradients of loss / world: the backward is linear in (dlogits, dfeat).
            if flat.numel() != red.total:
                raise RuntimeError("passt_amd.ddp.attach: the parameter set changed since attach(); call attach(net) again")
            inv = 1.0 / red.world
            dlogits = dlogits * inv
            dfeat = None if dfeat is None else dfeat * inv
            for k in dhidden:
                dhidden[k] = dhidden[k] * inv
            red.flat = flat
            try:
                dx = run_backward(model, c, dlogits, dfeat, grads, on_block_done=red.on_block_done, want_dx=ctx.want_dx)
            finally:
                red.wait()              # also after an exception: no collective may stay in flight on a buffer we drop
            if dx is not None:
                dx.mul_(float(red.world))       # not reduced: the gradient of THIS rank's loss (dlogits went in divided by world)
            if ag is not None:
                # so are the maps' gradients: d_att came down divided by world, "grad" is linear in it and relu(map * gradient)
                # commutes with a positive factor.  One more f32 rounding than a single rank's unless world is a power of two.
                for t in ag.targets:
                    for u in (t if isinstance(t, list) else [t]):
                        u.grad.mul_(float(red.world))
        else:
            dx = run_backward(model, c, dlogits, dfeat, grads, want_dx=ctx.want_dx)
        ctx.c = None
        _fill_rollout_grad(rr)
        if fl is not None:
            if not fl["fresh"]:                 # a second backward without zero_grad (gradient accumulation): add, as AccumulateGrad would
                fl["flat_g"].add_(flat)
            fl["fresh"] = False
            return lead + (dx, None)
        out = list(lead) + [dx] + [None] * len(named)      # the same list, in the same order, as PaSST.forward handed to apply()
        for i in plan.idx:
            if ctx.needs_input_grad[_NLEAD + 1 + i]:
                out[_NLEAD + 1 + i] = grads[named[i][0]]
        return tuple(out)


def _fill_rollout_grad(rr):
    """.grad of what a ``rollout="cam"`` forward returned: the rows the backward's chain ended on (packed: every clip's view gets its
    own view of the one buffer)."""
    if rr is None or rr.target is None or rr.result is None:
        return
    if isinstance(rr.target, list):
        for t, v in zip(rr.target, ops.rollout_views(rr.result, [t.shape[-1] for t in rr.target])):
            t.grad = v
    else:
        rr.target.grad = rr.result
    rr.result = rr.start = None


def _tree_signature(root):
    """[(module, ids of its parameters, ids of its sub-modules)] over the module tree: what PaSST._graph_params() validates its
    cached parameter list against on every forward (~110 modules, two small tuples each: ~30 us).  Local to this model: surgery
    anywhere in ITS tree (net.head[1] = nn.Linear(768, 50), a block's sub-module replaced, a parameter re-registered) changes
    a tuple; nothing is hooked process-wide."""
    return [(m, tuple(map(id, m._parameters.values())), tuple(map(id, m._modules.values()))) for m in root.modules()]


_LIVE = weakref.WeakSet()            # live PaSST instances: how passt_amd.optim.AdamW finds the model its parameters belong to
_RUNTIME_ATTRS = ("_staged", "_scratch", "_ddp", "_gemm_flags", "_flat", "_last_dt")


def _after_fused_step(opt, args, kwargs):
    """torch's fused optimizers (``fused=True``: torch._fused_adamw_ and its kin) rewrite the parameters in place WITHOUT bumping
    ``_version`` (tests/test_module_state_cpu.py pins it), so the staged weight copies cannot see their step: every live model
    that has a copy of one of the optimizer's parameters gets the epoch bump ``mark_params_updated`` gives.  Every other torch
    optimizer bumps the versions itself and costs one dict lookup per group here."""
    if not any(g.get("fused") for g in opt.param_groups):
        return
    ids = None
    for net in list(_LIVE):
        cache = net._staged.cache
        if not cache:
            continue
        if ids is None:
            ids = {id(p) for g in opt.param_groups for p in g["params"]}
        if any(key[0] in ids for key in cache):
            net.mark_params_updated()


register_optimizer_step_post_hook(_after_fused_step)


class PaSST(nn.Module):
    """Same constructor as the reference (models/passt.py:391-395)."""

    def __init__(self, u_patchout=0, s_patchout_t=0, s_patchout_f=0, img_size=(128, 998), patch_size=16, stride=16,
                 in_chans=1, num_classes=527, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., qkv_bias=True,
                 representation_size=None, distilled=False, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.,
                 embed_layer=PatchEmbed, norm_layer=None, act_layer=None, weight_init=''):
        super().__init__()
        if not distilled:
            raise NotImplementedError("passt_amd covers the distilled (cls+dist token) PaSST archs -- every "
                                      "arch get_model() can return (models/passt.py:963-1008)")
        if in_chans != 1 or drop_rate or attn_drop_rate or mlp_ratio != 4. or not qkv_bias or representation_size:
            raise NotImplementedError("passt_amd hot path: in_chans=1, no dropout (drop_rate / attn_drop_rate; stochastic depth, "
                                      "drop_path_rate, is covered; attention dropout is set on the modules, as with the reference's "
                                      "get_model(): net.blocks[i].attn.attn_drop.p = p), mlp_ratio=4, qkv_bias")
        if embed_dim % num_heads or embed_dim // num_heads != 64:
            raise NotImplementedError("attention kernels are built for head_dim 64 (768/12, 1024/16, 384/6 ...)")
        self.num_classes = num_classes
        self.u_patchout, self.s_patchout_t, self.s_patchout_f = u_patchout, s_patchout_t, s_patchout_f
        self.num_features = self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.num_tokens = 2
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-6)
        act_layer = act_layer or nn.GELU
        self.patch_embed = embed_layer(img_size=img_size, patch_size=patch_size, stride=stride, in_chans=in_chans,
                                       embed_dim=embed_dim, flatten=False)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.dist_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.new_pos_embed = nn.Parameter(torch.zeros(1, self.num_tokens, embed_dim))
        self.freq_new_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, self.patch_embed.grid_size[0], 1))
        self.time_new_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, 1, self.patch_embed.grid_size[1]))
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, depth)]      # stochastic depth decay rule (:444)
        self.blocks = nn.Sequential(*[
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop_path=dpr[i], norm_layer=norm_layer,
                  act_layer=act_layer) for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.pre_logits = nn.Identity()
        self.head = nn.Sequential(nn.LayerNorm(self.num_features),
                                  nn.Linear(self.num_features, num_classes) if num_classes > 0 else nn.Identity())
        self.head_dist = nn.Linear(self.embed_dim, self.num_classes) if num_classes > 0 else nn.Identity()
        self.precision = None          # None: follow torch.autocast; or "fp32" / "bf16"
        # opt-in: run weight/bias-gradient kernels on a second stream (+2.4 % step throughput measured on MI355X);
        # off by default so that every kernel runs alone and per-kernel timings (bench.py roofline, rocprof) are exact
        self.overlap_wgrad = False
        # opt-in: with TRAINABLE parameters, also hand back the gradient w.r.t. an input spectrogram that requires one (off: such a
        # call raises NotImplementedError, as it always did).  A fully frozen network needs no switch: there the input is the only
        # thing that can ask for a gradient
        self.input_grad = False
        # opt-in: forward(x, lengths=...) in eval mode becomes an autograd node (packed backward) -- x.grad for an input that requires
        # one, gradients for the parameters that require one, together if both do (input_grad is not looked at on that path).  Off:
        # the ragged forward records nothing, as it always did
        self.varlen_grad = False
        # opt-in: forward(x, lengths=...) in TRAINING mode -- Patchout per clip, drawn clip after clip as at batch size 1 -- as an autograd
        # node under the fixed path's rule (grad enabled and anything requires a gradient; varlen_grad / input_grad are not looked at).
        # Off: such a call raises NotImplementedError, as it always did
        self.varlen_train = False
        # ragged batches in training mode with stochastic depth / attention dropout active: refused unless asked for (forward's docstring)
        self.varlen_regularize = False
        self.init_weights(weight_init)
        self._reset_runtime()

    # ---- runtime state that must not be deep-copied / pickled (SWA deepcopies the net) ----------
    def _reset_runtime(self):
        object.__setattr__(self, "_staged", _Staged())
        object.__setattr__(self, "_scratch", {})
        object.__setattr__(self, "_ddp", None)          # passt_amd.ddp.attach(): gradient reducer of the autograd path
        object.__setattr__(self, "_gemm_flags", 0)      # pa_gemm_args.reserved bits of this model's GEMM launches
        object.__setattr__(self, "_flat", None)         # bind_flat_grads(): flat gradient buffer owned by a passt_amd.optim.AdamW
        object.__setattr__(self, "_last_dt", None)
        _LIVE.add(self)

    def __deepcopy__(self, memo):
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k in _RUNTIME_ATTRS:
                continue
            new.__dict__[k] = copy.deepcopy(v, memo)
        new._reset_runtime()
        return new

    def __getstate__(self):
        d = self.__dict__.copy()
        for k in _RUNTIME_ATTRS:
            d.pop(k, None)
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self._reset_runtime()

    def _graph_params(self, validate=True):
        """([(name, parameter)] without head_dist.*, total numel): what the autograd node takes and returns gradients for, in
        named_parameters() order.  Cached (named_parameters() over the tree costs 0.4 ms per call); the cache is validated per
        forward against the identity of every module's parameters and children (``_tree_signature``: the cached list keeps the
        old objects alive, so an id cannot be reused), and dropped when the module is moved / cast (``_apply``).  The backward
        of a forward passes validate=False: it must hand back gradients for exactly the list that forward gave to apply()."""
        hit = self._scratch.get("graph_params")
        if hit is not None and validate:
            for m, pids, mids in hit[2]:
                if tuple(map(id, m._parameters.values())) != pids or tuple(map(id, m._modules.values())) != mids:
                    hit = None
                    break
        if hit is None:
            named = [(n, p) for n, p in self.named_parameters() if not n.startswith("head_dist.")]
            hit = self._scratch["graph_params"] = (named, sum(p.numel() for _, p in named), _tree_signature(self))
        return hit[:2]

    def __setattr__(self, name, value):
        if isinstance(value, (nn.Module, nn.Parameter)) and "_scratch" in self.__dict__:
            self._scratch.pop("graph_params", None)
        super().__setattr__(name, value)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        if "_scratch" in self.__dict__:
            self._scratch.pop("graph_params", None)
            self.unbind_flat_grads()            # .to() / .cuda() / .float() replaced the storages the flat views pointed into
        return out

    # ---- one flat gradient for the drop-in path (FSDP use_orig_params-style) -------------------------------------
    def bind_flat_grads(self, flat_g):
        """Called by passt_amd.optim.AdamW once it owns this model's parameters as ONE flat buffer: ``flat_g`` (f32, numel = all
        parameters the network produces gradients for, named_parameters() order without head_dist.*) becomes the model's
        persistent gradient buffer.  From then on forward() hands autograd a single token instead of 159 parameters, the backward
        writes every gradient straight into ``flat_g`` and ``p.grad`` of every parameter is a standing view of it: no
        AccumulateGrad nodes, no per-parameter host work in backward / zero_grad / step -- what made the drop-in path host-bound at
        ESC-50's batch of 12 (ex_esc50.py:40).  ``state_dict`` keys, ``parameters()`` order and the parameters themselves are
        untouched.  Gradient semantics: after ``optimizer.zero_grad()`` (the bound optimizer marks the buffer fresh) a backward
        overwrites; a further backward without zero_grad adds, like autograd.  Not for a torch DistributedDataParallel wrapper (its
        reducer hooks AccumulateGrad; use passt_amd.ddp.attach, which reduces this buffer per block)."""
        named, total = self._graph_params()
        if any(not p.requires_grad for _, p in named):
            return None                                  # frozen parameters: autograd decides which gradients exist; stay unbound
        assert flat_g.numel() == total and flat_g.dtype == torch.float32
        views = torch._C._nn.unflatten_dense_tensors(flat_g, [p for _, p in named])
        # gradients that already exist (the optimizer binds inside its first step(): the first backward has run) move in
        have = [p.grad is not None for _, p in named]
        if all(have):
            torch._foreach_copy_(list(views), [p.grad for _, p in named])
        elif any(have):
            return None                                  # a partial set: leave this step to the per-parameter path
        for (n, p), v in zip(named, views):
            p.grad = v
        fl = dict(token=torch.zeros((), device=flat_g.device, requires_grad=True), flat_g=flat_g, grads={n: v for (n, _), v in zip(named, views)},
                  named=named, fresh=not all(have))
        object.__setattr__(self, "_flat", fl)
        return fl

    def unbind_flat_grads(self, keep_grads=False):
        """keep_grads: the gradients of the last backward stay in ``p.grad`` (still views of the old buffer) for the step that is
        about to consume them; parameters that were frozen meanwhile lose theirs."""
        fl = self.__dict__.get("_flat")
        if fl is not None:
            object.__setattr__(self, "_flat", None)
            for _, p in fl["named"]:
                if not (keep_grads and p.requires_grad and not fl["fresh"]):
                    p.grad = None

    @property
    def _grad_names(self):
        return {n for n, p in self.named_parameters() if p.requires_grad and not n.startswith("head_dist.")}

    @property
    def _n_grad_elems(self):
        names = self._grad_names
        return sum(p.numel() for n, p in self.named_parameters() if n in names)

    def init_weights(self, mode=''):
        """models/passt.py:471-484."""
        assert mode in ('jax', 'jax_nlhb', 'nlhb', '')
        nn.init.trunc_normal_(self.new_pos_embed, std=.02)
        nn.init.trunc_normal_(self.freq_new_pos_embed, std=.02)
        nn.init.trunc_normal_(self.time_new_pos_embed, std=.02)
        nn.init.trunc_normal_(self.dist_token, std=.02)
        if mode.startswith('jax'):
            raise RuntimeError("Not supported yet")
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.apply(_init_vit_weights)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'new_pos_embed', 'freq_new_pos_embed', 'time_new_pos_embed', 'cls_token', 'dist_token'}

    def get_classifier(self):
        return self.head, self.head_dist

    def reset_classifier(self, num_classes, global_pool=''):
        raise NotImplementedError("reset_classifier drops the head LayerNorm in the reference "
                                  "(models/passt.py:500-504); build a new model with n_classes instead")

    def forward_features(self, x):
        raise NotImplementedError("only forward() is on the accelerated path (returns (logits, features)); the token sequence the "
                                  "reference's forward_features holds before it pools is forward(x, hidden=(\"norm\",))")

    def mark_params_updated(self):
        """Every staged weight copy (the bf16 casts, the transposes the backward reads) is stale: the next forward re-makes them.
        A copy is current while its parameter's ``(_version, data_ptr())`` and this model's epoch are unchanged, so whatever bumps
        the version counter or moves the storage is seen without this call: torch optimizers (the ``fused=True`` ones through a
        step hook), ``load_state_dict``, in-place operations on the parameter under ``torch.no_grad()`` or on ``p.detach()``,
        ``nn.init.*``, ``p.data = tensor``, a replaced sub-module.  Call it after a write that does neither: an in-place operation on
        ``p.data`` (``p.data.mul_()``, ``p.data.copy_()``), a write through ``TrainStep.flat_p`` or the flat buffer of a
        ``passt_amd.optim.AdamW`` (restoring a checkpoint of either), a kernel given the raw device pointer (passt_amd.optim
        calls it itself)."""
        self._staged.epoch += 1

    @compile_opaque
    def forward(self, x, lengths=None, hidden=None, attn=None, attn_rows="all", attn_heads="each", attn_grad=None, rollout=None,
                rollout_from=0, drop_path_masks=None, attn_drop_seed=None):
        """x: (B,1,F,T) -> (logits (B,C), features (B,D)); always a tuple (models/passt.py:588,595).  With the keywords below:
        ``(logits, features[, hidden][, attn][, roll][, tok_offsets])``, tok_offsets whenever ``lengths`` comes with ``hidden``, ``attn``
        or ``rollout``.

        ``hidden`` (a list / tuple of block indices, negative allowed, and / or the string "norm"): also return the token sequence
        at those depths, ``(logits, features, hidden)`` -- with ``lengths``: ``(logits, features, hidden, tok_offsets)`` -- where
        ``hidden`` is a list in the order asked.  Entry ``i`` is the output of ``blocks[i]`` (what a forward hook on the reference's
        ``blocks[i]`` sees), f32 (B, Ntok, D): rows 0 / 1 are cls / dist, the others the kept patches in the reference's order --
        frequency-major in eval mode, so ``h[:, 2:].view(B, F', T', D)`` is the (frequency, time) grid; in training mode the
        patches Patchout kept (the draws are those of a call without ``hidden``).  "norm" is ``net.norm`` applied to every row of the
        last block's output: what the reference's ``forward_features`` holds before it pools; its rows 0 / 1 are the tokens whose mean
        is ``features``.  With ``lengths`` every entry is the packed (M, D) matrix and ``tok_offsets`` an int64 CPU tensor of B + 1
        row offsets (the convention of ``frames`` from ``mel(..., lengths=)``): clip i owns rows tok_offsets[i] : tok_offsets[i + 1],
        which are what the clip gets alone at batch size 1.  The entries are outputs of the same autograd node under the same rules
        as (logits, features): a loss on them reaches ``x.grad`` and the parameter gradients; one that does not feed the loss costs
        nothing.  They are the network's own buffers handed out (no copy): do not write into them before the backward.  Blocks
        below the last one cost nothing to ask for; the last block or "norm" makes the last block run on all rows instead of the
        two prefix rows (about one more block of forward and backward), and logits / features then agree with a call without
        ``hidden`` to rounding, not bit for bit (the all-queries attention kernel orders its sums differently).  A bare int, an
        empty sequence, an index out of range or an entry named twice raises ValueError before anything is launched or drawn.

        ``attn`` (a list / tuple / range of block indices, negative allowed): also return the attention probabilities
        softmax(q k^T * scale) of those blocks -- what a forward hook on the reference's ``blocks[i].attn.attn_drop`` sees as its
        input -- as a list in the order asked, f32, computed by a kernel of their own right behind the block's fused attention from
        the same qkv and row statistics.  An entry is (B, H, Nq, Ntok), or (B, Nq, Ntok) with ``attn_heads="mean"`` (the mean over
        heads, taken in f32 in head order); ``attn_rows="all"`` gives every query row (Nq = Ntok), ``"prefix"`` the cls and dist
        query rows only (Nq = 2: the usual saliency rows, and cheap).  Rows and columns are in the token order of ``hidden``: cls,
        dist, then the kept patches.  With ``lengths`` an entry is a list of B tensors, views of one device buffer: clip i's
        (H, Nq_i, N_i) or (Nq_i, N_i), what the clip gets alone at batch size 1.  The maps carry no gradient (no grad_fn; they are
        non-differentiable outputs of the autograd node) and change nothing else: same Patchout draws, and logits, features and
        every gradient are bit for bit those of a call without ``attn`` -- except that ``attn_rows="all"`` on the last block makes
        the last block run on all rows instead of the two prefix rows (about one more block of forward and backward), and logits /
        features then agree with a call without ``attn`` to rounding, not bit for bit (the all-queries attention kernel orders its
        sums differently); the last block's ``"prefix"`` rows come from the prefix-only tail as it is.  A map costs its own bytes:
        B * H * Nq * Ntok * 4.  A bare int, an empty sequence, an index out of range or named twice, or another value of
        ``attn_rows`` / ``attn_heads`` raises ValueError before anything is launched or drawn.

        ``attn_grad`` ("grad", "cam"; True means "grad"; needs ``attn``): the call returns exactly what it returns without it, and the
        BACKWARD of this forward also fills ``.grad`` of every returned map tensor (None before it), same shape, f32.  "grad": the
        gradient of the loss with respect to the block's attention probabilities -- what ``retain_grad()`` on the tensor a forward hook
        on the reference's ``blocks[i].attn.attn_drop`` sees holds after ``loss.backward()``; it needs ``attn_heads="each"``, and
        ``attn_rows="prefix"`` gives its cls / dist query rows.  "cam": relu(map * gradient), with ``attn_heads="mean"`` the mean over
        heads of that, (B, Nq, Ntok): the factor of gradient-weighted attention rollout.  One launch per requested block right behind the
        block's fused attention backward, from the qkv, row statistics and output gradient that one read; a gradient costs what its
        map costs.  With ``lengths`` clip i's tensor gets a view of one flat buffer, what the clip gets alone at batch size 1.  Logits,
        features, ``x.grad`` and every parameter gradient are bit for bit those of the call with ``attn`` alone.  The call must
        record a graph: under ``torch.no_grad()``, or when nothing requires a gradient (with ``lengths``: without ``varlen_grad`` /
        ``varlen_train``), it raises ValueError -- as do an unknown value, ``attn_grad`` without ``attn`` and "grad" with
        ``attn_heads="mean"`` -- before anything is launched or drawn.  Not taken by TrainStep or captured graphs.

        ``rollout`` ("attn", "cam") with ``rollout_from`` (a block index k, negative allowed; default 0): also return ``roll``, the cls
        and dist ROWS of an attention rollout through blocks k .. depth-1, f32 (B, 2, Ntok) -- row 0 the cls row, row 1 the dist row,
        columns in ``hidden``'s token order -- without forming a single attention map: a row of a product of matrices is a chain of
        row-vector x matrix products, and every product is taken tile by tile in registers (pa_attention_rollout), one launch per
        block.  With ``lengths``: a list of B views (2, N_i) of one buffer, and ``tok_offsets`` is returned.  "attn": the rows of
        prod_{l = depth-1 .. k} (0.5 mean_h A_l + 0.5 I), later blocks on the left (attention rollout, Abnar & Zuidema; its rows
        already sum to 1); computed behind the last block, in eval and train mode (kept patches), with or without a graph; no grad_fn.
        "cam": the forward launches nothing more and ``roll`` holds the one-hot start rows; the BACKWARD of this forward fills
        ``roll.grad`` (ragged: every view's) with the rows of prod_{l = depth-1 .. k} (I + mean_h relu(A_l * dA_l)) (gradient-weighted
        rollout, Chefer et al.), one launch right behind every block's attention backward.  "cam" must record a graph under
        ``attn_grad``'s rules and raises its ValueErrors; under ``passt_amd.ddp.attach`` the rows are this rank's own.  Independent
        of ``attn`` / ``attn_grad``; everything else the call returns or accumulates is bit for bit what it is without ``rollout``.
        Any other value, a ``rollout_from`` that is no int or out of range, or one without ``rollout`` raises ValueError before
        anything is launched or drawn.  Not taken by TrainStep or captured graphs.

        Stochastic depth (``drop_path_rate > 0`` at construction): in training mode every clip keeps or drops each branch of each
        block with an active ``DropPath`` -- kept: scaled by 1 / (1 - p), dropped: contributes nothing, forward and backward, that
        branch's weight and bias gradients included.  The draws are the reference's: per active module call one
        ``torch.rand((B, 1, 1), dtype=torch.float32, device=x.device)``, blocks ascending, attention branch then MLP branch, behind
        the Patchout draws (``drop_path_draws``); under autocast the reference would draw in the 16-bit type, this path always
        draws f32.  ``drop_path_masks`` (a (depth, 2, B) tensor of keep flags, 1 keep / 0 drop, [i, 0] the attention branch of block
        i, [i, 1] its MLP branch): used in place of the draws -- nothing is drawn; entries of blocks without an active ``DropPath``
        are ignored -- which is how a recorded run is replayed.  Ignored in eval mode, where, as at rate 0, the network launches
        exactly what it launches without stochastic depth.  With ``lengths`` in training mode an active ``DropPath`` raises
        NotImplementedError.

        Attention dropout (the reference's ``nn.Dropout`` on the attention probabilities, set the reference's way:
        ``for b in net.blocks: b.attn.attn_drop.p = 0.1``; the constructor still refuses ``attn_drop_rate``): in training mode a block
        with ``attn_drop.p > 0`` runs the fused attention with dropout, forward and backward (``pa_attention_fwd_dropout`` /
        ``_bwd_dropout``).  The rate is quantised to t = round(256 p) / 256 (``attn_drop_rates``; a p that rounds past 255 / 256 raises
        ValueError) and kept probabilities are scaled by 1 / (1 - t / 256): exact in expectation for the rate applied.  The mask is
        not the reference's (element-wise masks cannot be drawn reference-equal on the device) but a pure function of a 64-bit seed
        and (block, clip x head, query, key): ``passt_amd.attn_drop_mask(seed, block, B, H, Nq, Ntok, p)`` restates it on the CPU.  A
        training forward with at least one active block draws the seed once, ``torch.randint(-2**31, 2**31, (2,), dtype=torch.int32,
        device=x.device)``, behind the Patchout and the drop-path draws; eval mode and all-zero rates draw nothing and launch exactly
        what they launch without dropout.  ``attn_drop_seed`` (two ints < 2^32, or a (2,) tensor): used in place of the draw -- same
        seed, same inputs: bit-identical outputs and gradients; ignored in eval mode.  ``attn=`` maps and ``rollout="attn"`` stay the
        undropped softmax (the INPUT of ``attn_drop``).  NotImplementedError, before any draw: ``lengths`` in training mode with an
        active attention dropout (unless ``net.varlen_regularize = True``, below); ``attn_grad`` or ``rollout="cam"`` when a block they touch is active.  ``drop_rate`` (the other
        element-wise dropout sites) is not covered: the constructor raises.

        An ``x`` that requires a gradient gets one (``x.grad`` / ``torch.autograd.grad``), as in the reference: PaSST as a
        differentiable loss network.  With every parameter frozen (``net.requires_grad_(False)``) this needs no switch and the backward
        runs no weight-gradient kernel at all; with trainable parameters it is opt-in (``net.input_grad = True``, otherwise
        NotImplementedError as before) and everything is computed as in training, plus the input gradient.

        ``lengths`` (a sequence of ints or a 1-D integer tensor, one entry per clip): a batch of clips of DIFFERENT lengths, left-aligned
        in ``x`` (B, 1, n_mels, T_max); clip i is valid in its first lengths[i] frames and whatever lies behind them has no influence
        (it is never read).  Row i of both outputs is what ``forward(x[i:i+1, :, :, :lengths[i]])`` returns at batch size 1 -- the
        reference's own way of evaluating clips of different lengths (ex_fsd50k.py:53-56) -- but the batch runs as ONE packed kernel
        sequence over sum_i tokens.  Eval mode (training mode: ``varlen_train``, below).  The token geometry is decided on the host:
        ``lengths`` given as a device tensor costs one host read.  A clip shorter than one patch raises ValueError; clips whose patch
        columns reach the time embedding's length are cut to it, with one warning per call.
        Gradients through the ragged forward are opt-in: by default the outputs carry no grad_fn, also for an ``x`` that requires a
        gradient.  With ``net.varlen_grad = True`` (eval mode, grad enabled) the packed forward is an autograd node with a packed
        backward: an ``x`` that requires a gradient gets ``x.grad`` in its own shape / dtype / layout, every element written and
        exactly 0 at frames >= lengths[i] and behind the time cut; every parameter that requires a gradient gets one; a fully frozen
        network runs no weight-gradient kernel.  For a loss that is a sum over clips, ``x.grad[i, ..., :lengths[i]]`` is what clip i
        alone gives at batch size 1, and a parameter gradient is the sum over clips of those batch-1 gradients.  ``input_grad`` is not
        consulted here.
        Training mode with ``lengths`` raises NotImplementedError unless ``net.varlen_train = True``.  With it the contract above carries
        over to training: EVERY CLIP GETS WHAT IT WOULD GET ALONE AT BATCH SIZE 1 IN TRAINING MODE.  Patchout is drawn clip after clip,
        i = 0 .. B - 1, with the reference's own torch CPU RNG calls in the reference's order (randint for the time-positional offset
        of a clip with fewer patch columns than the time embedding, then randperm for s_patchout_t, s_patchout_f, u_patchout): after
        ``torch.manual_seed(s)`` one packed call leaves the CPU generator where the loop ``for i: net(x[i:i+1, :, :, :lengths[i]])``
        leaves it and gives clip i the same kept patches and offset, and the Patchout counts keep the reference's absolute meaning (not
        scaled to a clip's length).  A clip that cannot satisfy them -- no more patch columns than s_patchout_t, no more frequency rows
        than s_patchout_f, no more patches left than u_patchout, structured time Patchout on a clip with more patch columns than the
        time embedding (the reference itself fails there) -- raises a ValueError that names the clip, before any RNG call.  The call is
        an autograd node under the fixed path's rule -- grad enabled and anything requires a gradient; an ``x`` that requires one
        gets ``x.grad``, exactly 0 behind lengths[i] and on pixels that only dropped patches cover; ``varlen_grad`` and ``input_grad``
        are not consulted -- and a plain forward with Patchout under ``torch.no_grad()``.  ``hidden`` / ``attn`` hand out the kept
        tokens per clip, as above.  Not covered: ``AugmentMelSTFT(..., lengths=)`` in training mode (pad, run the train-mode mel, then
        ``net(spec, lengths=frames)``), EnsembelerModel.  The fused step takes ragged batches as ``TrainStep.step(x, y, lengths=)``,
        with its own definition of mixup between clips of different lengths (passt_amd.train).
        Stochastic depth and attention dropout on a ragged training batch are opt-in as well: by default (``net.varlen_regularize =
        False``) a model with either active raises NotImplementedError before any draw.  With ``net.varlen_regularize = True`` A RAGGED
        BATCH OF B CLIPS IS REGULARISED AS THE FIXED PATH REGULARISES A BATCH OF B CLIPS (not: each clip alone at batch size 1; Patchout
        keeps its clip-after-clip CPU draws).  Draw order: the per-clip Patchout draws on the CPU generator; then
        ``drop_path_draws(net, B, device)`` as it is -- one ``torch.rand((B, 1, 1))`` per active module call, blocks ascending,
        attention branch then MLP branch; then ``attn_drop_draw(device)``, one seed.  After ``torch.manual_seed(s)`` a ragged forward
        leaves the device generator where a fixed forward at the same B leaves it.  Clip b gets entry b of the (depth, 2, B) factors on
        all of its token rows, however many it has (2 rows on the prefix-only tail); ``drop_path_masks`` has the fixed path's shape and
        meaning.  The attention mask rule is unchanged: element (site = block, s = b*H + h, q, k) uses b, the clip's index in the
        batch, and q, k, the positions inside the clip.  The rule does not depend on the token count, so clip b gets bit for bit the
        mask the fixed path gives sequence b: ``passt_amd.attn_drop_mask(seed, block, b + 1, H, nq, N_b, p)[b]`` restates it on the
        CPU, and ``attn_drop_seed`` replays it.  A shape error in either keyword raises ValueError before any draw.  With every rate 0,
        and in eval mode, the switch changes nothing: the packed path launches what it launches without it.  Maps and
        ``rollout="attn"`` stay the undropped softmax; ``attn_grad`` / ``rollout="cam"`` through an active block keep their refusal.
        ``TrainStep.step(..., lengths=)`` reads the same switch on its net.

        ``torch.compile(net)`` (ex_audioset.py:135, model_speed_test :391): the whole forward is ONE opaque call to the
        compiler (``_lib.compile_opaque``: torch.compiler.disable's mechanism without the torch._dynamo import, installed at class
        definition so that every compile flow meets it) -- there is nothing for Inductor to fuse, every kernel of the network is already
        a hand-written launch behind the C ABI, and dynamo cannot trace ctypes calls; the compiled module therefore runs this
        function eagerly, captures no graph and never recompiles (tests/test_abi_cpu.py, tests/test_gpu_model.py speed-test
        flow).  Under ``torch.autocast`` of either 16-bit type (Lightning precision=16 / torch.cuda.amp.autocast() are fp16) the
        kernels run the bf16 MFMA path with f32 accumulation and return f32 logits / features: bf16 has f32's exponent range,
        so a GradScaler's loss scale flows through the backward without overflow and its inf checks never fire."""
        hid = None if hidden is None else parse_hidden(hidden, len(self.blocks))
        if attn is None:
            if attn_rows not in ("all", "prefix") or attn_heads not in ("each", "mean"):
                parse_attn((0,), 1, attn_rows, attn_heads)     # raises
            amap = None
        else:
            amap = parse_attn(attn, len(self.blocks), attn_rows, attn_heads)
        agrad = parse_attn_grad(attn_grad, attn, attn_heads)
        roll = parse_rollout(rollout, rollout_from, len(self.blocks))
        ad_t = attn_drop_rates(self)
        if any(ad_t):
            if agrad is not None and any(ad_t[i] for i in amap[0]):
                raise NotImplementedError("attn_grad on a block with an active attention dropout (attn_drop.p > 0 in training mode) is "
                                          "not supported: the gradient with respect to the undropped map needs the mask in "
                                          "pa_attention_probs_grad")
            if roll is not None and roll[0] == "cam" and any(ad_t[roll[1]:]):
                raise NotImplementedError("rollout=\"cam\" through a block with an active attention dropout (attn_drop.p > 0 in training "
                                          "mode) is not supported: its gradient factor needs the mask in pa_attention_probs_grad")
        train_ragged = lengths is not None and self.training
        if train_ragged and not getattr(self, "varlen_train", False):
            raise NotImplementedError("PaSST.forward(x, lengths=...): training on ragged batches is not supported (eval mode only; "
                                      "no reference flow trains on clips of different lengths) unless asked for: net.varlen_train = True "
                                      "gives every clip the Patchout it would get alone at batch size 1")
        grad = torch.is_grad_enabled()
        want_dx = grad and torch.is_tensor(x) and x.requires_grad
        named = None
        if lengths is None:
            if want_dx and not getattr(self, "input_grad", False) and any(p.requires_grad for _, p in self._graph_params()[0]):
                raise NotImplementedError("passt_amd.PaSST with trainable parameters produces a gradient w.r.t. its input spectrogram only "
                                          "when asked to: set net.input_grad = True (or freeze the network: net.requires_grad_(False); "
                                          "or detach() the input)")
            # head_dist.* is not part of the graph -- as in the reference, whose forward never touches it
            # (models/passt.py:583-595; hence find_unused_parameters=True under torch DDP there and here)
            node = grad and (want_dx or any(p.requires_grad for p in self.parameters()))
        elif grad and (train_ragged or getattr(self, "varlen_grad", False)):
            named = self._graph_params()[0]
            node = want_dx or any(p.requires_grad for _, p in named)
        else:
            node = False                                # the ragged forward records nothing unless asked to
        if agrad is not None:
            if not node:
                raise ValueError("attn_grad: the gradients of the maps come out of a backward, and this call records no graph (nothing "
                                 "requires a gradient, torch.no_grad() is active, or lengths= without net.varlen_grad / net.varlen_train)")
            req = _AttnGradRequest(amap, agrad)
        if roll is not None and roll[0] == "cam":
            if not node:
                raise ValueError("rollout=\"cam\": the rows come out of a backward, and this call records no graph (nothing requires a "
                                 "gradient, torch.no_grad() is active, or lengths= without net.varlen_grad / net.varlen_train)")
            roll = _RolloutRequest(roll[1])
        if node:
            if want_dx:
                # the kernels read a dense f32 spectrogram: the conversion happens where autograd sees it, so x.grad comes back in the
                # caller's own shape, dtype and layout (a sliced / transposed / 16-bit x)
                x = x.contiguous().float()
            if named is None:
                named = self._graph_params()[0]
            fl = self._flat
            if fl is not None and fl["named"] is not named:     # surgery since bind time: the optimizer re-binds at its next step
                self.unbind_flat_grads()
                fl = None
            # bound (same validated parameter list as at bind time): the single token stands for every parameter
            params = (fl["token"],) if fl is not None else [p for _, p in named]
            r = _Fwd.from_flat(_PasstFunction.apply(self, lengths, hid, amap if agrad is None else req, roll, drop_path_masks,
                                                    attn_drop_seed if any(ad_t) else None, x, *params), len(hid or ()),
                               len(amap[0]) if amap else 0, roll is not None)
        elif lengths is None and hid is None and amap is None and roll is None:
            if attn_drop_seed is not None and any(ad_t):
                return passt_forward(self, x, save=False, drop_path_masks=drop_path_masks, attn_drop_seed=attn_drop_seed)[:2]
            if drop_path_masks is not None:
                return passt_forward(self, x, save=False, drop_path_masks=drop_path_masks)[:2]
            return passt_forward(self, x, save=False)[:2]       # the plain call stays on the public entry (callers stand in for it)
        else:
            # the ragged forward records nothing unless asked to; the fixed one leaves that to the caller's own grad mode
            with torch.no_grad() if lengths is not None else contextlib.nullcontext():
                r = _run_forward(self, x, lengths, hidden=hid, attn=amap, rollout=roll,
                                 **({} if drop_path_masks is None else dict(drop_path_masks=drop_path_masks)),
                                 **({} if attn_drop_seed is None or not any(ad_t) else dict(attn_drop_seed=attn_drop_seed)))
        res = self._outputs(r, hid, amap)
        if agrad is not None:
            req.targets = list(res[2 if hid is None else 3])      # the tensors the caller holds: the backward fills their .grad
        if isinstance(roll, _RolloutRequest):
            roll.target = res[2 + (hid is not None) + (amap is not None)]
        return res

    @compile_opaque                 # one opaque eager call under torch.compile, like forward
    def forward_windows(self, x, lengths=None, *, window=None, hop=None, tail="align", pool="mean", pool_of="logits", max_tokens=None):
        """Sliding-window inference over recordings longer than the time embedding: -> (logits, features, win).

        ``x`` (B, 1, n_mels, T_max): B recordings, left-aligned; ``lengths``: frames per recording (sequence of ints or 1-D integer
        tensor; None = all of them T_max).  What lies behind a recording's length is never read.  Eval mode only
        (NotImplementedError in training mode); the outputs carry no grad_fn, like the default ragged forward; the precision is
        ``forward``'s (``precision`` / autocast).

        ``window`` (frames, default img_size[1]) and ``hop`` (default window // 2): a recording of n frames gets, for n <= window,
        the one window [0, n); otherwise K = ceil((n - window) / hop) + 1 windows.  ``tail`` = "align": starts k * hop for
        k < K - 1 and the last window at n - window -- every window is full and every frame is covered; "short": starts k * hop
        with lengths min(window, n - start), a last window shorter than one patch is dropped and listed in ``win.dropped``.  The
        hop is free: no multiple of the patch stride is asked for.  ValueError: window < one patch, hop < 1 or > window, a window
        with more patch columns than the time embedding (windows are never cut and never warn), a recording shorter than one
        patch or longer than T_max.  Every refusal comes before anything is launched.

        Window w of recording b gets what ``net(x[b:b+1, :, :, s:e])`` returns alone at batch size 1 in eval mode (time embedding
        from offset 0).  No unfolded copy is made: the patch gather reads every window in place (pa_patch_gather_windows), and all
        windows of all recordings run as ONE packed sequence through the kernels of ``net(x, lengths=)``; for the same windows the
        outputs equal ``net(unfolded, lengths=win.length)`` bit for bit.

        ``win`` (Windows): ``logits`` (W, C), ``features`` (W, D) per window; ``offsets`` (int64 CPU, B + 1): recording b owns
        windows offsets[b]:offsets[b + 1]; ``start`` / ``length`` (int64 CPU, W, frames); ``dropped``: [(recording, start, length)].

        ``pool`` "mean" / "max": the returned logits (B, C) and features (B, D) are pooled over each recording's own windows on
        the device (pa_window_pool: f32, rows in order, deterministic); ``pool_of`` = "sigmoid" pools sigmoid(logits) instead of
        the logits, the features are always pooled raw.  ``pool`` None returns the per-window tensors in their place.

        ``max_tokens``: None = one packed pass.  Otherwise the windows go, in order, into chunks of at most that many packed
        tokens (a single larger window is its own chunk), one packed pass per chunk: the same ``win`` geometry, outputs equal to the
        unchunked call within rounding (the GEMM plans depend on the row count), not bit for bit."""
        lengths, window, hop = check_window_call(self, x, lengths, window, hop, tail, pool, pool_of, max_tokens)
        win = _passt_forward_windows(self, x, lengths, window, hop, tail, max_tokens)
        return pool_windows(win.logits, win.features, win.offsets, pool, pool_of) + (win,)

    def _outputs(self, r, hid, amap):
        """A forward's record in forward()'s shape: (logits, features[, [token outputs]][, [attention maps]][, tok_offsets]); a packed
        batch's maps (one flat buffer each) are cut into the clips' views here."""
        res = (r.logits, r.feat)
        if hid is not None:
            res += (list(r.hidden),)
        if amap is not None:
            res += ([m if r.tok_offsets is None else _PackedLayout.attn_views(m, r.tok_offsets, self.num_heads, amap[1], amap[2])
                     for m in r.maps],)
        if r.roll is not None:
            res += (r.roll if r.tok_offsets is None else _PackedLayout.rollout_views(r.roll, r.tok_offsets),)
        return res if r.tok_offsets is None else res + (r.tok_offsets,)


# --------------------------------------------------------------------------------------------
# architecture constructors + get_model  (models/passt.py:734-1018)
# --------------------------------------------------------------------------------------------
_ARCHS = {
    # arch name -> (depth, expected stride, note)
    "passt_deit_bd_p16_384": (12, None),
    "passt_s_kd_p16_128_ap486": (12, (10, 10)),
    "passt_l_kd_p16_128_ap47": (7, (10, 10)),
    "passt_s_swa_p16_128_ap476": (12, (10, 10)),
    "passt_s_swa_p16_128_ap4761": (12, (10, 10)),
    "passt_s_p16_128_ap472": (12, (10, 10)),
    "passt_s_p16_s16_128_ap468": (12, (16, 16)),
    "passt_s_swa_p16_s16_128_ap473": (12, (16, 16)),
    "passt_s_swa_p16_s14_128_ap471": (12, (14, 14)),
    "passt_s_p16_s14_128_ap469": (12, (14, 14)),
    "passt_s_swa_p16_s12_128_ap473": (12, (12, 12)),
    "passt_s_p16_s12_128_ap470": (12, (12, 12)),
    "passt_s_f128_20sec_p16_s10_ap474": (12, (10, 10)),
    "passt_s_f128_30sec_p16_s10_ap473": (12, (10, 10)),
}


def fix_embedding_layer(model, embed="default"):
    if embed != "default":
        raise NotImplementedError("only embed='default' is reachable in the reference (models/passt.py:924-931)")
    return model


def lighten_model(model, cut_depth=0):
    """models/passt.py:934-954."""
    if cut_depth == 0:
        return model
    old = list(model.blocks.children())
    if cut_depth < 0:
        old = [old[0]] + old[1:-1:-cut_depth] + [old[-1]]
    else:
        if len(model.blocks) < cut_depth + 2:
            raise ValueError(f"Cut depth a VIT with {len(model.blocks)} layers should be between 1 and "
                             f"{len(model.blocks) - 2}")
        old = [old[0]] + old[cut_depth + 1:]
    model.blocks = nn.Sequential(*old)
    return model


def get_model(arch="passt_s_kd_p16_128_ap486", pretrained=True, n_classes=527, in_channels=1, fstride=10, tstride=10,
              input_fdim=128, input_tdim=998, u_patchout=0, s_patchout_t=0, s_patchout_f=0):
    """Same signature/defaults as models/passt.py:958-961.  ``pretrained=True`` needs a checkpoint
    download (vit_helpers.py:85-91) which this offline build cannot do: pass ``pretrained=False`` and
    ``load_state_dict`` a reference checkpoint (identical keys)."""
    if arch not in _ARCHS:
        raise RuntimeError(f"Unknown model {arch}")
    ckpt = None
    if pretrained:
        # the reference downloads <arch>.pt from its GitHub release (models/helpers/vit_helpers.py:85-91); this build is
        # offline, so the checkpoint must already be on disk: PASST_AMD_CHECKPOINT_DIR/<arch>.pt (same file, same keys)
        ckpt_dir = os.environ.get("PASST_AMD_CHECKPOINT_DIR")
        ckpt = os.path.join(ckpt_dir, arch + ".pt") if ckpt_dir else None
        if not ckpt or not os.path.isfile(ckpt):
            raise RuntimeError(f"pretrained=True: no local checkpoint for {arch} (no network here to download the reference's "
                               f"release file).  Put {arch}.pt into a directory and set PASST_AMD_CHECKPOINT_DIR to it, or use "
                               "pretrained=False and model.load_state_dict(torch.load(<reference .pt>))")
    depth, want = _ARCHS[arch]
    stride = (fstride, tstride)
    if want is not None and stride != want:
        warnings.warn(f"This model was pre-trained with strides {want}, but now you set (fstride,tstride) to {stride}.")
    model = PaSST(u_patchout=u_patchout, s_patchout_t=s_patchout_t, s_patchout_f=s_patchout_f,
                  img_size=(input_fdim, input_tdim), patch_size=16, stride=stride, in_chans=in_channels,
                  num_classes=n_classes, embed_dim=768, depth=depth, num_heads=12, distilled=True)
    if ckpt is not None:
        sd = torch.load(ckpt, map_location="cpu")
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
        if n_classes != 527:       # the reference drops the classifier of the pre-trained net when the label set differs
            sd = {k: v for k, v in sd.items() if not k.startswith(("head.1.", "head_dist."))}
            missing = model.load_state_dict(sd, strict=False)
            assert all(k.startswith(("head.1.", "head_dist.")) for k in missing.missing_keys), missing
        else:
            model.load_state_dict(sd, strict=True)
    model = fix_embedding_layer(model)
    model = lighten_model(model)
    return model


get_model_passt = get_model     # hear21passt's name for the same function (README.md:49,70,77)


class EnsembelerModel(nn.Module):
    """models/passt.py:1021-1037."""

    def __init__(self, models):
        super().__init__()
        self.models = nn.ModuleList(models)

    def forward(self, x, lengths=None, hidden=None, attn=None, attn_grad=None, rollout=None, rollout_from=0):
        """``lengths``: handed to every member (PaSST.forward's ragged-batch eval forward; gradients flow through the members that
        set ``varlen_grad``).  ``hidden`` and ``attn`` are not for an ensemble: its members have different depths, widths and heads."""
        if hidden is not None:
            raise ValueError("EnsembelerModel.forward: hidden= is not supported (the members' token sequences have different widths "
                             "and depths and cannot be averaged); call the member you want: model.models[i](x, hidden=...)")
        if rollout is not None or rollout_from != 0:
            raise ValueError("EnsembelerModel.forward: rollout= is not supported, as attn= is not; call the member you want: "
                             "model.models[i](x, rollout=...)")
        if attn_grad is not None and attn_grad is not False:
            raise ValueError("EnsembelerModel.forward: attn_grad= is not supported, as attn= is not; call the member you want: "
                             "model.models[i](x, attn=..., attn_grad=...)")
        if attn is not None:
            raise ValueError("EnsembelerModel.forward: attn= is not supported (the members have different depths, heads and token "
                             "counts; their attention maps cannot be averaged); call the member you want: model.models[i](x, attn=...)")
        all_out = None
        for m in self.models:
            out, _ = m(x) if lengths is None else m(x, lengths=lengths)
            all_out = out if all_out is None else out + all_out
        all_out = all_out / len(self.models)
        return all_out, all_out

    def forward_windows(self, x, lengths=None, *, window=None, hop=None, tail="align", pool="mean", pool_of="logits", max_tokens=None):
        """PaSST.forward_windows for the ensemble, mirroring ``forward``: the mean of the members' per-window logits, pooled
        afterwards; as there, the second output repeats the first (``win.features`` is ``win.logits``).  ``window`` / ``hop``
        default to the first member's; every member must accept the rule, all refusals come before the first launch."""
        if window is None:
            window = self.models[0].patch_embed.img_size[1]
        if hop is None:
            hop = window // 2
        for m in self.models:
            check_window_call(m, x, lengths, window, hop, tail, pool, pool_of, max_tokens)
        all_out = win = None
        for m in self.models:
            _, _, win = m.forward_windows(x, lengths, window=window, hop=hop, tail=tail, pool=None, max_tokens=max_tokens)
            all_out = win.logits if all_out is None else win.logits + all_out
        all_out = all_out / len(self.models)
        win = win._replace(logits=all_out, features=all_out)
        return pool_windows(all_out, all_out, win.offsets, pool, pool_of) + (win,)


def get_ensemble_model(arch_list=[], *, pretrained=True):
    """models/passt.py:1039-1045: every member through get_model() with ITS default pretrained=True, i.e. here through the
    local checkpoint directory (PASST_AMD_CHECKPOINT_DIR/<arch>.pt; raises without one: no network).  `pretrained` is a
    keyword-only extension for random-init members (tests, benchmarks)."""
    models_list = [get_model(arch=a, fstride=f, tstride=t, pretrained=pretrained) for a, f, t in arch_list]
    model = EnsembelerModel(models_list)
    print(model)
    return model


try:  # the reference exposes these through a sacred/ba3l ingredient (models/passt.py:915-922)
    from ba3l.ingredients.ingredient import Ingredient  # type: ignore

    model_ing = Ingredient("passt")
    model_ing.add_config(instance_cmd="get_model")
    fix_embedding_layer = model_ing.command(fix_embedding_layer)
    lighten_model = model_ing.command(lighten_model)
    get_model = model_ing.command(get_model)
    get_ensemble_model = model_ing.command(get_ensemble_model)
except Exception:  # ba3l not installed: plain functions
    model_ing = None

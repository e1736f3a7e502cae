"""The training step of the reference's caller, on the kernel path.

Mirrors ``M.training_step`` (ex_audioset.py:155-198) + the optimizer step Lightning performs:
waveform -> AugmentMelSTFT (:158) -> spectrogram mixup (:171-177, helpers/mixup.py) -> PaSST (:179)
-> BCE-with-logits mean on the mixed targets (:181-186) -> backward -> gradient all-reduce (DDP) ->
AdamW (:104-109) or SGD (model_speed_test, :392).  No autograd graph is built: forward/backward are
explicit kernel sequences, parameters and gradients live in flat f32 buffers (one fused optimizer
launch, per-block all-reduce buckets).
"""
import os

import numpy as np
import torch

from . import ops
from .ddp import GradReducer
from .passt import (_checked_input, _freq_rows, _precision, attn_drop_draw, attn_drop_rates, check_patchout_varlen, drop_path_draws,
                    drop_path_rates, param_stage, refuse_varlen_attn_drop,
                    passt_backward, passt_backward_varlen, passt_forward, passt_forward_varlen, patchout_draws, refuse_varlen_drop_path,
                    varlen_regularized,
                    trainable_plan)
from .preprocess import checked_lengths

# What the front end writes for a silent cell, (ln(0 + 1e-5) + 4.5) / 5 (models/preprocess.py:78,84), as one float32: the value a
# shorter mixup partner is continued with on a ragged batch (TrainStep.step(lengths=); TrainStep(mixup_pad=) overrides it)
MIXUP_PAD = float(np.float32((np.log(1e-5) + 4.5) / 5.0))


def group_scales(named_dims, depth, layer_decay=None, no_weight_decay=(), model_no_weight_decay=()):
    """The parameter groups of a fine-tuning recipe as one (lr_scale, wd_scale) pair per parameter, or None when there are none (every
    pair would be (1, 1)).  ``named_dims``: [(name, p.dim())] in flat-buffer order.
    ``layer_decay`` = d: the learning rate of stage s (passt.param_stage) is scaled by d ** (depth - s) -- the head by 1, block i by
    d ** (depth - i), the patch stage by d ** (depth + 1).
    ``no_weight_decay``: the names whose weight decay is 0, or "bias_norm": every 1-D parameter plus ``model_no_weight_decay``
    (net.no_weight_decay(): the tokens and position tables)."""
    if isinstance(no_weight_decay, str):
        if no_weight_decay != "bias_norm":
            raise ValueError(f'no_weight_decay: a collection of parameter names or "bias_norm", got {no_weight_decay!r}')
        nwd = {n for n, dim in named_dims if dim <= 1} | set(model_no_weight_decay)
    else:
        nwd = set(no_weight_decay)
        unknown = nwd - {n for n, _ in named_dims} - set(model_no_weight_decay)
        if unknown:
            raise ValueError(f"no_weight_decay names no trainable parameter: {sorted(unknown)[:3]}")
    if layer_decay is None and not any(n in nwd for n, _ in named_dims):
        return None
    d = 1.0 if layer_decay is None else float(layer_decay)
    return [(d ** (depth - param_stage(n, depth)), 0.0 if n in nwd else 1.0) for n, _ in named_dims]


class TrainStep:
    def __init__(self, net, mel=None, lr=2e-5, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, optimizer="adamw",
                 mixup_alpha=0.3, use_mixup=True, process_group=None, loss="bce", comm_dtype="fp32", transport="torch", graph=False,
                 layer_decay=None, no_weight_decay=(), clip_grad_norm=None, accumulate=1, mixup_pad=None):
        """A partly frozen network (``requires_grad`` as it stands at construction) is trained as it is: the flat buffers, the moments
        and the all-reduce buckets span the trainable parameters only, the frozen ones keep their storage and are never written, the
        forward keeps nothing of the blocks below the lowest trainable stage and the backward ends behind it (passt.trainable_plan).
        ``layer_decay`` / ``no_weight_decay`` (AdamW): parameter groups, see group_scales -- one fused launch per bucket as without
        them (pa_adamw_stage_groups), in graph mode too: the groups' factors multiply the learning rate the schedule sets.
        graph=True (single GPU): after ``graph_warmup`` eager steps the network's forward, the loss, the backward and the
        per-bucket optimizer launches (~290 of the step's ~300 launches) are captured once as a hipGraph (torch.cuda.CUDAGraph)
        and replayed; only the front end, mixup and the uploads of the step's host-drawn arrays stay eager.  Same kernels, same
        arguments, bit-identical parameters (tests/test_gpu_model.py::test_train_step_graph_equals_eager); what changes is the
        host: one replay instead of ~290 ctypes launches -- it matters where the step is short (ESC-50 at batch 12).
        Stochastic depth (a net built with drop_path_rate > 0): the step's factors are drawn on the device ahead of the replay
        (passt.drop_path_draws, where the eager forward draws them) into a buffer of fixed address next to the Patchout indices.
        Attention dropout (net.blocks[i].attn.attn_drop.p > 0): the step's seed is drawn the same way (passt.attn_drop_draw, behind
        the drop-path draws) into a (2,) buffer next to them; the dropout kernels read it from device memory, so the captured
        launches replay with a new mask every step.
        ``clip_grad_norm`` = c (AdamW; Lightning's trainer.gradient_clip_val): the update uses g * min(1, c / (norm + 1e-6)), norm
        being the global L2 norm over the flat gradient buffer (the trainable parameters; torch.nn.utils.clip_grad_norm_'s
        arithmetic).  Every bucket's partial sums of squares go out from the backward (pa_grad_accum_sumsq), the factor is formed
        on the device (pa_clip_coef) and the per-bucket AdamW launches read it from there (pa_adamw_stage_clip / pa_adamw_clip),
        after the backward: no host sync, capturable.  ``flat_g`` / ``p.grad`` keep the UNCLIPPED gradients (torch clips in
        place; not writing them saves a pass over the buffer).  ``grad_norm``: the last update's pre-clip norm, a 1-element
        device tensor.
        ``accumulate`` = k (trainer.accumulate_grad_batches): ``step()`` is called once per micro-batch and returns its loss; the
        loss gradient carries 1 / (world k); micro-steps 1 .. k - 1 fold their finished buckets into a second flat buffer
        (``flat_acc``) and touch nothing else -- no all-reduce (Lightning's no_sync), no optimizer launch, ``t`` stands still; the
        k-th folds, all-reduces, and updates from the accumulated buffer.  ``flush()`` applies a partial accumulation (the end
        of an epoch whose batch count is no multiple of k).
        ``mixup_pad`` (None: MIXUP_PAD, the front end's value of a silent cell): what a shorter mixup partner is continued with in a
        ragged step, see ``step(..., lengths=)``; not read by fixed-shape steps."""
        self.net, self.mel = net, mel
        self.mixup_pad = MIXUP_PAD if mixup_pad is None else float(mixup_pad)
        self.lr, self.wd, self.betas, self.eps, self.optimizer = lr, weight_decay, betas, eps, optimizer
        self.mixup_alpha, self.use_mixup = mixup_alpha, use_mixup
        assert loss in ("bce", "ce")      # bce: ex_audioset.py:181-186 ; ce: ex_esc50.py:159-165 (class-index targets)
        self.loss = loss
        if clip_grad_norm is not None and not float(clip_grad_norm) > 0.0:
            raise ValueError(f"TrainStep: clip_grad_norm must be positive (or None: no clipping), got {clip_grad_norm!r}")
        if clip_grad_norm is not None and optimizer != "adamw":
            raise ValueError("TrainStep: clip_grad_norm rides on the AdamW launches (pa_adamw_stage_clip); optimizer='sgd' has no such form")
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"TrainStep: accumulate is a count of micro-batches >= 1, got {accumulate!r}")
        self.clip = None if clip_grad_norm is None else float(clip_grad_norm)
        self.accumulate, self._micro, self._last = int(accumulate), 0, True
        dev = next(net.parameters()).device
        self.plan = trainable_plan(net)
        if not self.plan.wanted:
            raise ValueError("TrainStep: no PaSST parameter requires a gradient (head_dist.* is never trained): nothing to update")
        names = self.plan.wanted
        self.named = [(n, p) for n, p in net.named_parameters() if n in names]
        self._frozen_ids = {id(p) for p in net.parameters()} - {id(p) for _, p in self.named}
        self.groups = group_scales([(n, p.dim()) for n, p in self.named], len(net.blocks), layer_decay, no_weight_decay,
                                   net.no_weight_decay())
        if self.groups is not None and optimizer != "adamw":
            raise ValueError("TrainStep: layer_decay / no_weight_decay are parameter groups of AdamW; optimizer='sgd' has none")
        self._group_tabs = {}
        total = sum(p.numel() for _, p in self.named)
        # flat parameter buffer: every nn.Parameter becomes a view (state_dict / load_state_dict keep working)
        self.flat_p = torch.empty(total, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(total, device=dev, dtype=torch.float32)
        self.grads, off = {}, 0
        for n, p in self.named:
            k = p.numel()
            self.flat_p[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat_p[off:off + k].view(p.shape)
            self.grads[n] = self.flat_g[off:off + k].view(p.shape)
            p.grad = self.grads[n]
            off += k
        self.m = torch.zeros_like(self.flat_p) if optimizer == "adamw" else None
        self.v = torch.zeros_like(self.flat_p) if optimizer == "adamw" else None
        # accumulate > 1: the buffer the micro-batches' gradients are summed in; the all-reduce and the optimizer read THIS one
        self.flat_acc = torch.zeros_like(self.flat_g) if self.accumulate > 1 else None
        self._gbuf = self.flat_g if self.flat_acc is None else self.flat_acc
        self.reducer = GradReducer(self._gbuf, [(n, p.numel()) for n, p in self.named], len(net.blocks), process_group,
                                   comm_dtype=comm_dtype, transport=transport)
        # identical replicas: rank 0's parameters everywhere (what Lightning's DDP wrapper does at construction,
        # ex_audioset.py:488-489); a caller that seeded per rank or loaded different state must not train diverging copies
        self.reducer.broadcast_(self.flat_p)
        if self.reducer.world > 1 and os.environ.get("PASST_AMD_DDP_PERSISTENT") != "1":
            # the all-reduce kernels of the communication stream take CUs while the backward runs: GEMMs go out one work
            # item per workgroup (the hardware hands them to whatever CUs are free: -1.6 % alone on one GPU) instead of as 256
            # resident workgroups, which would wait for the occupied CUs and double the launch (PA_GEMM_NO_PERSIST).
            # Per model (net._gemm_flags rides on every pa_gemm_nt call of this net's forward / backward); close() undoes it.
            object.__setattr__(net, "_gemm_flags", getattr(net, "_gemm_flags", 0) | ops._lib.GEMM_NO_PERSIST)
            self._set_no_persist = True
        if graph and self.accumulate > 1:
            raise NotImplementedError("TrainStep(graph=True) with accumulate > 1 is not supported: the folding micro-steps and the "
                                      "updating one are two different launch sequences, i.e. two captured graphs; use graph=False")
        self.graph = bool(graph) and self.reducer.world == 1
        if self.graph and optimizer != "adamw":
            raise NotImplementedError("TrainStep(graph=True) captures the per-bucket AdamW launches (pa_adamw_dev reads its scalars "
                                      "from device memory); optimizer='sgd' has no such form: use graph=False")
        self.graph_warmup, self._g = 3, None
        self.t = self._t_now = 0
        self.block_optimizer = os.environ.get("PASST_AMD_BLOCK_OPT", "1") != "0"      # one GPU: per-bucket updates from the backward
        self.base_lr = lr
        # AdamW and the GEMM-ready weight copies in one launch per bucket (pa_adamw_stage, round 6): the copies the next forward
        # needs are written from the registers that hold the updated parameters; PASST_AMD_NO_FUSED_STAGE=1: A/B, the optimizer
        # leaves them stale and the next forward's first GEMM refreshes all of them with one pa_stage_weights launch
        self.fused_stage = optimizer == "adamw" and os.environ.get("PASST_AMD_NO_FUSED_STAGE") != "1"
        self._offsets = []
        off = 0
        for _, p in self.named:
            self._offsets.append(off)
            off += p.numel()
        self._fresh = []
        # clipping: one run of partial slots per bucket (pa_grad_norm_partials of its span) in ONE array, [norm, factor] behind it
        self._part, self.grad_norm = {}, None
        if self.clip is not None:
            n_part = 0
            for s_, e_ in self._spans():
                k = ops.grad_norm_partials(e_ - s_)
                self._part[(s_, e_)] = (n_part, n_part + k)
                n_part += k
            self._partials = torch.zeros(n_part, device=dev, dtype=torch.float32)
            self._clip_out = torch.zeros(2, device=dev, dtype=torch.float32)
            self.grad_norm = self._clip_out[:1]
        net.mark_params_updated()

    def _spans(self):
        """the non-empty buckets' flat spans in the order the backward completes them"""
        return [se for se in (self.reducer.spans[b] for b in self.reducer.launch_order()) if se[1] > se[0]]

    def _norm_partials(self, s, e, fold=False):
        """bucket [s, e): its partial sums of squares -- of the gradients as they stand, or (fold) of the accumulated buffer in the
        pass that adds this micro-batch to it"""
        a, b = self._part[(s, e)]
        if fold:
            ops.grad_accum_sumsq(self.flat_g[s:e], self.flat_acc[s:e], first=self._micro == 0, partials=self._partials[a:b])
        else:
            ops.grad_accum_sumsq(self._gbuf[s:e], partials=self._partials[a:b])

    def _optimizer(self, s, e):
        """the update of bucket [s, e): one launch"""
        capturing = self._g is not None and self._g.get("capturing")
        if self.optimizer != "adamw":
            if capturing:
                raise NotImplementedError("graph mode: AdamW only")
            return ops.sgd(self.flat_p[s:e], self._gbuf[s:e], self.lr)
        # the step's scalars: inside the capture from device memory (launch arguments must not change between replays)
        hyper = self._g["hyper"] if capturing else (self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self._t_now)
        # the clip factor: device memory as well (pa_clip_coef wrote it behind the backward)
        gs = None if self.clip is None else self._clip_out[1:]
        table, scales, dt, keys = None, None, None, []
        if self.fused_stage and not capturing:
            # the bucket's parameters and their GEMM-ready copies.  No kernel enqueued after this point reads this bucket's copies
            # before the next forward: the bucket's own input-gradient GEMMs (the readers of W^T) are already on the stream, earlier
            # blocks read their own weights
            dt = _precision(self.net)
            lo, hi = self._span_params(s, e)
            *table, keys = self.net._staged.adamw_table((s, e), [(self.named[i][1], self._offsets[i] - s) for i in range(lo, hi)], dt)
            scales = None if self.groups is None else self._group_table(s, e)[3]
        elif self.groups is not None:
            # one entry per parameter, no copies: no dtype either (pa_adamw_groups) -- pa_adamw_stage_clip takes one all the same
            *table, scales = self._group_table(s, e)
            dt = None if gs is None else _precision(self.net)
        ops.adamw_update(self.flat_p[s:e], self._gbuf[s:e], self.m[s:e], self.v[s:e], hyper, table=table, scales=scales, dtype=dt, gscale=gs)
        self._fresh += keys

    def _group_table(self, s, e):
        """(plain descriptor table, n, work items, scales) of flat span [s, e) for the launches with parameter groups: one entry per
        parameter, no copies (pa_adamw_groups); the scales alone serve pa_adamw_stage_groups, whose table lists the same parameters
        in the same order.  Uploaded once per span (graph mode: ahead of the capture)."""
        hit = self._group_tabs.get((s, e))
        if hit is None:
            lo, hi = self._span_params(s, e)
            dev = self.flat_p.device
            tab = ops.make_adamw_stage_table([(self._offsets[i] - s, 1, self.named[i][1].numel(), None, None) for i in range(lo, hi)], dev)
            hit = self._group_tabs[(s, e)] = tab + (ops.make_adamw_scales(self.groups[lo:hi], dev),)
        return hit

    def _span_params(self, s, e):
        """indices [lo, hi) into self.named of the parameters that make up flat span [s, e) (spans are unions of whole parameters)"""
        import bisect
        lo, hi = bisect.bisect_left(self._offsets, s), bisect.bisect_left(self._offsets, e)
        assert self._offsets[lo] == s and (hi == len(self._offsets) or self._offsets[hi] == e)
        return lo, hi

    def _params_updated(self):
        """End of a step: every parameter changed (epoch bump: all staged copies stale) -- except that the copies the fused
        optimizer launches of this step rewrote are current."""
        st = self.net._staged
        if self._frozen_ids:
            # ... and so are the copies of the frozen weights that were current before the bump: the step wrote none of those
            # parameters (one stale copy would make the next forward refresh every copy, the frozen ones included).  One that was
            # NOT current stays stale: the caller wrote the weight since its copy was made -- between a folding micro-step and
            # flush(), or while the network ran in the other precision
            self._fresh += [k for k, ent in st.cache.items() if k[0] in self._frozen_ids and ent[0] == st._version(ent[2])]
        self.net.mark_params_updated()
        if self._fresh:
            st.mark_fresh(self._fresh)
            self._fresh = []

    def _block_done(self, i):
        """Called by the backward on its finishing stream once bucket i's gradients are complete (head, blocks depth-1 .. 0,
        patch embedding).  One GPU: update that bucket's parameters right away -- no later kernel of this backward reads
        them (input gradients use the bf16 copies staged before the step), so the bandwidth-bound optimizer pass runs next
        to the remaining blocks' GEMMs instead of after them.  Several GPUs: start the bucket's all-reduce."""
        s, e = self.reducer.spans[i]
        one_gpu = self.reducer.world == 1
        if self.flat_acc is not None and e > s:
            # gradient accumulation: fold this micro-batch's bucket into the accumulated buffer -- and, on the updating micro-step of
            # one GPU with clipping, take the partial sums of squares of the result in the same pass
            if self._last and one_gpu and self.clip is not None:
                self._norm_partials(s, e, fold=True)
            else:
                ops.grad_accum_sumsq(self.flat_g[s:e], self.flat_acc[s:e], first=self._micro == 0)
        if not self._last:
            return                  # no all-reduce (Lightning's no_sync), no update
        if not one_gpu:
            return self.reducer.on_block_done(i)
        if self.clip is not None:
            # the norm needs every bucket: the extra read overlaps the rest of the backward, the updates go out behind it (_apply)
            if self.flat_acc is None and e > s:
                self._norm_partials(s, e)
        elif self.block_optimizer and e > s:
            self._optimizer(s, e)

    def _apply(self, flush=False):
        """The launches that end an update, behind the backward (or from flush()): all-reduce waits, the clip factor, and every
        optimizer launch _block_done could not issue."""
        total = self.flat_p.numel()
        if self.reducer.world > 1:
            if flush:                                       # the folding micro-steps reduced nothing
                for b in self.reducer.launch_order():
                    self.reducer.on_block_done(b)
            # one optimizer launch per all-reduce bucket, in the order the buckets were launched: the update of bucket k runs
            # while buckets k+1.. are still on the wire, so the LAST bucket (block 0 + patch embedding, released only when
            # the backward ends) is covered by ~0.4 ms of optimizer work instead of being exposed in front of one big launch.
            # With clipping a bucket's partial sums take the update's place here; the updates follow the factor.
            for s_, e_ in self.reducer.drain():
                if self.clip is None:
                    self._optimizer(s_, e_)
                else:
                    self._norm_partials(s_, e_)
        elif flush and self.clip is not None:
            for s_, e_ in self._spans():
                self._norm_partials(s_, e_)
        if self.clip is not None:
            ops.clip_coef(self._partials, self.clip, self._clip_out)
            if self.reducer.world == 1 and not self.block_optimizer:
                self._optimizer(0, total)
            else:
                for s_, e_ in self._spans():
                    self._optimizer(s_, e_)
        elif self.reducer.world == 1:
            if not self.block_optimizer:
                self._optimizer(0, total)
            elif flush:
                for s_, e_ in self._spans():
                    self._optimizer(s_, e_)

    def flush(self):
        """Apply what has accumulated since the last update (accumulate > 1: fewer than k micro-steps; the gradients keep their
        1 / k scale, as Lightning's last update of an epoch does).  Nothing pending: nothing happens."""
        if self._micro == 0:
            return
        self._t_now = self.t + 1
        self._apply(flush=True)
        self.t = self._t_now
        self._micro = 0
        self._params_updated()

    def close(self):
        """Release the reducer's communicator (C-ABI RCCL transport); torch.distributed groups belong to the caller."""
        self.reducer.close()
        if getattr(self, "_set_no_persist", False):
            object.__setattr__(self.net, "_gemm_flags", getattr(self.net, "_gemm_flags", 0) & ~ops._lib.GEMM_NO_PERSIST)
            self._set_no_persist = False

    def set_lr_factor(self, factor):
        """Per-epoch LR schedule (ex_audioset.py:86-101): lr = base_lr * factor, e.g. from
        schedule.exp_warmup_linear_down(5, 50, 50, 0.01)(epoch)."""
        self.lr = self.base_lr * float(factor)

    # ---- captured-graph mode ------------------------------------------------------------------------------------------
    def _graph_fill(self, g, d, x, y, y2, lam_d):
        g["x"].copy_(x)
        g["y"].copy_(y)
        if y2 is not None:
            g["y2"].copy_(y2)
        if lam_d is not None:
            g["lam"].copy_(lam_d)
        g["pf"].copy_(ops.upload_small(d["pf"], x.device))
        g["pt"].copy_(ops.upload_small(d["pt"], x.device))
        g["pt_pos"].copy_(ops.upload_small(d["pt"] + np.int32(d["toff"]), x.device))
        if g["dp"] is not None:
            g["dp"].copy_(d["dp"])          # stochastic depth: the step's factors, drawn on the device ahead of the replay
        if g.get("ad") is not None:
            g["ad"].copy_(d["ad"])          # attention dropout: the step's seed
        # (through the pinned ring like the index arrays: a fixed host buffer could be rewritten for step k + 1 before the
        # asynchronous copy of step k has read it)
        ops.adamw_hyper(self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self._t_now, g["hyper_host"])
        g["hyper"].copy_(ops.upload_small(g["hyper_host"], x.device))

    def _graph_body(self, g):
        net = self.net
        logits, feat, ctx = passt_forward(net, g["x"], save=self.plan, draws=g)
        if self.loss == "bce":
            loss, dlogits = ops.bce_fwd_bwd(logits, g["y"], grad_scale=1.0)
        elif g["y2"] is not None:
            loss, dlogits = ops.ce_mixup_fwd_bwd(logits, g["y"], g["y2"], g["lam"], grad_scale=1.0)
        else:
            loss, dlogits = ops.ce_mixup_fwd_bwd(logits, g["y"], grad_scale=1.0)
        passt_backward(net, ctx, dlogits, None, self.grads, on_block_done=self._block_done)
        self._apply()
        return loss

    def step(self, wave_or_spec, target, lengths=None):
        """wave (B,1,L) / (B,L) when a mel module was given, else a spectrogram (B,1,F,T).
        Returns the loss as a 1-element device tensor (no host sync).

        ``lengths`` (a sequence of ints or a 1-D integer tensor, one entry per clip): a batch of clips of DIFFERENT lengths,
        left-aligned and padded to the longest -- with a mel module zero-padded waveforms (B, L_max) / (B, 1, L_max) and SAMPLES per
        clip, without one a padded spectrogram (B, 1, F, T_max) and FRAMES per clip (what lies behind a clip's frames is never
        used and may be anything).  The step then runs the packed kernel sequence over the clips' own tokens: ``mel(wave,
        lengths=)``, the ragged mixup below, ``passt_forward_varlen``, today's loss kernels, ``passt_backward_varlen``, and the same
        callbacks as the fixed step -- clipping, accumulation, parameter groups, frozen prefixes, the per-bucket optimizer and the
        reducer are reached through them and have no second form.  ``lengths=None``: the launch sequence and the RNG consumption of
        the fixed step, untouched.

        Mixup on a ragged batch (``use_mixup``): partner j = perm[i] and lam_i are drawn exactly as on the fixed path (one
        ``torch.randperm(B)``, one ``np.random.beta(alpha, alpha, B)``, lam = max(lam, 1 - lam)), whatever the lengths.  The mixed clip
        KEEPS ITS OWN LENGTH n_i; the partner is brought to it the way the reference's loaders bring every clip to one length
        (pad_or_truncate): cut if it is longer, continued with silence if it is shorter, silence at the spectrogram level being the
        constant ``mixup_pad`` (default: what the front end writes for a silent cell, (ln(1e-5) + 4.5) / 5):
            t <  n_i :  out[i, f, t] = x[i, f, t] * lam_i + (x[j, f, t] if t < n_j else pad) * (1 - lam_i)
            t >= n_i :  out[i, f, t] = 0.0 exactly
        (ops.mixup_varlen; with all n_i equal to the row pitch it is ops.mixup bit for bit).  Targets have no time axis and mix as on
        the fixed path; for loss="ce" the partner's label rides in pa_ce_mixup_fwd_bwd.  One difference from a waveform-level pad is
        deliberate: the last frames of a shorter partner are the STFT of a reflect-padded clip end, not of a clip continued with
        zeros, so the seam is not what padding the waveform would give.

        RNG order of a ragged step: all front-end draws of the batch, clip after clip (preprocess.varlen_clip_draws; a mel module in
        eval mode: its two ``randint`` per call); then ``randperm`` and ``beta``; then the Patchout draws, clip after clip
        (passt.varlen_geometry_train); then, with ``net.varlen_regularize = True``, the stochastic-depth draws and the
        attention-dropout seed on the device generator, as the fixed step draws them for a batch of B clips (PaSST.forward).

        Every check runs before the first draw and the first launch, so a rejected step consumes no random number and changes no
        buffer: NotImplementedError for a net in training mode without ``net.varlen_train = True``, for a mel module in training mode
        without ``mel.varlen_train = True``, and -- unless ``net.varlen_regularize = True`` -- for an active ``drop_path_rate`` or
        attention dropout (the refusals of ``net(x, lengths=)``, string for string); the checks of
        ``lengths`` (preprocess.checked_lengths for samples, the packed forward's for frames); the Patchout feasibility of every
        clip (passt.check_patchout_varlen, on frames = 1 + (n - 1) // hop when ``lengths`` are samples).

        graph=True: a step with ``lengths`` always runs the eager sequence, as a batch of another shape does (_graph_fits); a
        captured graph stays valid for later fixed-shape steps."""
        if lengths is not None:
            return self._step_varlen(wave_or_spec, target, lengths)
        net = self.net
        x = wave_or_spec
        if self.mel is not None:
            if x.dim() == 3:
                x = x.reshape(-1, x.shape[2])                                   # mel_forward, :142-145
            x = self.mel(x.contiguous().float()).unsqueeze(1)
        else:
            x = x.contiguous().float()
        # the kernels reinterpret raw memory: hand them dense f32 targets (BCE) / integer class ids (CE)
        y = target.contiguous() if self.loss == "ce" else target.to(torch.float32).contiguous()
        if self.use_mixup:
            B = x.shape[0]
            perm = torch.randperm(B)                                            # helpers/mixup.py:6
            lam = np.random.beta(self.mixup_alpha, self.mixup_alpha, B).astype(np.float32)
            lam = np.maximum(lam, 1.0 - lam)
            perm_d = ops.upload_small(perm.to(torch.int32), x.device)           # page-locked staging: asynchronous H2D
            lam_d = ops.upload_small(lam, x.device)
            x = ops.mixup(x, perm_d, lam_d)
            if self.loss == "bce":
                y = ops.mixup(y, perm_d, lam_d)
        if self.graph and self.t >= self.graph_warmup and self._graph_fits(x):
            return self._graph_step(x, y, perm_d if self.use_mixup else None, lam_d if self.use_mixup else None)
        logits, feat, ctx = passt_forward(net, x, save=self.plan)
        return self._loss_backward_update(logits, ctx, y, perm_d if self.use_mixup else None, lam_d if self.use_mixup else None,
                                          passt_backward)

    def _loss_backward_update(self, logits, ctx, y, perm_d, lam_d, backward):
        """What follows the forward, fixed or packed (``backward``: passt_backward / passt_backward_varlen): the loss kernel, the
        backward with the per-bucket callbacks, and on an updating micro-step the launches that end the update.  ``perm_d`` / ``lam_d``:
        the step's mixup draws on the device, None without mixup."""
        net = self.net
        gs = 1.0 / (self.reducer.world * self.accumulate)
        if self.loss == "bce":
            loss, dlogits = ops.bce_fwd_bwd(logits, y, grad_scale=gs)
        else:
            y32 = y.to(torch.int32)
            if perm_d is not None:
                loss, dlogits = ops.ce_mixup_fwd_bwd(logits, y32, y32[perm_d.long()].contiguous(), lam_d, grad_scale=gs)
            else:
                loss, dlogits = ops.ce_mixup_fwd_bwd(logits, y32, grad_scale=gs)
        # The step count advances only when the whole step was enqueued.  With per-bucket updates (the default) a step that
        # raises in the middle of the backward (out of memory, a PA_E* code) has ALREADY updated the buckets that completed
        # before it (head, later blocks) with step number t + 1 -- parameters, m and v of those buckets -- and not the rest:
        # a failed step is not atomic; recover from a checkpoint (or run with PASST_AMD_BLOCK_OPT=0, where nothing is
        # touched before the backward has finished).
        self._t_now = self.t + 1
        self._last = self._micro + 1 >= self.accumulate         # does this micro-step end with the update?
        backward(net, ctx, dlogits, None, self.grads, on_block_done=self._block_done)
        self._micro += 1
        if not self._last:
            return loss             # parameters, moments, staged copies and t untouched
        self._apply()
        self.t = self._t_now
        self._micro = 0
        self._params_updated()
        return loss

    def _checked_varlen(self, x, lengths):
        """Every check of a ragged step, none of which draws or launches: returns (the front end's input or the spectrogram, samples
        per clip or None, frames per clip)."""
        net, mel = self.net, self.mel
        if net.training and not getattr(net, "varlen_train", False):
            raise NotImplementedError("TrainStep.step(..., lengths=): a network in training mode takes a ragged batch only with the "
                                      "switch net.varlen_train = True (every clip then gets the Patchout it would get alone at batch size 1)")
        if mel is not None and mel.training and not mel.varlen_train:
            raise NotImplementedError("TrainStep.step(..., lengths=): a front end in train mode takes a ragged batch only with the "
                                      "switch mel.varlen_train = True (every clip then gets its own fmin / fmax jitter and masks)")
        if not varlen_regularized(net):         # net.varlen_regularize with an active rate: the packed forward draws and applies them
            refuse_varlen_drop_path(net)
            refuse_varlen_attn_drop(net)
        if mel is not None:
            if x.dim() == 3:
                x = x.reshape(-1, x.shape[2])
            if x.dim() != 2:
                raise ValueError(f"TrainStep.step(..., lengths=): expected (B, L_max) or (B, 1, L_max) waveforms, got {tuple(x.shape)}")
            samples = checked_lengths(mel, lengths, *x.shape)
            frames = [1 + (n - 1) // mel.hopsize for n in samples]
            F, T = mel.n_mels, max(frames)
        else:
            x, _ = _checked_input(net, x, True)
            if torch.is_tensor(lengths):
                if lengths.dim() != 1 or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
                    raise ValueError("lengths must be a sequence of ints or a 1-D integer tensor")
                lengths = lengths.tolist()
            samples, frames = None, [int(v) for v in lengths]
            if len(frames) != x.shape[0]:
                raise ValueError(f"lengths has {len(frames)} entries for a batch of {x.shape[0]} clips")
            F, T = x.shape[2], x.shape[3]
        check_patchout_varlen(net, frames, _freq_rows(net, F), T_max=T)
        return x, samples, frames

    def _step_varlen(self, x, target, lengths):
        """step() on a ragged batch (see there): front end, ragged mixup, packed forward, loss, packed backward, update."""
        net = self.net
        x, samples, frames = self._checked_varlen(x, lengths)
        if self.mel is not None:
            spec, _ = self.mel(x.contiguous().float(), lengths=samples)     # the front-end draws of the batch, clip after clip
            x = spec.unsqueeze(1)
        y = target.contiguous() if self.loss == "ce" else target.to(torch.float32).contiguous()
        perm_d = lam_d = None
        if self.use_mixup:
            B = x.shape[0]
            perm = torch.randperm(B)                                            # helpers/mixup.py:6, as on the fixed path
            lam = np.random.beta(self.mixup_alpha, self.mixup_alpha, B).astype(np.float32)
            lam = np.maximum(lam, 1.0 - lam)
            perm_d = ops.upload_small(perm.to(torch.int32), x.device)
            lam_d = ops.upload_small(lam, x.device)
            lens_d = ops.upload_small(torch.tensor(frames, dtype=torch.int32), x.device)
            x = ops.mixup_varlen(x, lens_d, perm_d, lam_d, self.mixup_pad)
            if self.loss == "bce":
                y = ops.mixup(y, perm_d, lam_d)
        logits, feat, ctx = passt_forward_varlen(net, x, frames, save=self.plan)      # the Patchout draws, clip after clip
        return self._loss_backward_update(logits, ctx, y, perm_d, lam_d, passt_backward_varlen)

    def _graph_fits(self, x):
        """The captured graph replays ONE batch shape.  The reference's loaders never set drop_last, so the last batch of an epoch
        is smaller (and variable-length clips change the frame count): such a step runs the eager kernel sequence instead --
        same kernels, same results, decided here before any of the step's random draws is consumed (the number of kept patches
        follows from the shape alone).  The graph stays valid for the next full batch."""
        g = self._g
        return g is None or "graph" not in g or tuple(x.shape) == tuple(g["x"].shape)

    def _graph_step(self, x, y, perm_d, lam_d):
        """x: mixed spectrogram; y: targets (BCE: already mixed f32; CE: class ids).  Host draws in the eager order, fixed-address
        buffers refilled, ONE graph replay."""
        net = self.net
        y2 = None
        if self.loss == "ce":
            y = y.to(torch.int32)
            if perm_d is not None:
                y2 = y[perm_d.long()].contiguous()
            else:
                lam_d = None
        else:
            lam_d = None
        self._t_now = self.t + 1
        d = patchout_draws(net, x.shape)                     # the Patchout draws of this step, where passt_forward would draw them
        if any(p > 0.0 for p in drop_path_rates(net)):       # ... and behind them the stochastic-depth draws, as passt_forward orders them
            d["dp"] = drop_path_draws(net, x.shape[0], x.device)
        if any(attn_drop_rates(net)):                        # ... and behind those the attention-dropout seed
            d["ad"] = attn_drop_draw(x.device)
        g = self._g
        if g is None or "graph" not in g:
            if g is None:
                g = dict(capturing=False, x=torch.empty_like(x), Np=d["Np"],
                         pf=torch.empty(d["Np"], device=x.device, dtype=torch.int32), pt=torch.empty(d["Np"], device=x.device, dtype=torch.int32),
                         pt_pos=torch.empty(d["Np"], device=x.device, dtype=torch.int32), y=torch.empty_like(y),
                         y2=None if y2 is None else torch.empty_like(y2), lam=None if lam_d is None else torch.empty_like(lam_d),
                         hyper=torch.empty(7, device=x.device, dtype=torch.float32), hyper_host=torch.empty(7, dtype=torch.float32),
                         dp=torch.empty_like(d["dp"]) if "dp" in d else None, ad=torch.empty_like(d["ad"]) if "ad" in d else None)
                self._g = g
            self._graph_fill(g, d, x, y, y2, lam_d)
            net.mark_params_updated()                        # the staged weight copies are stale: their refresh launch is captured too
            net._staged.stage_table(_precision(net))         # (its descriptor table is uploaded here: no copies inside a capture)
            if self.groups is not None:                      # ... and so are the tables and factors of the parameter groups
                for s_, e_ in list(self.reducer.spans.values()) + [(0, self.flat_p.numel())]:
                    if e_ > s_:
                        self._group_table(s_, e_)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            g["capturing"] = True
            try:
                with torch.cuda.graph(graph):
                    g["loss"] = self._graph_body(g)
            finally:
                g["capturing"] = False
            g["graph"] = graph
        else:
            # _graph_fits() routed every other shape to the eager path before the draws; the kept-patch count follows from the shape
            assert d["Np"] == g["Np"] and x.shape == g["x"].shape
            self._graph_fill(g, d, x, y, y2, lam_d)
        g["graph"].replay()
        self.t = self._t_now
        net.mark_params_updated()
        # a fresh tensor per step, like the eager path: the next replay overwrites the captured one, and callers collect losses
        # lazily (append now, .item() later)
        return g["loss"].clone()

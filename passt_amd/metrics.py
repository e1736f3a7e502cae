"""Validation metrics on the device: what validation_step / validation_epoch_end of the reference's experiment files compute with
per-batch ``.cpu()`` copies and two scikit-learn calls (ex_audioset.py:216-291, ex_openmic.py:205-270, ex_fsd50k.py:220-260).

    acc = EvalAccumulator(527)
    for x, y in val_loader:  acc.update(net(x)[0], y)            # device tensors in, nothing comes back
    res = acc.compute();  mAP = res["mAP"].item()                # the caller's .item() is the epoch's one sync

Per-class average precision and ROC-AUC come from pa_eval_append / pa_eval_rank (include/passt_amd.h): exact
integer rank counts, ties as scikit-learn treats them.  No fallback: CPU tensors raise."""
import torch

from . import _lib, ops

_MODES = {"sigmoid": _lib.EVAL_SIGMOID, "raw": _lib.EVAL_RAW}


class EvalAccumulator:
    """Accumulates one validation epoch of a multi-label problem with ``n_classes`` classes.

    scores="sigmoid": update() takes logits; samples are ranked by the f32 sigmoid, as the reference ranks them (its saturation ties
    included), and the validation loss the reference logs is kept as well.  scores="raw": the values are ranked as given
    (probabilities, or logits for a saturation-free ranking); no loss is kept (``val_loss`` is NaN).  capacity: samples the
    buffers hold before they double."""

    def __init__(self, n_classes, capacity=4096, scores="sigmoid"):
        if scores not in _MODES:
            raise ValueError(f"scores must be 'sigmoid' or 'raw', got {scores!r}")
        if int(n_classes) < 1 or int(capacity) < 1:
            raise ValueError("n_classes and capacity must be >= 1")
        self.n_classes, self.capacity, self.scores = int(n_classes), int(capacity), scores
        self._mode = _MODES[scores]
        self._keys = self._state = self._ws = self._loss_sum = self._loss = self._dlogits = self._bce_ws = None
        self.n = self.n_batches = 0

    # ---- storage -----------------------------------------------------------------------------------------------------
    def _alloc(self, dev, capacity):
        keys = torch.empty((self.n_classes, capacity), device=dev, dtype=torch.int32)
        state = torch.empty((self.n_classes, capacity), device=dev, dtype=torch.uint8)
        return keys, state

    def _reserve(self, dev, need):
        if self._keys is None:
            while self.capacity < need:
                self.capacity *= 2
            self._keys, self._state = self._alloc(dev, self.capacity)
            self._loss_sum = torch.zeros(1, device=dev, dtype=torch.float32)
            self._loss = torch.empty(1, device=dev, dtype=torch.float32)
        elif need > self.capacity:
            cap = self.capacity
            while cap < need:
                cap *= 2
            keys, state = self._alloc(dev, cap)
            keys[:, :self.n].copy_(self._keys[:, :self.n])
            state[:, :self.n].copy_(self._state[:, :self.n])
            self._keys, self._state, self._ws, self.capacity = keys, state, None, cap

    # ---- the epoch ---------------------------------------------------------------------------------------------------
    def update(self, scores, target, mask=None):
        """One validation batch: logits (or scores) [B][C], targets [B][C] (positive when > 0.5), optional mask [B][C] (valid when
        > 0.5: OpenMIC's y_mask).  Device f32 tensors; nothing is synchronised, nothing allocated while the capacity lasts."""
        if not scores.is_cuda:
            raise _lib.PasstAmdError("passt_amd kernels need CUDA/HIP tensors (no CPU fallback)")
        if scores.dim() != 2 or scores.shape[1] != self.n_classes:
            raise _lib.PasstAmdError(f"expected [B][{self.n_classes}] scores, got {tuple(scores.shape)}")
        B = scores.shape[0]
        if B == 0:
            return
        self._reserve(scores.device, self.n + B)
        ops.eval_append(scores, target, self._keys, self._state, self.n, mask=mask, mode=self._mode)
        if self._mode == _lib.EVAL_SIGMOID:          # F.binary_cross_entropy_with_logits(y_hat, y).mean() of the batch
            numel = B * self.n_classes
            if self._dlogits is None or self._dlogits.numel() < numel:
                self._dlogits = torch.empty(numel, device=scores.device, dtype=torch.float32)
                self._bce_ws = torch.empty(1 + (numel + 255) // 256, device=scores.device, dtype=torch.float32)
            ops.bce_fwd_bwd(scores, target, grad_scale=0.0, out=(self._loss, self._dlogits, self._bce_ws))
            self._loss_sum.add_(self._loss)
        self.n += B
        self.n_batches += 1

    def reset(self):
        """Start a new epoch; the buffers stay."""
        self.n = self.n_batches = 0
        if self._loss_sum is not None:
            self._loss_sum.zero_()

    def _gathered(self, group):
        """Every rank's columns side by side in rank order (the reference's self.all_gather(out), ex_audioset.py:275-280): lengths
        first, columns padded to the longest, the valid ranges kept."""
        import torch.distributed as dist
        world = dist.get_world_size(group)
        lens = [None] * world
        dist.all_gather_object(lens, (self.n, self.n_batches), group=group)
        dev = self._keys.device
        longest = max(max(n for n, _ in lens), 1)
        mine_k = torch.zeros((self.n_classes, longest), device=dev, dtype=torch.int32)
        mine_s = torch.zeros((self.n_classes, longest), device=dev, dtype=torch.uint8)
        mine_k[:, :self.n].copy_(self._keys[:, :self.n])
        mine_s[:, :self.n].copy_(self._state[:, :self.n])
        all_k = [torch.empty_like(mine_k) for _ in range(world)]
        all_s = [torch.empty_like(mine_s) for _ in range(world)]
        loss = [torch.empty_like(self._loss_sum) for _ in range(world)]
        dist.all_gather(all_k, mine_k, group=group)
        dist.all_gather(all_s, mine_s, group=group)
        dist.all_gather(loss, self._loss_sum, group=group)
        total = sum(n for n, _ in lens)
        if total == 0:                        # nothing anywhere: one excluded column, n = 0
            keys, state = mine_k, mine_s
        else:
            keys = torch.cat([k[:, :n] for k, (n, _) in zip(all_k, lens)], dim=1).contiguous()
            state = torch.cat([s[:, :n] for s, (n, _) in zip(all_s, lens)], dim=1).contiguous()
        return keys, state, total, torch.stack(loss).sum(0), sum(b for _, b in lens)

    def compute(self, process_group=None):
        """-> dict of device tensors.  Per class [C]: ``ap``, ``auc`` (float64), ``n_pos``, ``n_neg``, ``auc_num`` (int64).  Scalars:
        ``mAP``, ``mAUC`` (plain means: NaN when any class is NaN, as np.mean in the reference), ``val_loss`` (mean over the batches
        of the per-batch BCE means), ``n``.  Nothing is synchronised here.  process_group (torch.distributed.group.WORLD or a
        subgroup): the ranks' samples are concatenated in rank order first and every rank gets the same result."""
        if self._keys is None:                # an epoch without a batch: the current device
            if not torch.cuda.is_available():
                raise _lib.PasstAmdError("passt_amd kernels need a CUDA/HIP device (no CPU fallback)")
            self._reserve(torch.device("cuda", torch.cuda.current_device()), 0)
        if process_group is not None:
            keys, state, n, loss_sum, n_batches = self._gathered(process_group)
            ws = None
        else:
            keys, state, n, loss_sum, n_batches = self._keys, self._state, self.n, self._loss_sum, self.n_batches
            if self._ws is None:
                self._ws = torch.empty(_lib.load().pa_eval_ws_bytes(self.n_classes, self.capacity), device=keys.device, dtype=torch.uint8)
            ws = self._ws
        n_pos, n_neg, auc_num, ap, auc = ops.eval_rank(keys, state, n, ws=ws)
        dev = keys.device
        if self._mode == _lib.EVAL_SIGMOID and n_batches > 0:
            val_loss = (loss_sum / n_batches).reshape(())
        else:
            val_loss = torch.full((), float("nan"), device=dev, dtype=torch.float32)
        return {"ap": ap, "auc": auc, "n_pos": n_pos, "n_neg": n_neg, "auc_num": auc_num, "mAP": ap.mean(), "mAUC": auc.mean(),
                "val_loss": val_loss, "n": torch.full((), n, device=dev, dtype=torch.int64)}

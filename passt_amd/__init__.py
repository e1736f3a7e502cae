"""passt_amd -- the kkoutini/PaSST training hot path, hand-written for MI355X (gfx950).

Public surface mirrors the reference's two model modules:
  passt_amd.passt       <-> models/passt.py       (PaSST, get_model, get_model_passt, ...)
  passt_amd.preprocess  <-> models/preprocess.py  (AugmentMelSTFT)
plus the caller glue of ex_audioset.py's training step (passt_amd.train) and the data-parallel
gradient reducer (passt_amd.ddp).  All compute goes through libpasst_amd.so (include/passt_amd.h).
"""
from .passt import PaSST, get_model, get_model_passt, get_ensemble_model, EnsembelerModel, Windows, window_geometry  # noqa: F401
from .passt import attn_drop_rates  # noqa: F401     (per block: t = round(256 p) of blocks[i].attn.attn_drop.p in training mode)
from .ops import attn_drop_mask  # noqa: F401         (the attention-dropout keep mask of a seed, restated on the CPU)
from .preprocess import AugmentMelSTFT  # noqa: F401
from . import metrics  # noqa: F401     (passt_amd.metrics.EvalAccumulator: validation mAP / ROC-AUC on the device)
from . import windows  # noqa: F401     (passt_amd.windows.tag: waveform -> front end once -> PaSST.forward_windows)

__version__ = "0.1.0"

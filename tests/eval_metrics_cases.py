"""Cases and the NumPy restatement for the validation-metric kernels (pa_eval_append / pa_eval_rank).

The inputs live in tests/golden/eval_metrics.npz (made by tests/golden/make_eval_metrics_golden.py): one [1000][65] block of
logits (int16 / 4096: within +-8, exactly representable in f32), a target bit and a mask bit per element.  Every case is a prefix
(n samples, C classes) of that block seen through one content kind; the expected AP / AUC of every (kind, n, C) come from
scikit-learn and are stored next to the inputs.  restate() is the sort-free formula of the kernels in NumPy: integer counts, one
f64 division per positive, sums in index order."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")
N_MAX, C_MAX, SEED = 1000, 65, 20264
NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
CS = (1, 3, 20, 65)
BS = (1, 7, 20, 64)              # 20 = the reference's validation batch
KINDS = ("random", "ties8", "equal", "one_pos_first", "one_pos_last", "degenerate", "masked", "denormal", "nan", "dense")
SIGMOID_C = 20                   # the sigmoid-mode case: all 1000 samples of the first 20 classes


def batch_size(n, C):
    """the append batch of case (n, C): every B meets every alignment of n0 over the grid of cases"""
    return BS[(NS.index(n) + CS.index(C)) % len(BS)]


def make_inputs():
    """-> logits_i16 [N][C] int16, flags [N][C] uint8 (bit 0: target, bit 1: mask valid).  About 6 % positives, 60 % valid."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    logits = rng.integers(-32768, 32768, size=(N_MAX, C_MAX), dtype=np.int64)
    # Sigmoid mode is compared against an f32 sigmoid made by ANOTHER exp (torch's on the CPU; the kernel's).  Two good expf
    # implementations differ only where exp(-z) lies next to a rounding boundary of f32, so logits whose exp(-z) is within 0.02 ulp
    # of one (4 % of the grid) are moved to the next grid value: every expf with an error below 0.52 ulp then returns the same
    # float, and the sigmoids built from it with IEEE add and divide are equal bit for bit.
    grid = np.arange(-32768, 32768, dtype=np.int64)
    e = np.exp(-(grid.astype(np.float64) / 4096.0))
    frac = e / np.spacing(e.astype(np.float32)).astype(np.float64)
    frac = np.abs(frac - np.floor(frac) - 0.5)
    allowed = grid[frac > 0.02]
    logits = allowed[np.minimum(np.searchsorted(allowed, logits), len(allowed) - 1)].astype(np.int16)
    target = rng.random((N_MAX, C_MAX)) < 0.06
    target[:2] = [[c % 2 == 0 for c in range(C_MAX)], [c % 2 == 1 for c in range(C_MAX)]]     # both labels present from n = 2 on
    mask = rng.random((N_MAX, C_MAX)) < 0.6
    return logits, (target.astype(np.uint8) | (mask.astype(np.uint8) << 1))


def base(inputs):
    logits = inputs["logits_i16"].astype(np.float32) / np.float32(4096.0)
    return logits, (inputs["flags"] & 1).astype(np.float32), ((inputs["flags"] >> 1) & 1).astype(np.float32)


def case(inputs, kind, n, C):
    """-> scores [n][C] f32, target [n][C] f32, mask [n][C] f32 or None"""
    logits, target, mask = base(inputs)
    s, t, m = logits[:n, :C].copy(), target[:n, :C].copy(), None
    if kind == "ties8":
        s = np.floor((s + np.float32(8.0)) / np.float32(2.0)).astype(np.float32)              # 8 levels: heavy ties
    elif kind == "equal":
        s[:] = np.float32(0.25)
    elif kind == "one_pos_first":
        t[:] = 0
        t[0] = 1
    elif kind == "one_pos_last":
        t[:] = 0
        t[n - 1] = 1
    elif kind == "degenerate":
        t[:, 0] = 0                                                       # a class without positives
        if C > 1:
            t[:, 1] = 1                                                   # and one without negatives
    elif kind == "masked":
        m = mask[:n, :C].copy()
        m[t[:, C - 1] > 0.5, C - 1] = 0                                   # the last class's positives are all masked out
    elif kind == "denormal":
        # +-0 and the f32 denormals around them: distinct denormals must not tie, -0 must tie with +0
        q = (inputs["logits_i16"][:n, :C].astype(np.int64) & 7)           # 0..7
        bits = np.array([0x80000003, 0x80000002, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x00000002, 0x00000003],
                        dtype=np.uint32)
        s = bits[q].view(np.float32)
    elif kind == "nan":
        s[n // 2, C - 1] = np.float32("nan")
    elif kind == "dense":
        t = mask[:n, :C].copy()                                           # 60 % positives: several 256-positive tiles per class
    elif kind != "random":
        raise ValueError(kind)
    return np.ascontiguousarray(s), np.ascontiguousarray(t), m


def large_case(n=2600, C=3):
    """Past the fixture's sizes, for the paths N <= 1000 cannot reach: more than 1024 positives AND more than 1024 negatives per
    class (the compared keys pass through LDS 1024 at a time), 200 score levels, a 90 % mask.  Judged against restate()."""
    rng = np.random.Generator(np.random.PCG64(SEED + 1))
    s = (rng.integers(0, 200, size=(n, C)).astype(np.float32) - np.float32(100.0)) / np.float32(16.0)
    t = (rng.random((n, C)) < 0.5).astype(np.float32)
    m = (rng.random((n, C)) < 0.9).astype(np.float32)
    return s, t, m


def expected(inputs, kind, n, C):
    """the stored scikit-learn values of one case: (ap [C], auc [C]) float64.  ap_<kind> / auc_<kind> hold the cases back to back,
    n-major, in the order of NS and CS."""
    off = 0
    for nn in NS:
        for cc in CS:
            if (nn, cc) == (n, C):
                return inputs["ap_" + kind][off:off + C], inputs["auc_" + kind][off:off + C]
            off += cc
    raise KeyError((n, C))


def score_key(s):
    """the kernels' order-preserving u32 key of an f32 score (-0 folded onto +0)"""
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    neg = (b & 0x80000000) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_score(k):
    """inverse of score_key"""
    k = np.asarray(k, dtype=np.uint32)
    b = np.where((k & 0x80000000) != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32)
    return b.view(np.float32)


def restate(scores, target, mask=None):
    """The kernels' arithmetic in NumPy -> dict(n_pos, n_neg, auc_num: int64 [C]; ap, auc: float64 [C]).  Compares integer keys
    only; a valid NaN-scored sample is in neither count and makes its class's ap and auc NaN."""
    n, C = scores.shape
    keys = score_key(scores).astype(np.int64)
    isnan = np.isnan(scores)
    valid = np.ones((n, C), bool) if mask is None else mask > 0.5
    out = dict(n_pos=np.zeros(C, np.int64), n_neg=np.zeros(C, np.int64), auc_num=np.zeros(C, np.int64), ap=np.zeros(C, np.float64),
               auc=np.zeros(C, np.float64))
    for c in range(C):
        ok = valid[:, c] & ~isnan[:, c]
        pos = keys[ok & (target[:, c] > 0.5), c]
        neg = np.sort(keys[ok & ~(target[:, c] > 0.5), c])
        pos_sorted = np.sort(pos)
        P, Nn = len(pos), len(neg)
        gep = P - np.searchsorted(pos_sorted, pos, side="left")
        gen = Nn - np.searchsorted(neg, pos, side="left")
        gtn = Nn - np.searchsorted(neg, pos, side="right")
        num = int(np.sum(2 * (Nn - gen) + (gen - gtn), dtype=np.int64))
        acc = 0.0
        for r in gep.astype(np.float64) / (gep.astype(np.float64) + gen.astype(np.float64)):       # index order
            acc += r
        bad = bool((valid[:, c] & isnan[:, c]).any())
        out["n_pos"][c], out["n_neg"][c], out["auc_num"][c] = P, Nn, num
        out["ap"][c] = np.nan if bad else (acc / P if P > 0 else 0.0)
        out["auc"][c] = np.nan if (bad or P == 0 or Nn == 0) else num / (2.0 * P * Nn)
    return out


def sklearn_expected(scores, target, mask=None):
    """scikit-learn called as the reference calls it: average=None on the whole matrix (ex_audioset.py:256-262), or one column
    at a time with sample_weight=mask (ex_openmic.py:241-248).  A column holding a NaN score (scikit-learn refuses it) is NaN in
    both and is left out of the call."""
    import warnings

    from sklearn import metrics
    n, C = scores.shape
    ap, auc = np.full(C, np.nan), np.full(C, np.nan)
    cols = [c for c in range(C) if not np.isnan(scores[:, c]).any()]
    if not cols:
        return ap, auc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if mask is None:
            ap[cols] = np.atleast_1d(metrics.average_precision_score(target[:, cols], scores[:, cols], average=None))
            try:
                auc[cols] = np.atleast_1d(metrics.roc_auc_score(target[:, cols], scores[:, cols], average=None))
            except ValueError:                # one label in a single-column (binary) call: the reference's np.nan (ex_audioset.py:263)
                pass
        else:
            for c in cols:
                if not (mask[:, c] > 0.5).any():          # no valid sample at all: scikit-learn 1.7.2 fails inside (IndexError); the
                    ap[c] = 0.0                           # kernels' P = 0 convention stands in
                    continue
                ap[c] = metrics.average_precision_score(target[:, c], scores[:, c], sample_weight=mask[:, c])
                try:
                    auc[c] = metrics.roc_auc_score(target[:, c], scores[:, c], sample_weight=mask[:, c])
                except ValueError:
                    pass
    return ap, auc


def sigmoid_sweep():
    """sorted logits over [-100, 100]: +-0, the saturation regions of the f32 sigmoid, a dense middle"""
    z = np.concatenate([np.linspace(-100, 100, 2001), np.linspace(-20, 20, 4001), np.linspace(-1, 1, 2001),
                        [-0.0, 0.0, -88.8, 88.8, -103.0, 103.0, 16.7, 17.4, -16.7, -17.4]]).astype(np.float32)
    z = np.unique(z)                          # sorted; -0.0 and 0.0 collapse to one entry, so both are put back side by side
    i = int(np.searchsorted(z, 0.0))
    return np.concatenate([z[:i], np.array([-0.0, 0.0], np.float32), z[i + 1:]]).astype(np.float32)


def ulp_error(s32, z):
    """error of the f32 values s32 against the float64 sigmoid of z, in units of the f32 spacing at the exact value"""
    exact = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    ulp = np.spacing(np.maximum(exact, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    return np.abs(s32.astype(np.float64) - exact) / ulp

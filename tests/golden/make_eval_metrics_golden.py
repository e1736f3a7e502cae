"""Writes tests/golden/eval_metrics.npz: the inputs of tests/eval_metrics_cases.py and, for every (content kind, n, C) of its
grid, the per-class average precision and ROC-AUC scikit-learn returns when it is called the way the reference's experiment
files call it (average=None on the matrix; one column at a time with sample_weight=mask for the masked kind).  Arrays only.

    python tests/golden/make_eval_metrics_golden.py [out.npz]

The file is reproducible bit for bit: seeded NumPy generators, members written uncompressed in a fixed order with a fixed
timestamp.  The sigmoid-mode members (the f32 torch.sigmoid of the first 20 classes' logits on the CPU, and scikit-learn on
those) are made with torch's plain scalar kernels (ATEN_CPU_CAPABILITY=default, set before torch is imported), so that the
vector width of the CPU at hand does not enter.  Needs scikit-learn (1.7.2 made the committed file)."""
import io
import os
import sys
import zipfile

os.environ["ATEN_CPU_CAPABILITY"] = "default"

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import eval_metrics_cases as K  # noqa: E402


def build():
    import torch
    logits_i16, flags = K.make_inputs()
    out = {"logits_i16": logits_i16, "flags": flags}
    for kind in K.KINDS:
        aps, aucs = [], []
        for n in K.NS:
            for C in K.CS:
                s, t, m = K.case(out, kind, n, C)
                ap, auc = K.sklearn_expected(s, t, m)
                aps.append(ap)
                aucs.append(auc)
        out["ap_" + kind], out["auc_" + kind] = np.concatenate(aps), np.concatenate(aucs)
    # sigmoid mode: what the reference ranks (ex_audioset.py:238) on the CPU, and scikit-learn on it
    logits, target, _ = K.base(out)
    sig = torch.sigmoid(torch.from_numpy(logits[:, :K.SIGMOID_C].copy())).numpy()
    out["sigmoid_f32"] = sig
    out["ap_sigmoid"], out["auc_sigmoid"] = K.sklearn_expected(sig, target[:, :K.SIGMOID_C])
    return out


def write(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    write(sys.argv[1] if len(sys.argv) > 1 else K.GOLDEN, build())

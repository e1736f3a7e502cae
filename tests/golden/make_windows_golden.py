"""Fixture of sliding-window inference (PaSST.forward_windows): tests/golden/windows_eval.npz, from the real reference implementation
(kkoutini/PaSST, imported read-only through oracle/ref_import.py exactly as make_varlen_golden.py does; none of its text is here).

The reference has no window entry: its answer to a recording longer than the time embedding is to cut it.  What forward_windows
promises per window is what the reference returns for that window ALONE, so that is what is recorded: the reference ``PaSST.eval()``
run window by window at batch size 1 on the slices x[b:b+1, :, :, start:start+length], the windows enumerated by the brute-force rule
of tests/windows_cases.py (not by the code under test).  Weights and inputs are oracle/detgen.py streams, so the tests regenerate
them instead of storing them.  Arrays only:

    <case>.<hop>.<tail>.logits (W, n_classes)   .features (W, D)   .start / .length (W,)   .offsets (B + 1,)

    python tests/golden/make_windows_golden.py        (CPU, about a minute)
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import detgen, ref_import  # noqa: E402
from oracle import passt_oracle as O   # noqa: E402
from tests import windows_cases as W   # noqa: E402
from tests.golden import make_golden as G  # noqa: E402
from tests.golden import make_varlen_golden as V  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    # the small model (time embedding of 25 columns, windows of 24): every recording shape of the window rule
    "small": dict(cfg=O.make_cfg(**G.SMALL), seed=51, recordings=W.RECORDINGS, window=W.WINDOW, rules=[(100, "align"), (100, "short"),
                                                                                                       (37, "align"), (37, "short")]),
    # the ragged fixture's d768 model: windows that fill its time embedding exactly (99 columns)
    "d768": dict(cfg=V.MODELS["d768"]["cfg"], seed=V.MODELS["d768"]["seed"], recordings=[2400, 998, 1500], window=998,
                 rules=[(499, "align"), (499, "short")]),
}


def model_input(case):
    """(B, 1, n_mels, longest recording) -- recording b is its first recordings[b] frames"""
    return detgen.uniform(case["seed"], "x", (len(case["recordings"]), 1, case["cfg"]["img_size"][0], max(case["recordings"])), -1.5, 1.5)


def windows_of(case, hop, tail):
    """(offsets, [(recording, start, length)]) by the brute-force rule"""
    P = case["cfg"]["patch"]
    offsets, wins = [0], []
    for b, n in enumerate(case["recordings"]):
        wins += [(b, s, m) for s, m in W.brute_windows(n, case["window"], hop, tail, P)[0]]
        offsets.append(len(wins))
    return offsets, wins


def main():
    assert ref_import.reference_available(), "needs the reference checkout"
    out = {}
    for name, case in CASES.items():
        m = ref_import.build_reference_passt(case["cfg"], detgen.passt_state_dict(case["cfg"], case["seed"]))
        m.eval()
        x = model_input(case)
        done = {}
        for hop, tail in case["rules"]:
            offsets, wins = windows_of(case, hop, tail)
            for key in wins:
                if key not in done:
                    b, s, n = key
                    with torch.no_grad(), warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        logits, feat = ref_import.run_silently(m, torch.from_numpy(np.ascontiguousarray(x[b:b + 1, :, :, s:s + n])))
                    done[key] = (logits.numpy()[0], feat.numpy()[0])
            k = f"{name}.{hop}.{tail}"
            out[k + ".logits"], out[k + ".features"] = np.stack([done[w][0] for w in wins]), np.stack([done[w][1] for w in wins])
            out[k + ".start"], out[k + ".length"] = np.array([w[1] for w in wins], np.int64), np.array([w[2] for w in wins], np.int64)
            out[k + ".offsets"] = np.array(offsets, np.int64)
            print(k, len(wins), "windows, logits absmax", float(np.abs(out[k + ".logits"]).max()))
    np.savez_compressed(os.path.join(HERE, "windows_eval.npz"), **out)


if __name__ == "__main__":
    main()

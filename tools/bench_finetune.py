#!/usr/bin/env python
"""Cost of a fine-tuning step as a function of what is trainable, config-#2 shapes: passt_s (768 / 12 / 12, stride 10, 128 mel bands,
998 frames, s_patchout_t = 40, s_patchout_f = 4 -> 474 tokens), B = 64, bf16, one GPU.  One JSON line per measurement.

  cases   all     every parameter trainable
          last4   blocks 8 .. 11 + final norm + head
          head    final norm + head (a linear probe on the pooled tokens)
  paths   trainstep   passt_amd.train.TrainStep, eager (mixup + forward + BCE + backward + per-bucket AdamW)
          autograd    net(x); BCE; loss.backward(); passt_amd.optim.AdamW over the trainable parameters; zero_grad

Per case and path: the step time (median over --reps blocks of --iters steps, device events around a block and a synchronise behind
it, every block's value alongside), the library calls made while the backward runs (every ``pa_*`` call is counted at its status
check; TrainStep's per-bucket optimizer launches ride inside its backward and are counted with it) and
torch.cuda.max_memory_allocated over the timed steps.  A path the build under test refuses (a TrainStep on frozen parameters before
partial fine-tuning existed) is reported as such, so the same file measures an older commit as the baseline.

    python tools/bench_finetune.py --out profiles/finetune.txt --tag this
"""
import argparse
import json
import os
import statistics
import sys
import warnings

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
B, TOKENS, D, DEPTH = 64, 474, 768, 12
CASES = {
    "all": lambda n: True,
    "last4": lambda n: n.startswith(("blocks.8.", "blocks.9.", "blocks.10.", "blocks.11.", "norm.", "head.")),
    "head": lambda n: n.startswith(("norm.", "head.")),
}


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


class CallCounter:
    """counts the library calls made while ``active`` (ops.check sees the status of every one)"""

    def __init__(self, ops):
        self.n, self.active, self._check = 0, False, ops.check
        ops.check = self

    def __call__(self, rc, what=""):
        self.n += self.active
        return self._check(rc, what)


def build(case):
    import torch

    import passt_amd
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.PaSST(s_patchout_t=40, s_patchout_f=4, img_size=(128, 998), stride=10, num_classes=527, embed_dim=D, depth=DEPTH,
                              num_heads=12, distilled=True).cuda().train()
    net.precision = "bf16"
    for n, p in net.named_parameters():
        p.requires_grad_(bool(CASES[case](n)))
    return net


def measure(a, case, path, counter):
    import numpy as np
    import torch

    from passt_amd import optim as pa_optim
    from passt_amd import train
    net = build(case)
    x = torch.randn(B, 1, 128, 998, device="cuda")
    y = (torch.rand(B, 527, device="cuda") < 0.05).float()
    np.random.seed(0)
    if path == "trainstep":
        ts = train.TrainStep(net, None, lr=2e-5, weight_decay=1e-4, use_mixup=True, loss="bce")
        real_backward = train.passt_backward

        def counted_backward(*args, **kw):
            counter.active = True
            try:
                return real_backward(*args, **kw)
            finally:
                counter.active = False
        train.passt_backward = counted_backward

        def step():
            ts.step(x, y)
    else:
        opt = pa_optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=2e-5, weight_decay=1e-4)

        def step():
            logits, _ = net(x)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y)
            counter.active = True
            loss.backward()
            counter.active = False
            opt.step()
            opt.zero_grad()

    def block(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            block(a.warmup)
            counter.n = 0
            step()
            calls = counter.n
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ms = [round(block(a.iters), 4) for _ in range(a.reps)]
        peak = torch.cuda.max_memory_allocated()
    finally:
        if path == "trainstep":
            train.passt_backward = real_backward
            ts.close()
    return {"ms_per_step": statistics.median(ms), "blocks_ms": ms, "backward_calls": calls, "max_memory_allocated_MiB": round(peak / 2 ** 20, 1),
            "trainable_params": sum(p.numel() for p in net.parameters() if p.requires_grad)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="all,last4,head")
    ap.add_argument("--paths", default="trainstep,autograd")
    ap.add_argument("--tag", default="", help="names the build under test in every line (e.g. the commit)")
    ap.add_argument("--out", default="", help="append the result lines to this file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune.py measures on the GPU: no device found")
    from passt_amd import ops
    counter = CallCounter(ops)
    for case in a.cases.split(","):
        for path in a.paths.split(","):
            rec = {"bench": "finetune_step", "build": a.tag, "case": case, "path": path, "precision": "bf16", "batch": B, "tokens": TOKENS,
                   "steps_per_block": a.iters}
            try:
                rec.update(measure(a, case, path, counter))
            except NotImplementedError as e:
                rec["unsupported"] = str(e)[:120]
            emit(a, rec)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

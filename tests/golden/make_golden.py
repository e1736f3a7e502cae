"""Generate the golden fixtures in this directory by running the REAL reference
(kkoutini/PaSST, imported read-only from /root/reference through oracle/ref_import.py).

    python tests/golden/make_golden.py          # rewrites tests/golden/*.npz
    python tests/golden/make_golden.py live     # only the live_*.npz the CPU pinning tests compare with

Only outputs are stored; inputs/weights are regenerated bit-exactly by oracle/detgen.py.
The GPU box has no /root/reference -- the `-m gpu` parity tests compare the HIP path with
these committed files (and with the oracle, itself pinned to these files by the CPU suite).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import detgen, ref_import  # noqa: E402
from oracle import passt_oracle as O   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

# ---- shared case definitions (imported by the tests too) ---------------------------------
SMALL = dict(embed_dim=128, depth=2, num_heads=2, num_classes=37, img_size=(128, 250),
             stride=(10, 10))
CASES = {
    # conv grid is 12x24 but the embedding grid is 12x25 -> exercises the time-pos-embed crop
    "model_small_eval": dict(cfg=O.make_cfg(**SMALL), B=2, T=250, training=False, seed=11),
    "model_small_train": dict(cfg=O.make_cfg(**SMALL, s_patchout_t=6, s_patchout_f=3, u_patchout=5),
                              B=3, T=250, training=True, seed=12, torch_seed=1234),
    # structured patchout only, 3 heads, stride 16 grid
    "model_s16_train": dict(cfg=O.make_cfg(embed_dim=192, depth=1, num_heads=3, num_classes=50,
                                           img_size=(128, 320), stride=(16, 16),
                                           s_patchout_t=5, s_patchout_f=2),
                            B=2, T=320, training=True, seed=13, torch_seed=77),
    # BASELINE config #1 at full width/depth: passt_s_swa_p16_128_ap476, eval, no patchout
    "model_passt_s_eval": dict(cfg=O.make_cfg(), B=1, T=998, training=False, seed=14),
}
# Full-size cases (r02): the headline training configuration at real depth (prefix-only tail and batched weight gradients
# active), BASELINE config #4 (1024/24/16, unstructured patchout 400) and the 20 s / 30 s inference archs.  Gradients
# of these are stored COMPACT (1024 evenly spaced entries + L2 norm per tensor): the full sets would be 0.3-1.2 GB.
BIG_CASES = {
    "model_passt_s_train_full": dict(cfg=O.make_cfg(s_patchout_t=40, s_patchout_f=4), B=2, T=998, training=True,
                                     seed=15, torch_seed=4321, compact=True),
    "model_vitl_u400_train": dict(cfg=O.make_cfg(embed_dim=1024, depth=24, num_heads=16, u_patchout=400), B=1, T=998,
                                  training=True, seed=16, torch_seed=99, compact=True),
    # passt_s_f128_20sec_p16_s10_ap474 / passt_s_f128_30sec_p16_s10_ap473 (models/passt.py:990-1003): N = 2390 / 3590
    "model_passt_s_20s_eval": dict(cfg=O.make_cfg(img_size=(128, 2000)), B=1, T=2000, training=False, seed=17),
    "model_passt_s_30s_eval": dict(cfg=O.make_cfg(img_size=(128, 3000)), B=1, T=3000, training=False, seed=18),
    # r03: BASELINE config #5 at real depth -- ESC-50 fine-tune (ex_esc50.py:60): n_classes=50, 5 s clips (500 frames into a
    # 998-frame model: random time-pos-embed offset), s_patchout_t=10, s_patchout_f=3 => 353 tokens
    "model_esc50_train_full": dict(cfg=O.make_cfg(num_classes=50, s_patchout_t=10, s_patchout_f=3), B=2, T=500, training=True,
                                   seed=19, torch_seed=555, compact=True),
}
# r05: BASELINE config #2 EXACTLY, at the benchmarked batch (768/12/12, s_patchout t = 40 / f = 4 => 474 tokens, B = 64,
# M = 30 336 token rows: 237 row tiles, persistent rounds, 7-slice batched weight gradients, XCD mapping) -- once on a
# random spectrogram and once on the constant batch the reference's own speed test uses (x = ones(B,1,128,998), target =
# ones(B,527): ex_audioset.py:384-385).  ~1.5 min of CPU each for the real reference; gradients stored compact.
B64_CASES = {
    "model_passt_s_train_b64": dict(cfg=O.make_cfg(s_patchout_t=40, s_patchout_f=4), B=64, T=998, training=True,
                                    seed=25, torch_seed=6464, compact=True),
    "model_passt_s_train_b64_ones": dict(cfg=O.make_cfg(s_patchout_t=40, s_patchout_f=4), B=64, T=998, training=True,
                                         seed=26, torch_seed=6465, compact=True, inputs="ones"),
}
# r06: the two remaining bench configurations at THEIR benchmarked batch.  BASELINE config #4 exactly (1024/24/16, u_patchout
# 400 => 790 tokens, B = 32: M = 25 280 token rows; the reference runs with its blocks under torch.utils.checkpoint -- the
# arithmetic is the same, recomputed, and 24 blocks of saved (32,16,790,790) score tensors would not fit this container's
# 64 GB) and config #5 exactly (ESC-50 fine-tune, ex_esc50.py:40,60: n_classes 50, B = 12, 500 frames into the 998-frame model,
# s_patchout_t 10 / f 3 => 353 tokens, M = 4 236: the split-K path of every [M, 768] GEMM and the two-kernel attention
# backward; class-index targets and the CE loss of ex_esc50.py:166-168).
BENCH_CASES = {
    "model_vitl_u400_train_b32": dict(cfg=O.make_cfg(embed_dim=1024, depth=24, num_heads=16, u_patchout=400), B=32, T=998,
                                      training=True, seed=27, torch_seed=3232, compact=True, checkpoint=True),
    "model_esc50_train_b12": dict(cfg=O.make_cfg(num_classes=50, s_patchout_t=10, s_patchout_f=3), B=12, T=500, training=True,
                                  seed=28, torch_seed=1212, compact=True, loss="ce"),
}
FRONTEND_CASES = {
    "frontend_eval": dict(B=2, L=32000, training=False, seed=21,
                          kw=dict(fmin_aug_range=10, fmax_aug_range=2000)),
    "frontend_eval_10s": dict(B=1, L=320000, training=False, seed=22,
                              kw=dict(fmin_aug_range=10, fmax_aug_range=2000)),
    "frontend_train": dict(B=2, L=48000, training=True, seed=23, torch_seed=99,
                           kw=dict(fmin_aug_range=10, fmax_aug_range=2000, freqm=48, timem=40)),
    "frontend_esc50": dict(B=2, L=16000, training=False, seed=24,
                           kw=dict(fmin_aug_range=10, fmax_aug_range=2000, freqm=48, timem=80)),
}


def model_inputs(case):
    cfg, B, T = case["cfg"], case["B"], case["T"]
    if case.get("inputs") == "ones":                     # model_speed_test's batch (ex_audioset.py:384-385)
        return (np.ones((B, 1, cfg["img_size"][0], T), np.float32), np.ones((B, cfg["num_classes"]), np.float32))
    x = detgen.uniform(case["seed"], "x", (B, 1, cfg["img_size"][0], T), -1.5, 1.5)
    if case.get("loss") == "ce":                         # class ids (ex_esc50.py:166)
        return x, np.floor(detgen.uniform(case["seed"], "y", (B,), 0.0, float(cfg["num_classes"]))).astype(np.int64).clip(0, cfg["num_classes"] - 1)
    y = (detgen.uniform(case["seed"], "y", (B, cfg["num_classes"]), 0.0, 1.0) < 0.1).astype(np.float32)
    return x, y


def frontend_inputs(case):
    w = detgen.uniform(case["seed"], "wave", (case["B"], case["L"]), -1.0, 1.0)
    # a little structure so the spectrum is not flat: amplitude-modulated noise + a chirp
    n = np.arange(case["L"], dtype=np.float64)
    chirp = 0.3 * np.sin(2 * np.pi * (200.0 + 0.05 * n) * n / 32000.0)
    return (0.1 * w * (1.0 + 0.5 * np.sin(n / 977.0)) + chirp).astype(np.float32)


def subsample(g, compact=False):
    """Full tensor for small ones; every 7th element (compact: 1024 evenly spaced elements) + L2 norm for large ones."""
    flat = np.ascontiguousarray(g).reshape(-1)
    if flat.size <= 4096:
        return flat.copy(), float(np.linalg.norm(flat.astype(np.float64)))
    if compact:
        idx = np.linspace(0, flat.size - 1, 1024).astype(np.int64)
        return flat[idx].copy(), float(np.linalg.norm(flat.astype(np.float64)))
    return flat[::7].copy(), float(np.linalg.norm(flat.astype(np.float64)))


def gen_model_case(name, case):
    cfg = case["cfg"]
    sd = detgen.passt_state_dict(cfg, case["seed"])
    x, y = model_inputs(case)
    m = ref_import.build_reference_passt(cfg, sd)
    m.train(case["training"])
    out = {}
    if case.get("checkpoint"):
        # the reference's own Block.forward, run under activation checkpointing (same arithmetic, recomputed in the backward)
        from torch.utils.checkpoint import checkpoint
        for blk in m.blocks:
            blk.forward = (lambda x_, f=blk.forward: checkpoint(f, x_, use_reentrant=False))
    if case["training"]:
        torch.manual_seed(case["torch_seed"])
        logits, feat = ref_import.run_silently(m, torch.from_numpy(x))
        if case.get("loss") == "ce":
            loss = torch.nn.functional.cross_entropy(logits, torch.from_numpy(y), reduction="none").mean()   # ex_esc50.py:166-167
        else:
            loss = torch.nn.functional.binary_cross_entropy_with_logits(
                logits, torch.from_numpy(y), reduction="none").mean()          # ex_audioset.py:184-186
        loss.backward()
        out["loss"] = np.float32(loss.item())
        for k, p in m.named_parameters():
            if p.grad is None:
                out["gradnone." + k] = np.zeros(0, np.float32)
            else:
                s, nrm = subsample(p.grad.numpy(), case.get("compact", False))
                out["grad." + k] = s
                out["gradnorm." + k] = np.float64(nrm)
        # replay the index draws (same seed, same call order) so the fixture holds them
        torch.manual_seed(case["torch_seed"])
        Fd = (cfg["img_size"][0] - cfg["patch"]) // cfg["stride"][0] + 1
        Td = (case["T"] - cfg["patch"]) // cfg["stride"][1] + 1
        d = O.draw_patchout(cfg, Fd, Td, True)
        out["toff"] = np.int64(d["toff"])
        for k in ("idx_t", "idx_f", "idx_u"):
            out[k] = d[k].numpy() if d[k] is not None else np.zeros(0, np.int64)
    else:
        with torch.no_grad():
            logits, feat = ref_import.run_silently(m, torch.from_numpy(x))
    out["logits"] = logits.detach().numpy()
    out["features"] = feat.detach().numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(name, "logits", out["logits"].shape, "absmax", float(np.abs(out["logits"]).max()))


def gen_frontend_case(name, case):
    _, ref_pre = ref_import.load_reference()
    wave = frontend_inputs(case)
    mel = ref_import.run_silently(ref_pre.AugmentMelSTFT, **case["kw"])
    mel.train(case["training"])
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            out = mel(torch.from_numpy(wave))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), mel=out.numpy())
    print(name, tuple(out.shape), "range", float(out.min()), float(out.max()))


WAVE_CASE = dict(seed=31, L=4000, lens=[4000, 2600, 5200, 4000, 3999], gain_db=[-7, 0, 3, 6, -2],
                 shift=[0, 17, -50, 50, -1], partner=[2, -1, 0, 4, 3], lam=[0.31, 0.5, 0.77, 0.5, 0.05])


def wave_inputs(case):
    return [0.2 * detgen.uniform(case["seed"], f"raw{i}", (n,), -1.0, 1.0) + 0.05 * (i - 2) for i, n in enumerate(case["lens"])]


def gen_wave_case():
    """Runs the REAL bodies of pad_or_truncate / pydub_augment / get_roll_func / MixupDataset from
    audioset/dataset.py (extracted with ast: the module needs av, h5py, librosa to import) on WAVE_CASE."""
    import ast
    src = open(os.path.join(ref_import.REFERENCE_ROOT, "audioset", "dataset.py")).read()
    keep = []
    for node in ast.parse(src).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in ("pad_or_truncate", "pydub_augment",
                                                                              "get_roll_func", "MixupDataset"):
            node.decorator_list = []
            keep.append(node)
    ns = {"np": np, "torch": torch, "TorchDataset": object}
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        exec(compile(ast.Module(body=keep, type_ignores=[]), "<reference audioset/dataset.py>", "exec"), ns)
    c = WAVE_CASE
    raws = wave_inputs(c)

    class Items:                                      # what AudioSetDataset.__getitem__ + roll_func hand over
        def __len__(self):
            return len(raws)

        def __getitem__(self, i):
            class OneDraw:                            # pydub_augment draws gain with torch.randint(2*7, (1,))
                pass
            saved = torch.randint
            torch.randint = lambda *a, **k: torch.tensor([c["gain_db"][i] + 7])
            try:
                w = ns["pydub_augment"](raws[i], gain_augment=7, ir_augment=0)
            finally:
                torch.randint = saved
            w = ns["pad_or_truncate"](w, c["L"]).reshape(1, -1)
            with contextlib.redirect_stdout(io.StringIO()):
                x, _, y = ns["get_roll_func"](axis=1, shift=c["shift"][i])((w, f"clip{i}", np.eye(len(raws), dtype=np.float32)[i]))
            return x, f"clip{i}", torch.as_tensor(y)

    base = Items()
    with contextlib.redirect_stdout(io.StringIO()):
        mix = ns["MixupDataset"](base, beta=2, rate=0.5)
    out, tgt = [], []
    for b in range(len(raws)):
        s_rand, s_randint, s_beta = torch.rand, torch.randint, np.random.beta
        torch.rand = lambda *a, **k: torch.tensor([0.0 if c["partner"][b] >= 0 else 1.0])
        torch.randint = lambda *a, **k: torch.tensor([max(c["partner"][b], 0)])
        np.random.beta = lambda *a, **k: c["lam"][b]
        try:
            x, _, y = mix[b]
        finally:
            torch.rand, torch.randint, np.random.beta = s_rand, s_randint, s_beta
        out.append(np.asarray(x, np.float32).reshape(-1))
        tgt.append(np.asarray(y, np.float32))
    np.savez_compressed(os.path.join(HERE, "wave_augment.npz"), out=np.stack(out), target=np.stack(tgt))
    print("wave_augment", np.stack(out).shape, float(np.abs(np.stack(out)).max()))


SWA_CASE = dict(seed=31, shapes=[(5, 7), (11,), (2, 3, 4)], max_epochs=12,
                runs=[dict(swa_epoch_start=4, swa_freq=3), dict(swa_epoch_start=0.5, swa_freq=3), dict(swa_epoch_start=1, swa_freq=5)])


def swa_snapshots(case):
    """[max_epochs][n] f32: the network's parameters (flat, parameter order) at the start of every epoch"""
    n = sum(int(np.prod(s)) for s in case["shapes"])
    return np.stack([detgen.uniform(case["seed"], f"epoch{e}", (n,), -1.0, 1.0).astype(np.float32) + 0.1 * e
                     for e in range(case["max_epochs"])])


def gen_swa_case(out_dir=HERE):
    """Runs the REAL helpers/swa_callback.py (StochasticWeightAveraging: setup, on_fit_start, on_train_epoch_start ->
    update_parameters / avg_fn, on_validation_epoch_start) over SWA_CASE's epochs with a stand-in trainer; Lightning's Callback
    base class is stubbed (oracle/ref_import.py), everything the callback computes is its own code."""
    import contextlib, io, warnings
    mod = ref_import.import_reference_file("helpers/swa_callback.py")
    c = SWA_CASE
    snaps = swa_snapshots(c)
    out = {}
    for ri, run in enumerate(c["runs"]):
        net = torch.nn.Module()
        for i, shp in enumerate(c["shapes"]):
            net.register_parameter(f"p{i}", torch.nn.Parameter(torch.zeros(shp)))

        class PlModule(torch.nn.Module):
            device = torch.device("cpu")

        plm = PlModule()
        plm.net = net

        class Trainer:
            pass

        tr = Trainer()
        tr.max_epochs, tr.current_epoch, tr.lr_scheduler_configs = c["max_epochs"], 0, []
        tr.optimizers = [torch.optim.SGD(net.parameters(), lr=0.1)]
        cb = mod.StochasticWeightAveraging(swa_epoch_start=run["swa_epoch_start"], swa_freq=run["swa_freq"])
        avgs, counts, flags = [], [], []
        with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cb.setup(tr, plm, "fit")
            cb.on_fit_start(tr, plm)
            for e in range(c["max_epochs"]):
                tr.current_epoch = e
                off = 0
                with torch.no_grad():
                    for p in net.parameters():
                        p.copy_(torch.from_numpy(snaps[e, off:off + p.numel()].copy()).view(p.shape))
                        off += p.numel()
                cb.on_train_epoch_start(tr, plm)
                cb.on_validation_epoch_start(tr, plm)
                started = hasattr(cb, "n_averaged")
                avgs.append(torch.cat([p.detach().reshape(-1) for p in cb._average_model.parameters()]).numpy().copy()
                            if started else np.zeros(snaps.shape[1], np.float32))
                counts.append(int(cb.n_averaged) if started else 0)
                flags.append(bool(plm.do_swa))
        out[f"run{ri}.avg"], out[f"run{ri}.n_averaged"], out[f"run{ri}.do_swa"] = np.stack(avgs), np.array(counts), np.array(flags)
        print("swa run", ri, run, "updates at", [e for e, f in enumerate(flags) if f], "n_averaged", counts[-1])
    np.savez_compressed(os.path.join(out_dir, "swa_callback.npz"), **out)


# ---- outputs of the reference's own code for the pinning tests that used to import it live (CPU suite) ----------------
# Arrays longer than 4096 entries are stored the way subsample() stores the model gradients above (every 7th entry), those of
# live_geometries.npz as at most GEOMETRY_SAMPLE evenly spaced entries; next to each: the whole array's L2 norm and largest
# magnitude (pin_sample / _pinned_into).
# live_train_step.npz  : the reference PaSST, train mode, one BCE step on model_small_train's geometry (seed 991): logits, features,
#                        every gradient
# live_geometries.npz  : the same for GEOMETRY_CASES (other strides, u_patchout, the 2000-frame model), 4 torch seeds each; a seed
#                        on which the reference raises IndexError (it indexes past its own time cut) is stored as failed
# live_frontend.npz    : the reference AugmentMelSTFT, eval and train mode, on the default STFT and on STFT_CASES
# live_helpers.npz     : helpers/mixup.py's my_mixup draws, helpers/ramp.py's exp_warmup_linear_down values, what
#                        helpers/models_size.py's count_non_zero_params reports for a passt_amd.PaSST, the reference's parameter
#                        names / shapes of a small PaSST
LIVE_TRAIN_STEP = dict(cfg=CASES["model_small_train"]["cfg"], seed=991, torch_seed=5)
GEOMETRY_CASES = [(dict(stride=(12, 12), s_patchout_t=30, s_patchout_f=3), 998),
                  (dict(stride=(20, 20), s_patchout_t=10, s_patchout_f=1), 990),
                  (dict(stride=(10, 16), u_patchout=100), 998),
                  (dict(img_size=(128, 2000), s_patchout_t=80, s_patchout_f=4), 2000),
                  (dict(stride=(20, 20), s_patchout_t=10, s_patchout_f=1), 998)]
GEOMETRY_SEEDS = range(4)
FRONTEND_LIVE = dict(B=2, L=40000, seed=31, torch_seed=3, kw=dict(fmin_aug_range=10, fmax_aug_range=2000))
STFT_CASES = [dict(hopsize=160), dict(hopsize=100), dict(hopsize=500, win_length=1024), dict(win_length=400, n_mels=64),
              dict(hopsize=333, fmin=50.0, fmax=14000)]
STFT_LIVE = dict(B=2, L=24000, seed=32, torch_seed=4, kw=dict(fmin_aug_range=10, fmax_aug_range=2000))
MIXUP_CASES = [(64, 0.3), (12, 0.3), (1, 0.3), (7, 2.0)]
MIXUP_SEEDS = (0, 1, 1234)
RAMP_EPOCHS = list(range(0, 131)) + [0.25, 4.5, 50.5, 99.9]
MODELS_SIZE_SEED = 0
NAMES_CFG = dict(embed_dim=128, depth=2, num_heads=2, num_classes=9, img_size=(128, 100))


def geometry_cfg(kw):
    return O.make_cfg(embed_dim=48, depth=1, num_heads=3, num_classes=11, **kw)


GEOMETRY_SAMPLE = 256


def pin_sample(a, limit=None):
    """The entries of ``a`` a live_*.npz fixture keeps: subsample()'s, or at most ``limit`` evenly spaced ones."""
    flat = np.ascontiguousarray(a).reshape(-1)
    if limit is None or flat.size <= limit:
        return subsample(flat)[0]
    return flat[np.linspace(0, flat.size - 1, limit).astype(np.int64)].copy()


def _pinned_into(out, key, a, limit=None):
    a = np.ascontiguousarray(a, np.float32)
    out[key] = pin_sample(a, limit)
    out[key + ".stats"] = np.array([np.linalg.norm(a.astype(np.float64)), np.abs(a).max() if a.size else 0.0])


def _grads_into(out, prefix, named_params, limit=None):
    """every parameter's gradient, packed: names, has_grad, stats (L2 norm, largest magnitude), and the pin_sample() entries of
    all of them concatenated (samples[offsets[i]:offsets[i + 1]] belongs to names[i])"""
    names, has, stats, samples, offsets = [], [], [], [], [0]
    for k, p in named_params:
        g = None if p.grad is None else p.grad.detach().numpy().astype(np.float32)
        names.append(k)
        has.append(g is not None)
        stats.append([np.linalg.norm(g.astype(np.float64)), np.abs(g).max()] if g is not None else [0.0, 0.0])
        samples.append(pin_sample(g, limit) if g is not None else np.zeros(0, np.float32))
        offsets.append(offsets[-1] + samples[-1].size)
    out[prefix + "names"], out[prefix + "has_grad"] = np.array(names), np.array(has)
    out[prefix + "stats"], out[prefix + "offsets"] = np.array(stats, np.float64), np.array(offsets, np.int64)
    out[prefix + "samples"] = np.concatenate(samples).astype(np.float32)


def gen_live_cases(out_dir=HERE):
    import warnings
    # the reference's train step on the oracle's small geometry
    c = LIVE_TRAIN_STEP
    sd_np = detgen.passt_state_dict(c["cfg"], c["seed"])
    x, y = model_inputs(dict(CASES["model_small_train"], seed=c["seed"]))
    m = ref_import.build_reference_passt(c["cfg"], sd_np)
    m.train()
    torch.manual_seed(c["torch_seed"])
    lr, fr = ref_import.run_silently(m, torch.from_numpy(x))
    O.bce_loss(lr, torch.from_numpy(y)).backward()
    out = {"logits": lr.detach().numpy(), "features": fr.detach().numpy()}
    _grads_into(out, "", m.named_parameters())
    np.savez_compressed(os.path.join(out_dir, "live_train_step.npz"), **out)

    # other geometries, four torch seeds each
    out = {}
    for ci, (kw, T) in enumerate(GEOMETRY_CASES):
        cfg = geometry_cfg(kw)
        sd_np = detgen.passt_state_dict(cfg, 993)
        x, y = model_inputs(dict(cfg=cfg, B=2, T=T, seed=993))
        m = ref_import.build_reference_passt(cfg, sd_np)
        m.train()
        for seed in GEOMETRY_SEEDS:
            m.zero_grad()
            pre = f"c{ci}.s{seed}."
            torch.manual_seed(seed)
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    lo, fo = ref_import.run_silently(m, torch.from_numpy(x))
                O.bce_loss(lo, torch.from_numpy(y)).backward()
            except IndexError:
                out[pre + "failed"] = np.bool_(True)
                continue
            out[pre + "failed"] = np.bool_(False)
            out[pre + "logits"], out[pre + "features"] = lo.detach().numpy(), fo.detach().numpy()
            _grads_into(out, pre, m.named_parameters(), GEOMETRY_SAMPLE)
        print("geometry", ci, kw, T, "failed seeds", [s for s in GEOMETRY_SEEDS if out[f"c{ci}.s{s}.failed"]])
    np.savez_compressed(os.path.join(out_dir, "live_geometries.npz"), **out)

    # the front end: default STFT and other STFT geometries, eval and train mode
    _, ref_pre = ref_import.load_reference()
    out = {}
    for tag, case, kws in [("base", FRONTEND_LIVE, [{}])] + [("stft", STFT_LIVE, STFT_CASES)]:
        wave = torch.from_numpy(frontend_inputs(case))
        for i, kw in enumerate(kws):
            mel = ref_import.run_silently(ref_pre.AugmentMelSTFT, **dict(case["kw"], **kw))
            for training in (False, True):
                mel.train(training)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    torch.manual_seed(case["torch_seed"])
                    with torch.no_grad():
                        mel_out = mel(wave).numpy()
                    _pinned_into(out, f"{tag}{i}.train{int(training)}", mel_out)
                    out[f"{tag}{i}.train{int(training)}.shape"] = np.array(mel_out.shape, np.int64)
    np.savez_compressed(os.path.join(out_dir, "live_frontend.npz"), **out)

    # small helpers of the caller
    out = {}
    my_mixup = ref_import.import_reference_file("helpers/mixup.py").my_mixup
    for size, alpha in MIXUP_CASES:
        for seed in MIXUP_SEEDS:
            torch.manual_seed(seed)
            np.random.seed(seed)
            idx, lam = my_mixup(size, alpha)
            after = (torch.randint(1 << 30, (1,)).item(), np.random.randint(1 << 30))
            pre = f"mixup.{size}_{alpha}.s{seed}."
            out[pre + "idx"], out[pre + "lam"], out[pre + "after"] = idx.numpy(), lam.numpy(), np.array(after, np.int64)
    ramp = ref_import.import_reference_file("helpers/ramp.py").exp_warmup_linear_down(5, 50, 50, 0.01)
    out["ramp"] = np.array([ramp(e) for e in RAMP_EPOCHS], np.float64)
    import passt_amd
    count = ref_import.import_reference_file("helpers/models_size.py").count_non_zero_params
    torch.manual_seed(MODELS_SIZE_SEED)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = passt_amd.get_model(arch="passt_s_swa_p16_128_ap476", pretrained=False, s_patchout_t=40, s_patchout_f=4)
    desc, total, nonzero = count(net)
    out["models_size.desc"] = np.array([l for l in desc.split("\n") if l.strip()])
    out["models_size.total"], out["models_size.nonzero"] = np.int64(total), np.int64(nonzero)
    cfg = O.make_cfg(**NAMES_CFG)
    ref = ref_import.build_reference_passt(cfg, detgen.passt_state_dict(cfg, 1))
    out["names.params"] = np.array([n for n, _ in ref.named_parameters()])
    out["names.state"] = np.array(list(ref.state_dict()))
    out["names.shapes"] = np.array([",".join(map(str, v.shape)) for v in ref.state_dict().values()])
    np.savez_compressed(os.path.join(out_dir, "live_helpers.npz"), **out)
    print("live fixtures written")


def gen_rng_kat():
    """SURVEY.md App. C KAT: the index path on torch CPU."""
    torch.manual_seed(123)
    a = torch.randperm(99)[:59].sort().values.numpy()
    b = torch.randperm(12)[:8].sort().values.numpy()
    c = torch.randperm(472)[:72].sort().values.numpy()
    np.savez_compressed(os.path.join(HERE, "rng_kat.npz"), t=a, f=b, u=c)


if __name__ == "__main__":
    assert ref_import.reference_available(), "needs /root/reference"
    torch.set_num_threads(min(32, os.cpu_count()))
    if len(sys.argv) > 1 and sys.argv[1] == "swa":       # the SWA callback run live (r06)
        gen_swa_case()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "live":      # what the CPU pinning tests compare with (live_*.npz)
        gen_live_cases()
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "big":      # only the full-size cases (minutes of CPU time); big <name>: one of them
        for n, c in BIG_CASES.items():
            if len(sys.argv) < 3 or n in sys.argv[2:]:
                gen_model_case(n, c)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "b64":       # config #2 at the benchmarked batch
        for n, c in B64_CASES.items():
            if len(sys.argv) < 3 or n in sys.argv[2:]:
                gen_model_case(n, c)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "bench":     # configs #4 / #5 at their benchmarked batch (r06)
        for n, c in BENCH_CASES.items():
            if len(sys.argv) < 3 or n in sys.argv[2:]:
                gen_model_case(n, c)
        sys.exit(0)
    for n, c in CASES.items():
        gen_model_case(n, c)
    for n, c in FRONTEND_CASES.items():
        gen_frontend_case(n, c)
    gen_rng_kat()
    gen_wave_case()
    gen_swa_case()
    gen_live_cases()

"""CPU tests of the gradient w.r.t. the waveform: the reference fixture (tests/golden/wave_grad.npz) against the oracle's own
float64 autograd, the C ABI additions, and the resources of the front-end kernels in the built library.

Bound: errors of dwave are taken per clip, relative to that clip's largest |dwave| (the convention of varlen_grad.npz); the limit is
the project's parity-mode bound 1e-3.  (For scale: f32 against f64 autograd of the oracle differ by 0.6-2.3e-5 on these inputs.)"""
import os
import re
import subprocess
import tempfile
import warnings

import numpy as np
import pytest
import torch

from oracle import ref_import
from oracle import passt_oracle as O
from passt_amd import _lib
from tests.golden import make_golden as G
from tests.golden import make_wave_grad_golden as WG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pa_mel_frontend_bwd", "pa_mel_frontend_bwd_varlen")
LIMIT = 1e-3
LLVM = "/opt/rocm/lib/llvm/bin/"


def oracle_dwave(case, wave_np, g_np, dtype=torch.float64):
    """(spec, dwave) of the oracle front end under the fixture's loss (mel * g).sum(); wave_np (B, L), g_np (B, n_mels, T)."""
    w = torch.from_numpy(np.ascontiguousarray(wave_np)).to(dtype).requires_grad_()
    if "torch_seed" in case:
        torch.manual_seed(case["torch_seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        spec = O.mel_frontend(w, training=case["training"], dtype=dtype, **case["kw"])
    (spec * torch.from_numpy(np.ascontiguousarray(g_np)).to(dtype)).sum().backward()
    return spec.detach(), w.grad


def clip_errors(gold, key, got, ten_s=False):
    """(error on the kept samples, error of the largest magnitude, error of the L2 norm) of one clip's whole dwave ``got`` against
    the fixture: the first two relative to the clip's largest |dwave|, the third relative to the norm."""
    got = np.ascontiguousarray(got, np.float64)
    nrm, scale = (float(v) for v in gold[key + ".stats"])
    smp = G.pin_sample(got, WG.TEN_S_SAMPLE) if ten_s else got[WG.keep_index(got.size)]
    assert smp.shape == gold[key].shape, key
    return (float(np.abs(smp - gold[key]).max() / scale), abs(float(np.abs(got).max()) - scale) / scale,
            abs(float(np.linalg.norm(got)) - nrm) / nrm)


def test_fixture_regenerates_bit_identically(golden_dir, tmp_path, monkeypatch):
    if not ref_import.reference_available():
        pytest.skip("the reference checkout is not on this machine")
    monkeypatch.setattr(WG, "HERE", str(tmp_path))
    WG.main()
    new, old = dict(np.load(tmp_path / "wave_grad.npz")), dict(np.load(os.path.join(golden_dir, "wave_grad.npz")))
    assert sorted(new) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k


@pytest.mark.parametrize("name", list(WG.CASES))
def test_oracle_autograd_dwave_matches_reference_fixture(golden_dir, name):
    gold = dict(np.load(os.path.join(golden_dir, "wave_grad.npz")))
    case = WG.CASES[name]
    wave = G.frontend_inputs(case)
    T = WG.frames_of(case["L"], case["kw"].get("hopsize", 320))
    spec, dw = oracle_dwave(case, wave, WG.upstream(case, (case["B"], case["kw"].get("n_mels", 128), T)))
    for i in range(case["B"]):
        e = clip_errors(gold, f"{name}.dwave.{i}", dw[i].numpy(), ten_s=name == "frontend_eval_10s")
        print(f"wave_grad oracle f64 vs reference {name} clip {i}: samples {e[0]:.2e} absmax {e[1]:.2e} norm {e[2]:.2e}")
        assert max(e) <= LIMIT, (name, i, e)


def test_oracle_autograd_dwave_ragged_clips_match_reference_fixture(golden_dir):
    gold = dict(np.load(os.path.join(golden_dir, "wave_grad.npz")))
    case = WG.RAGGED
    waves = G.frontend_inputs(case)
    g = WG.upstream(case, (case["B"], 128, WG.frames_of(max(WG.RAGGED_LENS))))
    for i, n in enumerate(WG.RAGGED_LENS):
        _, dw = oracle_dwave(case, waves[i:i + 1, :n], g[i:i + 1, :, :WG.frames_of(n)])
        e = clip_errors(gold, f"ragged.dwave.{i}", dw[0].numpy())
        print(f"wave_grad oracle f64 vs reference ragged clip {i} ({n}): samples {e[0]:.2e} absmax {e[1]:.2e} norm {e[2]:.2e}")
        assert max(e) <= LIMIT, (i, e)


def test_header_declares_the_new_entry_points_and_abi_6():
    src = open(os.path.join(ROOT, "include", "passt_amd.h")).read()
    assert re.search(r"#define\s+PA_ABI_VERSION\s+6\b", src)
    for n in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n


def test_binding_and_library_carry_the_new_entry_points():
    lib = _lib.load()
    assert lib.pa_abi_version() == 6
    for n in NEW_SYMBOLS:
        assert n in _lib.SIGNATURES, n
        assert hasattr(lib, n), n
    assert len(_lib.SIGNATURES["pa_mel_frontend_bwd"][1]) == 12 and len(_lib.SIGNATURES["pa_mel_frontend_bwd_varlen"][1]) == 14
    # argument validation answers without a GPU, with the forward's codes
    p = _lib.MelParams()
    p.n_fft, p.hop, p.n_mels, p.n_frames = 1024, 320, 128, 99
    one = 1 << 12          # any non-null address: the checks fail before anything is touched
    assert lib.pa_mel_frontend_bwd(None, 1, 32000, one, one, one, one, one, None, 0, p, None) == -1
    assert lib.pa_mel_frontend_bwd(one, 1, 400, one, one, one, one, one, None, 0, p, None) == -2       # too short to reflect
    assert lib.pa_mel_frontend_bwd(one, 1, 32000, one, one, one, one, one, None, 0, p, None) == -1     # n_frames does not fit L
    p.n_mels = 200
    assert lib.pa_mel_frontend_bwd(one, 1, 32000, one, one, one, one, one, None, 0, p, None) == -2
    assert lib.pa_mel_frontend_bwd_varlen(one, 1, 32000, one, one, one, one, one, 100, one, None, 0, p, None) == -2
    p.n_mels = 128
    assert lib.pa_mel_frontend_bwd_varlen(one, 1, 32000, None, one, one, one, one, 100, one, None, 0, p, None) == -1
    assert lib.pa_mel_frontend_bwd_varlen(one, 1, 32000, one, one, one, one, one, 101, one, None, 0, p, None) == -1


def _mel_kernel_resources():
    """{kernel name: (vgpr, sgpr, scratch bytes, static lds)} of the front-end kernels in the built library."""
    so = _lib.LIB_PATH
    tools = [LLVM + t for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(so) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library not built / no llvm tools")
    res = {}
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([tools[0], "--dump-section", f".hip_fatbin={fat}", so, os.path.join(d, "copy.so")], check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
        for k, st in enumerate(starts):
            part, co = os.path.join(d, f"b{k}.bin"), os.path.join(d, f"b{k}.co")
            open(part, "wb").write(blob[st:starts[k + 1] if k + 1 < len(starts) else len(blob)])
            subprocess.run([tools[1], "--type=o", "--unbundle", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([tools[2], "--notes", co], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count")[1:]:
                n = re.search(r"\.name:\s+(\S+)", blk)
                if n and "mel_frontend" in n.group(1):
                    g = lambda key: int(re.search(key + r":\s+(\d+)", blk).group(1))      # noqa: E731
                    res[n.group(1)] = (g(r"\.vgpr_count"), g(r"\.sgpr_count"), g(r"\.private_segment_fixed_size"),
                                       g(r"\.group_segment_fixed_size"))
    return res


def test_backward_kernels_use_no_scratch_and_forward_kernels_keep_their_resources():
    res = _mel_kernel_resources()
    bwd = {k: v for k, v in res.items() if "mel_frontend_bwd_kernel" in k}
    assert len(bwd) == 2, sorted(res)                        # fixed-length and ragged instance
    for k, (vgpr, sgpr, scratch, lds) in bwd.items():
        print(k, "vgpr", vgpr, "sgpr", sgpr, "scratch", scratch, "lds", lds)
        assert scratch == 0 and vgpr <= 256, (k, vgpr, scratch)
    # the shipped forward instances as they were before the backward joined their translation unit (one-tile, ragged: 168 VGPRs,
    # no scratch, dynamic LDS only; 168 VGPRs = three waves per SIMD)
    fwd = {k: v for k, v in res.items() if "mel_frontend_kernelILi16ELb0E" in k}
    assert len(fwd) == 2, sorted(res)
    for k, (vgpr, sgpr, scratch, lds) in fwd.items():
        assert (vgpr, scratch, lds) == (168, 0, 0), (k, vgpr, scratch, lds)
    assert sorted(v[1] for v in fwd.values()) == [54, 56]


def test_band_transpose_and_one_sided_inverse_emulated_on_the_cpu():
    import importlib.util
    spec = importlib.util.spec_from_file_location("emulate_mel_bwd", os.path.join(ROOT, "tools", "emulate_mel_bwd.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.main() == 0

"""Exact-operand and guarded-buffer parity of the mel front end -- pa_mel_frontend_fwd, _fwd_varlen, _fwd_varlen_aug, _bwd, _bwd_varlen,
_bwd_varlen_aug and the persistent form of the forward -- through the C ABI, so that the test owns every buffer and every field of
pa_mel_params (tests/mel_cases.py holds the case lists, operand families, f64 references, derived bounds and checkers; the same
checkers pass against plain f32 torch in tests/test_mel_cases_cpu.py).  The worst got / bound per group goes to
mel_exact_parity_metrics.json in $PASST_AMD_METRICS_DIR (default: test_metrics/ in the repository root);
profiles/mel_exact_parity.txt keeps them."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from passt_amd import _lib  # noqa: E402
from tests import mel_cases as M  # noqa: E402
from tests.mel_cases import PA_EINVAL, PA_OK, SENTINEL, GuardedOut  # noqa: E402
from tests.row_kernel_cases import GUARD, guarded_in  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mel_persist_worker.py")
_FIG = {}
NAN_BITS = 0x7FC00000


def metrics_dir():
    out = os.environ.get("PASST_AMD_METRICS_DIR") or os.path.join(ROOT, "test_metrics")
    os.makedirs(out, exist_ok=True)
    return out


def record(group, **figs):
    g = _FIG.setdefault(group, {"checks": 0})
    g["checks"] += 1
    for k, v in figs.items():
        g[k] = (g.get(k, 0) + v) if k in ("loose", "live") else max(g.get(k, 0.0), float(v))
    with open(os.path.join(metrics_dir(), os.environ.get("PASST_AMD_MEL_METRICS_FILE", "mel_exact_parity_metrics.json")), "w") as f:
        json.dump(_FIG, f, indent=1, sort_keys=True)


def guarded_wave(t):
    """[B][pitch] on the device between at least one row of NaN on either side, the base pointer 16-byte aligned whatever the pitch:
    rows are misaligned through pitch mod 4 only"""
    n = t.numel()
    guard = -(-max(GUARD, t.shape[-1]) // 4) * 4
    buf = torch.full((guard + n + guard,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[guard:guard + n].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return view


def guarded_clip_table(rows):
    """pa_mel_clip_params[B] between NaN dwords"""
    words = []
    for r in rows:
        words += list(struct.unpack("<6i", struct.pack("<2f4i", float(r[0]), float(r[1]), *(int(v) for v in r[2:]))))
    nan = struct.unpack("<i", struct.pack("<I", NAN_BITS))[0]
    buf = torch.tensor([nan] * GUARD + words + [nan] * GUARD, dtype=torch.int32).to(DEV)
    return buf[GUARD:GUARD + len(words)]


def untouched(g, what):
    assert bool((g.buf == SENTINEL).all()), f"{what}: written"


class Hip:
    """The six C entries of libpasst_amd.so behind the calling conventions of mel_cases.TorchMel.  The waveform, the three tables, dout,
    lens and the clip table are views into larger allocations with NaN in front of and behind them; out and dwave are GuardedOut
    allocations filled with the sentinel, which `take` requires to be written completely and nowhere else."""
    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self.st = torch.cuda.current_stream().cuda_stream

    def params(self, mp, nfr, over=None):
        over = over or {}
        p = _lib.MelParams()
        p.n_fft, p.hop, p.n_mels, p.n_frames = over.get("n_fft", M.NFFT), over.get("hop", mp.hop), over.get("n_mels", mp.n_mels), nfr
        p.preemph, p.mel_low, p.inv_mel_delta = mp.preemph, mp.mel_low, mp.inv_mel_delta
        p.log_eps, p.out_add, p.out_scale = mp.log_eps, mp.out_add, mp.out_scale
        (p.fmask_start, p.fmask_end), (p.tmask_start, p.tmask_end) = mp.fmask, mp.tmask
        return p

    def call(self, entry, wave, tabs, mp, lens=None, dout=None, T_max=None, fill=M.FILL, clip=None, over=None):
        """one launch; over: the deliberate faults of the argument table (mel_cases.ARG_FAULTS).  Returns (rc, GuardedOut)."""
        over = over or {}
        B, pitch = wave.shape
        varlen, bwd, aug = "varlen" in entry, entry.startswith("bwd"), entry.endswith("aug")
        Larg = over.get("L", pitch)
        hop = over.get("hop", mp.hop)
        nfr = (T_max if varlen else self.lib.pa_mel_num_frames(Larg, hop))
        if "T_max_extra" in over:
            nfr = self.lib.pa_mel_num_frames(Larg, hop) + over["T_max_extra"]
        T_arg = over.get("T_max", nfr)
        p = self.params(mp, (nfr if "T_max" not in over else T_arg) + over.get("dframes", 0), over)
        keep = dict(wave=guarded_wave(wave), window=guarded_in(tabs["window"], DEV), bin_mel=guarded_in(tabs["bin_mel"], DEV),
                    twiddle=guarded_in(tabs["twiddle"], DEV))
        if varlen:
            keep["lens"] = guarded_in(torch.tensor(lens, dtype=torch.int32), DEV)
        if aug:
            keep["clip"] = guarded_clip_table(clip)
        if bwd:
            keep["dout"] = guarded_in(dout, DEV)
        T_out = max(nfr, 1)
        res = GuardedOut((B, pitch) if bwd else (B, mp.n_mels, T_out), torch.float32, DEV)
        ptr = {k: v.data_ptr() for k, v in keep.items()}
        ptr["wave"] += 4 * over.get("misalign", 0)
        ptr["result"], ptr["p"] = res.ptr(), C.byref(p)
        if over.get("null"):
            assert over["null"] in ptr, (entry, over)
            ptr[over["null"]] = None
        Barg = over.get("B", B)
        tab3 = (ptr["window"], ptr["bin_mel"], ptr["twiddle"])
        L = self.lib
        if entry == "fwd":
            rc = L.pa_mel_frontend_fwd(ptr["wave"], Barg, Larg, *tab3, ptr["result"], ptr["p"], self.st)
        elif entry == "fwd_varlen":
            rc = L.pa_mel_frontend_fwd_varlen(ptr["wave"], Barg, Larg, ptr["lens"], *tab3, ptr["result"], T_arg, fill, ptr["p"], self.st)
        elif entry == "fwd_varlen_aug":
            rc = L.pa_mel_frontend_fwd_varlen_aug(ptr["wave"], Barg, Larg, ptr["lens"], *tab3, ptr["result"], T_arg, fill, ptr["p"], ptr["clip"], self.st)
        elif entry == "bwd":
            rc = L.pa_mel_frontend_bwd(ptr["wave"], Barg, Larg, *tab3, ptr["dout"], ptr["result"], None, 0, ptr["p"], self.st)
        elif entry == "bwd_varlen":
            rc = L.pa_mel_frontend_bwd_varlen(ptr["wave"], Barg, Larg, ptr["lens"], *tab3, ptr["dout"], T_arg, ptr["result"], None, 0, ptr["p"], self.st)
        else:
            rc = L.pa_mel_frontend_bwd_varlen_aug(ptr["wave"], Barg, Larg, ptr["lens"], *tab3, ptr["dout"], T_arg, ptr["result"], None, 0, ptr["p"],
                                                  ptr["clip"], self.st)
        torch.cuda.synchronize()
        del keep
        return rc, res

    def _take(self, rc, res, what):
        return rc, (res.take(what) if rc == PA_OK else None)

    def fwd(self, wave, tabs, mp):
        return self._take(*self.call("fwd", wave, tabs, mp), "out")

    def bwd(self, wave, tabs, mp, dout):
        return self._take(*self.call("bwd", wave, tabs, mp, dout=dout), "dwave")

    def fwd_varlen(self, wave, lens, tabs, mp, T_max, fill, clip=None):
        return self._take(*self.call("fwd_varlen_aug" if clip else "fwd_varlen", wave, tabs, mp, lens=lens, T_max=T_max, fill=fill, clip=clip), "out")

    def bwd_varlen(self, wave, lens, tabs, mp, dout, T_max, clip=None):
        return self._take(*self.call("bwd_varlen_aug" if clip else "bwd_varlen", wave, tabs, mp, lens=lens, dout=dout, T_max=T_max, clip=clip), "dwave")


@pytest.fixture(scope="module")
def hip():
    return Hip()


@pytest.mark.parametrize("c", M.forward_cases(), ids=lambda c: c.name)
def test_forward(hip, c):
    """pa_mel_frontend_fwd: masked cells exactly the constant, silent frames bit-equal to an all-zero clip's cells, every other cell
    inside its derived bound; no loose cell in the impulse and graded families"""
    M.check_forward(hip, c, record)


@pytest.mark.parametrize("c", M.backward_cases(), ids=lambda c: c.name)
def test_backward(hip, c):
    """pa_mel_frontend_bwd: dense and one-hot upstream gradients; exactly 0 outside the support, inside the bound within it; NaN at
    masked cells of dout does not reach dwave"""
    M.check_backward(hip, c, record)


@pytest.mark.parametrize("c", M.packed_cases() + [M.packed_impulse_case()], ids=lambda c: c.name)
def test_packed(hip, c):
    """the four packed entries: NaN behind lens[b] in every row, `fill` behind a clip's frames, exact zeros behind its samples, every
    row bit-equal to the clip transformed alone through the fixed-length entry"""
    M.check_packed(hip, c, record)


def test_equal_lengths_give_the_fixed_length_result(hip):
    """lens[b] = ldw for every b, and a table that repeats *p's six values: bit for bit the fixed-length entries' results"""
    c = M.MC("graded", 5121, M.MP(fmask=(3, 9), tmask=(-1, 2)), range(3), seed=11)
    tabs, wave, dout = M.tables(c.mp.window), M.case_wave(c), M.case_dout(c)
    lens, tab = [c.L] * c.B, [c.mp.clip()] * c.B
    _, out = hip.fwd(wave, tabs, c.mp)
    _, dw = hip.bwd(wave, tabs, c.mp, dout)
    for clip in (None, tab):
        assert torch.equal(hip.fwd_varlen(wave, lens, tabs, c.mp, c.T, M.FILL, clip)[1], out)
        assert torch.equal(hip.bwd_varlen(wave, lens, tabs, c.mp, dout, c.T, clip)[1], dw)


def test_argument_checks(hip):
    """every entry refuses every fault of mel_cases.ARG_FAULTS with the header's code and launches nothing: out / dwave keep the sentinel"""
    mp, tabs = M.MP(bank_name="m5"), M.tables()
    B, L = 2, M.ARG_L
    wave = M.graded_noise(B, L, 3, mp.hop)
    T = M.n_frames(L, mp.hop)
    lens, clip, dout = [L, 900], [mp.clip()] * B, torch.ones(B, mp.n_mels, T)
    for entry in M.ENTRIES:
        args = dict(lens=lens, T_max=T, clip=clip if entry.endswith("aug") else None, dout=dout if entry.startswith("bwd") else None)
        rc, res = hip.call(entry, wave, tabs, mp, **args)
        assert rc == PA_OK, entry
        res.take(entry)
        for name, over, want in M.ARG_FAULTS:
            if over.get("null") == "dout" and not entry.startswith("bwd") or over.get("null") == "lens" and "varlen" not in entry \
                    or over.get("null") == "clip" and not entry.endswith("aug") or ("T_max" in over or "T_max_extra" in over) and "varlen" not in entry:
                continue
            rc, res = hip.call(entry, wave, tabs, mp, over=over, **args)
            assert rc == want, (entry, name, rc)
            untouched(res, f"{entry} refused ({name})")
    assert PA_EINVAL != PA_OK


def test_persistent_form():
    """PA_MEL_PERSIST is read once per process: a fresh child runs the fixed-length forward checkers with it set, among them a call
    with more tiles than resident workgroups (tests/mel_persist_worker.py)"""
    env = dict(os.environ, PA_MEL_PERSIST="1", PASST_AMD_MEL_METRICS_FILE="mel_exact_parity_persist_metrics.json")
    r = subprocess.run([sys.executable, WORKER], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "mel persist OK" in out, out[-4000:]

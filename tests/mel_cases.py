"""Case lists, operand families, f64 references, derived bounds and checkers of the mel front-end parity suite.

Used by tests/test_gpu_mel_exact.py (the six C entry points pa_mel_frontend_fwd / _fwd_varlen / _fwd_varlen_aug / _bwd / _bwd_varlen /
_bwd_varlen_aug and the persistent form, through the C ABI) and tests/test_mel_cases_cpu.py (the same checkers against `TorchMel`,
plain f32 torch on the CPU, and against thirteen fault models).  A checker hands an `impl` object CPU tensors and gets CPU tensors
back; it neither knows nor cares where the arithmetic ran.

Reference.  The numbered forward / backward formulas at pa_mel_frontend_bwd in include/passt_amd.h, evaluated in f64 from the same f32
tables (`F64Mel`).  Only the filterbank geometry is f32: t_k = (bin_mel[k] - mel_low) * inv_mel_delta as two correctly rounded f32
operations, j_k = floor(t_k), u_k = t_k - j_k (exact), so a bin on a triangle edge lands in the kernel's triangle.  The backward
reference is autograd through that f64 forward; the explicit steps 1-7 of the header are implemented as well (`backward`): they give
the intermediates the bounds need, are what the f32 twin runs, and test_mel_cases_cpu.py shows them equal to autograd.

Bounds.  Per cell, derived from the algorithm as documented in passt_amd/csrc/mel.hip, u = 2^-24:
  d_t     = u (R sum_i |f_t[i]| + sum_i |w[i]| |preemph x[src(i)]|)             error of one spectrum value of frame t
            Every rounding on a path through the transform is a relative error u of an intermediate; the intermediates of one
            level add up (triangle inequality) to at most sum_i |f_t[i]|, so a level costs u sum|f|.  R = 31 levels:
              2  the pre-emphasis result, the window product
              15 three 8-point DFTs: three add levels, the product with the constant 1/sqrt 2 and that constant's own rounding
              8  two twiddle products: 2 sqrt 2 < 3 for the complex product (a product and an FMA per component), 1 for the
                 f32 table entry (the reference transform is exact, the table is not)
              6  the real-FFT untangle: the conjugate sums (1), the product with W^k (3 + 1), the final sum (1)
            The second sum is the rounding of the product preemph x[i], whose magnitude is that of x and not of y = x[i+1] -
            preemph x[i] (0 when preemph = 0).
  d mel_j = sum_k W_jk (2 |X_k| d_t + d_t^2) + u (G mel_j + 2 sum_{k: j_k = j + 1} P_k)
            G = 26: the squares and their sum (2), the product with u_k (1), and 23 for the band sum -- a lane adds its eight bins
            (8), the segmented scan has six steps (6), the lane adds its eight bins again on top of the carry (8), up- and
            down-slope sums are added (1).  The last term: the kernel forms the down-slope contribution P (1 - u) as P - P u, two
            roundings relative to P, not to P (1 - u).
  d out   = out_scale (-log(1 - r) + e_log) + u (|log(mel + eps) + out_add| out_scale + |out|),  r = d mel / (mel + log_eps)
            (r >= 1: no bound, the cell counts as loose and only has to be finite).  e_log: the ROCm device library ships as
            bitcode, without a statement of the fast logarithm's accuracy, so e_log = 4 x what f32 torch.log on
            the CPU needs on the same cells (largest |f32 log - f64 log| over the call's unmasked cells) + u for the rounding of
            mel + log_eps.
  backward  the same terms through steps 1-7: e(dmel) = |dmel| (r / (1 - r) + 5 u) (product, sum, division to 2.5 ulp);
            e(dP) = W^T e(dmel) + 3 u W^T |dmel|;  e(G_k) = 2 (|dP_k| d_t + e(dP_k) (|X_k| + d_t)) + 2 u |G_k|;
            e(df_t) = sum_k e(G_k) + R_INV u sum_k |G_k| on every tap (R_INV = 30: the H formation 6, the transform 23, the
            window product 1);  taps, overlap-add, reflect adjoint and pre-emphasis adjoint are linear with the non-negative
            coefficients |w|, 1, |preemph|, so the errors run through them unchanged, and every sum of n terms adds (n - 1) u
            times the sum of the absolute terms.  The magnitudes are those of the reference around the sample (the absolute taps
            overlap-added locally), never the global maximum; where no term is non-zero the bound is 0 and the result must be
            exactly 0.

Guards: tests/row_kernel_cases.py (`guarded_in`, `GuardedOut`, the sentinel); `guarded_wave` in tests/test_gpu_mel_exact.py keeps the
waveform's base pointer 16-byte aligned.
"""
import math

import torch

from tests.row_kernel_cases import GUARD, SENTINEL, GuardedOut  # noqa: F401  (re-exported for the GPU file)

NFFT, NC, SR = 1024, 512, 32000
FR, FR_PERSIST, VEC_CAP = 16, 8, 12 * 4 * 256
U24 = 2.0 ** -24
R_FWD, G_BAND, R_INV = 31, 26, 30
LOOSE = 1e-4                       # a tenth of the old whole-tensor tolerance
FILL = -7.25                       # no result can equal it: exact in f32, below (log(eps) + out_add) out_scale of every case
F32, F64 = torch.float32, torch.float64
PA_OK, PA_EINVAL, PA_EUNSUPPORTED = 0, -1, -2


def f32(v):
    return float(torch.tensor(v, dtype=F32))


def bwd_rows(hop):
    """samples one workgroup of the backward owns (documented launch geometry)"""
    return hop * max(FR, -(-2 * NFFT // hop))


def n_frames(L, hop):
    return 0 if L < 2 else 1 + (L - 1) // hop


# ---- tables and parameters -----------------------------------------------------------------------------------------------
def window_table(kind):
    if kind == "rect":
        return torch.ones(NFFT)
    if kind == "hann":
        return torch.hann_window(NFFT, periodic=True)
    assert kind == "hann800"
    w = torch.zeros(NFFT)
    w[112:912] = torch.hann_window(800, periodic=False)       # the shipped window, centred as torch.stft centres it
    return w


_TABS = {}


def tables(window="hann800"):
    if window not in _TABS:
        k = torch.arange(NC, dtype=F64)
        ang = 2.0 * math.pi * k / NFFT
        _TABS[window] = dict(window=window_table(window), bin_mel=(1127.0 * torch.log1p(k * (SR / NFFT) / 700.0)).float(),
                             twiddle=torch.stack([torch.cos(ang), -torch.sin(ang)], 1).float().contiguous())
    return _TABS[window]


def bank(n_mels, fmin, fmax):
    lo, hi = 1127.0 * math.log(1.0 + fmin / 700.0), 1127.0 * math.log(1.0 + fmax / 700.0)
    return f32(lo), f32((n_mels + 1) / (hi - lo))


SHIPPED_BANK = (128, 0.0, 15500.0)
BANKS = {"shipped": SHIPPED_BANK, "m64": (64, 50.0, 14000.0), "m5": (5, 300.0, 9000.0), "m4": (4, 0.0, 16000.0),
         "low128": (128, 20.0, 1200.0)}          # 128 bands under 1.2 kHz: 38 bins for 129 edges, most triangles are empty


class MP:
    """pa_mel_params of one call, every float the f32 number the kernel receives"""

    def __init__(self, hop=320, bank_name="shipped", preemph=0.97, log_eps=1e-5, out_add=4.5, out_scale=0.2, fmask=(0, 0), tmask=(0, 0),
                 window="hann800"):
        self.hop, self.window, self.bank_name = hop, window, bank_name
        self.n_mels = BANKS[bank_name][0]
        self.mel_low, self.inv_mel_delta = bank(*BANKS[bank_name])
        self.preemph, self.log_eps, self.out_add, self.out_scale = f32(preemph), f32(log_eps), f32(out_add), f32(out_scale)
        self.fmask, self.tmask = tuple(fmask), tuple(tmask)

    def clip(self):
        """this call's six per-clip values as an entry of the pa_mel_clip_params table"""
        return (self.mel_low, self.inv_mel_delta, *self.fmask, *self.tmask)

    def with_clip(self, c):
        q = MP.__new__(MP)
        q.__dict__.update(self.__dict__)
        q.mel_low, q.inv_mel_delta, q.fmask, q.tmask = c[0], c[1], (c[2], c[3]), (c[4], c[5])
        return q

    def mask_const(self):
        return float(torch.tensor(self.out_add, dtype=F32) * torch.tensor(self.out_scale, dtype=F32))      # (0 + out_add) out_scale in f32


def geometry(mp, tabs):
    """(j_k, u_k) as the kernel forms them: two correctly rounded f32 operations, floor, an exact difference"""
    t = (tabs["bin_mel"] - torch.tensor(mp.mel_low, dtype=F32)) * torch.tensor(mp.inv_mel_delta, dtype=F32)
    fl = torch.floor(t)
    return fl.clamp(-1.0, 100000.0).long(), t - fl


# ---- the arithmetic: one implementation, f32 (the twin) and f64 (the reference) -----------------------------------------
class TorchMel:
    """The header's formulas in plain torch on the CPU with the kernels' calling conventions.  dt = f32: the twin whose every result
    must meet the bounds.  The small methods are the places where the fault models of test_mel_cases_cpu.py differ."""
    name, dt = "torch_f32", F32
    preemph_after_pad = False
    bwd_mirror_512 = bwd_last_term = True
    bwd_oa_miss = False

    # -- hooks --
    def mirror_lo(self, i):
        return -i

    def mirror_hi(self, i, Ly):
        return 2 * (Ly - 1) - i

    def window(self, w):
        return w

    def origin(self):
        return 0

    def slopes(self, u):
        return u, 1.0 - u

    def top_down_slope(self):
        return True

    def nyquist_weight(self):
        return 0.0

    def tmasked(self, t, ts, te):
        return (t >= ts) & (t < te)

    def reflect_len(self, L, ldw):
        return L

    # -- forward --
    def pad_index(self, Ly):
        i = torch.arange(-NC, Ly + NC)
        i = torch.where(i < 0, self.mirror_lo(i), i)
        i = torch.where(i >= Ly, self.mirror_hi(i, Ly), i)
        return i.clamp(0, Ly - 1)

    def basis(self, mp, tabs):
        """[n_mels][513]: bin k feeds triangle j_k with u_k and triangle j_k - 1 with 1 - u_k; column 512 is zero"""
        j, u = geometry(mp, tabs)
        up, down = self.slopes(u.to(self.dt))
        W = torch.zeros(mp.n_mels, NC + 1, dtype=self.dt)
        k = torch.arange(NC)
        a = (j >= 0) & (j < mp.n_mels)
        W[j[a], k[a]] += up[a]
        b = (j >= 1) & (j <= (mp.n_mels if self.top_down_slope() else mp.n_mels - 1))
        W[j[b] - 1, k[b]] += down[b]
        W[mp.n_mels - 1, NC] = self.nyquist_weight()
        return W

    def mask(self, mp, T):
        band, t = torch.arange(mp.n_mels)[None, :], torch.arange(T)[:, None]
        return ((band >= mp.fmask[0]) & (band < mp.fmask[1])) | self.tmasked(t, *mp.tmask)       # [T][n_mels]

    def padded_signal(self, x, L, mp, Lr=None):
        pre = torch.tensor(mp.preemph, dtype=self.dt)
        Lr = L if Lr is None else Lr                          # the length the reflection is taken from (a fault model's differs)
        if self.preemph_after_pad:
            i = torch.arange(-NC, L + NC)
            i = torch.where(i < 0, -i, i)
            i = torch.where(i >= L, 2 * (L - 1) - i, i).clamp(0, L - 1)
            xp = x[i]
            return xp[1:] - pre * xp[:-1], None
        y = x[1:Lr] - pre * x[:Lr - 1]
        idx = self.pad_index(Lr - 1)
        return y[idx], idx

    def forward(self, x, L, mp, tabs, Lr=None):
        """one clip: x 1-D of dtype dt, its first L samples; every intermediate of the header's forward"""
        w = self.window(tabs["window"]).to(self.dt)
        yp, idx = self.padded_signal(x, L, mp, Lr)
        o = self.origin()
        if o:
            yp = torch.cat([yp[o:], torch.zeros(o, dtype=self.dt)])
        T = n_frames(L, mp.hop)
        fr = yp.unfold(0, NFFT, mp.hop)[:T] * w
        X = torch.fft.rfft(fr, dim=1)
        P = X.real ** 2 + X.imag ** 2
        W = self.basis(mp, tabs)
        mel = P @ W.t()
        val = (torch.log(mel + torch.tensor(mp.log_eps, dtype=self.dt)) + torch.tensor(mp.out_add, dtype=self.dt)) * torch.tensor(mp.out_scale, dtype=self.dt)
        mask = self.mask(mp, T)
        out = torch.where(mask, torch.tensor(mp.mask_const(), dtype=self.dt), val)
        return dict(fr=fr, X=X, P=P, W=W, mel=mel, out=out.t(), mask=mask, idx=idx, w=w, T=T)

    # -- backward: steps 1-7 of the header --
    def backward(self, x, L, mp, tabs, dout):
        """one clip: dout [n_mels][T] -> dwave [L] and the intermediates"""
        f = self.forward(x, L, mp, tabs)
        T, Ly, hop = f["T"], L - 1, mp.hop
        g = dout.t().to(self.dt)
        dmel = torch.where(f["mask"], torch.zeros((), dtype=self.dt),
                           g * torch.tensor(mp.out_scale, dtype=self.dt) / (f["mel"] + torch.tensor(mp.log_eps, dtype=self.dt)))      # 1
        dP = dmel @ f["W"]                                                                     # 2
        G = 2 * dP[:, :NC] * f["X"][:, :NC]                                                    # 3
        Z = torch.zeros(T, NFFT, dtype=G.dtype)
        Z[:, :NC] = G
        df = torch.fft.ifft(Z, dim=1).real * NFFT                                              # 4: the one-sided sum, no 1/N
        tap = df * f["w"]
        q = (torch.arange(T)[:, None] * hop + torch.arange(NFFT)[None, :]).reshape(-1)
        dyp = torch.zeros(Ly + NFFT + hop, dtype=self.dt).index_add_(0, q, tap.reshape(-1))[:Ly + NFFT]      # 5
        if self.bwd_oa_miss:
            rows = bwd_rows(hop)
            for n0 in range(rows, L, rows):
                qlo = n0 - 1 + NC
                t = (qlo - 1) // hop                         # the frame that starts in front of this workgroup's run
                if t < T:
                    hi = min(t * hop + NFFT, qlo + rows, Ly + NFFT)
                    dyp[qlo:hi] -= tap[t, qlo - t * hop:hi - t * hop]
        if not self.bwd_mirror_512:
            dyp = dyp.clone()
            dyp[0] = 0
        dy = torch.zeros(Ly, dtype=self.dt).index_add_(0, f["idx"], dyp)                        # 6: the adjoint of the gather
        z = torch.zeros(1, dtype=self.dt)
        dw = torch.cat([z, dy]) - torch.tensor(mp.preemph, dtype=self.dt) * torch.cat([dy, z])  # 7
        if not self.bwd_last_term:
            dw[L - 1] = 0
        return dict(f, dmel=dmel, dP=dP, G=G, tap=tap, dyp=dyp, dy=dy, dw=dw, q=q)

    # -- the kernels' calling conventions --
    def fwd(self, wave, tabs, mp):
        return PA_OK, torch.stack([self.forward(x.to(self.dt), wave.shape[1], mp, tabs)["out"] for x in wave]).float()

    def bwd(self, wave, tabs, mp, dout):
        return PA_OK, torch.stack([self.backward(x.to(self.dt), wave.shape[1], mp, tabs, g)["dw"] for x, g in zip(wave, dout)]).float()

    def fwd_varlen(self, wave, lens, tabs, mp, T_max, fill, clip=None):
        B, ldw = wave.shape
        out = torch.full((B, mp.n_mels, T_max), fill, dtype=F32)
        for b, L in enumerate(lens):
            if L - 1 > NC:
                Lr = self.reflect_len(L, ldw)
                o = self.forward(wave[b, :max(L, Lr)].to(self.dt), L, mp.with_clip(clip[b]) if clip else mp, tabs, Lr)["out"]
                out[b, :, :o.shape[1]] = o[:, :T_max]
        return PA_OK, out

    def bwd_varlen(self, wave, lens, tabs, mp, dout, T_max, clip=None):
        B, ldw = wave.shape
        dw = torch.zeros(B, ldw, dtype=F32)
        for b, L in enumerate(lens):
            if L - 1 > NC:
                T = n_frames(L, mp.hop)
                dw[b, :L] = self.backward(wave[b, :L].to(self.dt), L, mp.with_clip(clip[b]) if clip else mp, tabs, dout[b, :, :T])["dw"]
        return PA_OK, dw


class F64Mel(TorchMel):
    name, dt = "f64", F64


REF = F64Mel()


def ref_backward_autograd(x, L, mp, tabs, dout):
    """the backward reference: autograd through the f64 forward (dout: [n_mels][T], NaN at masked cells allowed)"""
    xr = x.double().clone().requires_grad_(True)
    f = REF.forward(xr, L, mp, tabs)
    g = torch.where(f["mask"].t(), torch.zeros((), dtype=F64), dout.double())
    f["out"].backward(g)
    return xr.grad


# ---- bounds --------------------------------------------------------------------------------------------------------------
def spectrum_error(f, x, mp):
    """d_t [T]"""
    T, hop = f["T"], mp.hop
    S = f["fr"].abs().sum(1)
    if mp.preemph != 0.0 and f["idx"] is not None:
        px = (abs(mp.preemph) * x.double().abs())[f["idx"]]
        S_pre = (px.unfold(0, NFFT, hop)[:T] * f["w"].abs()).sum(1)
    else:
        S_pre = torch.zeros(T, dtype=F64)
    return U24 * (R_FWD * S + S_pre)


def forward_bounds(f, x, mp, tabs):
    """per cell [n_mels][T]: the output-domain bound (inf: none), r = d mel / (mel + eps), and the call's e_log"""
    d = spectrum_error(f, x, mp)[:, None]
    Xa, W = f["X"].abs(), f["W"]
    j, _ = geometry(mp, tabs)
    down = torch.zeros(mp.n_mels, NC + 1, dtype=F64)
    sel = (j >= 1) & (j <= mp.n_mels)
    down[j[sel] - 1, torch.arange(NC)[sel]] = 1.0
    dmel = (2 * Xa * d + d * d) @ W.t() + U24 * (G_BAND * f["mel"] + 2 * (f["P"] @ down.t()))
    a = f["mel"] + mp.log_eps
    r = dmel / a
    a32 = a.float()
    live = ~f["mask"]
    e_torch = float((torch.log(a32).double() - torch.log(a32.double())).abs()[live].max()) if bool(live.any()) else 0.0
    e_log = 4 * e_torch + U24
    lg = torch.log(a)
    bound = mp.out_scale * (torch.where(r < 1, -torch.log1p(-r.clamp(max=1 - 1e-16)), torch.full_like(r, math.inf)) + e_log) \
        + U24 * ((lg + mp.out_add).abs() * mp.out_scale + f["out"].t().abs())
    bound = torch.where(f["mask"], torch.zeros_like(bound), bound)
    return bound.t(), r.t(), e_log


def backward_bounds(bk, x, mp, tabs):
    """per sample [L]: the bound of dwave, from the f64 intermediates of `backward`"""
    T, hop, L = bk["T"], mp.hop, x.numel()
    Ly = L - 1
    d = spectrum_error(bk, x, mp)[:, None]
    _, r, _ = forward_bounds(bk, x, mp, tabs)
    r = r.t()
    W, Xa = bk["W"], bk["X"].abs()[:, :NC]
    dm = bk["dmel"].abs()
    e_dm = dm * (torch.where(r < 1, r / (1 - r.clamp(max=1 - 1e-16)), torch.full_like(r, math.inf)) + 5 * U24)
    e_dm = torch.where(dm == 0, torch.zeros_like(e_dm), e_dm)
    e_dP = (e_dm @ W + 3 * U24 * (dm @ W))[:, :NC]
    dPa, Ga = bk["dP"].abs()[:, :NC], bk["G"].abs()
    e_G = 2 * (dPa * d + e_dP * (Xa + d)) + 2 * U24 * Ga
    e_df = e_G.sum(1) + R_INV * U24 * Ga.sum(1)                        # [T], the same on every tap
    wa, ta = bk["w"].abs(), bk["tap"].abs()
    e_tap = wa[None, :] * e_df[:, None] + U24 * ta

    def oa(v):
        return torch.zeros(Ly + NFFT + hop, dtype=F64).index_add_(0, bk["q"], v.reshape(-1))[:Ly + NFFT]

    cover = oa(torch.ones(T, NFFT, dtype=F64))
    A_dyp = oa(ta)
    E_dyp = oa(e_tap) + U24 * cover * A_dyp

    def fold(v):
        return torch.zeros(Ly, dtype=F64).index_add_(0, bk["idx"], v)

    A_dy = fold(A_dyp)
    E_dy = fold(E_dyp) + 2 * U24 * A_dy
    z = torch.zeros(1, dtype=F64)
    pre = abs(mp.preemph)
    A_dw = torch.cat([z, A_dy]) + pre * torch.cat([A_dy, z])
    return torch.cat([z, E_dy]) + pre * torch.cat([E_dy, z]) + 2 * U24 * A_dw


def local_max(v, half=NC):
    """max |v| over the 1024 samples around every position"""
    return torch.nn.functional.max_pool1d(v.abs()[None, None], 2 * half + 1, 1, half)[0, 0]


def _rec(rec, group, **figs):
    if rec is not None:
        rec(group, **figs)


def usage(got, ref, bound):
    """largest |got - ref| / bound over the cells with a finite non-zero bound; NaN or inf in `got` gives inf"""
    if not bool(torch.isfinite(got).all()):
        return math.inf
    sel = torch.isfinite(bound) & (bound > 0)
    if not bool(sel.any()):
        return 0.0
    return float(((got.double() - ref).abs()[sel] / bound[sel]).max())


# ---- cases ---------------------------------------------------------------------------------------------------------------
class MC:
    """one call: a family, its parameters, the clips"""

    def __init__(self, fam, L, mp, clips, name=None, seed=0, dout="dense", ldw=None, lens=None, clip_tab=None):
        self.fam, self.L, self.mp, self.clips, self.seed, self.dout = fam, L, mp, tuple(clips), seed, dout
        self.ldw, self.lens, self.clip_tab = ldw, lens, clip_tab
        self.name = name or f"{fam}[hop{mp.hop},L{L},{mp.bank_name},{mp.window}]"

    @property
    def B(self):
        return len(self.clips)

    @property
    def T(self):
        return n_frames(self.L, self.mp.hop)


def impulse_positions(L, hop=320):
    """both ends, the reflect edges, each side of the forward tile boundary (frames 15 | 16) and of the backward workgroup boundary"""
    rows = bwd_rows(hop)
    t16 = FR * hop                                       # first padded position of frame 16; sample s sits at padded position s + 511
    cand = [0, 1, 511, 512, 513, L - 1, L - 2, L - 514, t16 - 512, t16 - 511, t16 - hop + 512, t16 - hop + 513,
            rows - 1, rows, rows + 1, 2 * rows - 1, 2 * rows, 2 * rows + 1]
    return sorted({s for s in cand if 0 <= s < L})


def impulse_wave(L, positions):
    w = torch.zeros(len(positions), L)
    w[torch.arange(len(positions)), torch.tensor(positions)] = 1.0
    return w


def tone_bins(mp, tabs):
    """first and last bin of a lane's run of eight, bins that open and close a triangle, bin 0, bin 511, bins below fmin and above
    fmax, the highest band's down-slope"""
    j, _ = geometry(mp, tabs)
    j = j.tolist()
    ks = {0, 511, 8, 15, 248, 255, 256, 263, 504}
    opens = [k for k in range(1, NC) if j[k] != j[k - 1] and 0 <= j[k] <= mp.n_mels]
    for k in opens[:2] + opens[len(opens) // 2:len(opens) // 2 + 2] + opens[-2:]:
        ks.update((k - 1, k))
    below = [k for k in range(NC) if j[k] < 0]
    above = [k for k in range(NC) if j[k] > mp.n_mels]
    top = [k for k in range(NC) if j[k] == mp.n_mels]
    for grp in (below, above, top):
        if grp:
            ks.update((grp[0], grp[-1]))
    return sorted(ks)


def tone_wave(L, bins):
    """x[n] = cos(2 pi k0 (n - 1) / 1024): with preemph = 0 the signal is y[i] = x[i + 1], even about i = 0, so the start reflection
    continues it; the end reflection does when L - 2 is a multiple of 512"""
    n = torch.arange(L, dtype=F64) - 1
    return torch.stack([torch.cos(2 * math.pi * k * n / NFFT) for k in bins]).float()


def graded(x, hop):
    """sample n times 2^((n div hop) mod 7 - 3): exact scalings, frame t of the signal is one of seven magnitudes"""
    return x * 2.0 ** ((torch.arange(x.shape[-1]) // hop) % 7 - 3).float()


GRADED_AMP = 2.0 ** -13


def graded_noise(B, L, seed, hop, amp=GRADED_AMP):
    """Uniform noise in +-amp, graded per hop.  The amplitude is what makes `no bound above 1e-4` possible at the shipped log_eps:
    for a one-bin band 2 |X| d_t / (|X|^2 + eps) <= d_t / sqrt(eps) whatever |X| is, so the Rayleigh nulls of a noise spectrum stay
    tight as long as d_t = R u sum|f| is small against sqrt(eps) = 3.2e-3; amp = 2^-13 keeps sum|f| of the loudest frames near 0.25
    (mel there is 10 to 100 eps, in the quietest frames eps / 40).  At amplitude 1 (`loud`) 3 % of the cells are loose, whatever the
    seed: |X_k| < 0.17 sigma happens that often."""
    g = torch.Generator().manual_seed(seed)
    return graded((torch.rand(B, L, generator=g) * 2 - 1) * amp, hop)


def case_wave(c):
    if c.fam == "impulse":
        return impulse_wave(c.L, c.clips)
    if c.fam == "tone":
        return tone_wave(c.L, c.clips)
    if c.fam == "graded":
        return graded_noise(c.B, c.L, c.seed, c.mp.hop)
    if c.fam == "loud":
        return graded_noise(c.B, c.L, c.seed, c.mp.hop, 1.0)
    if c.fam == "zero":
        return torch.zeros(c.B, c.L)
    raise ValueError(c.fam)


# parameters of the families.  impulse: log_eps = 2^-7 -- a two-term frame has |X_k| = |a + b e^(-i phi k)| anywhere in [|a - b|, a + b];
# the bound 2 |X| d / (|X|^2 + eps) peaks at d / sqrt(eps) = 2 R u (a + b) / sqrt(eps) = 9e-5 for a = b = 1 before out_scale.
# tone: log_eps = 1, out_add = 0, out_scale = 1 -- the bands the tone does not reach hold rounding noise of at most d_t^2 per bin,
# which a small eps would turn into a loose cell; with eps = 1 the masked / empty cells are log(1) = 0.
def mp_impulse(window, **kw):
    return MP(preemph=0.0, log_eps=2.0 ** -7, window=window, **kw)


def mp_tone(**kw):
    return MP(preemph=0.0, log_eps=1.0, out_add=0.0, out_scale=1.0, window="rect", **kw)


TONE_L = 2050
HOPS = (320, 160, 100, 333, 748, 752, 1024, 7)
FWD_LENGTHS_320 = (514, 515, 700, 1025, 1537, 4800, 5120, 5121, 10436, 10437, 10440)


def hop_length(hop):
    """the shortest length at which the second forward tile of this hop is an interior one (a multiple of 4 where the hop allows it)"""
    span = (FR - 1) * hop + NFFT
    L = FR * hop - NC + span + 4 + 1
    return -(-L // 4) * 4


def forward_cases():
    cs = []
    for i, L in enumerate(FWD_LENGTHS_320):                # hop 320: every length, impulse family with both windows
        win = ("rect", "hann")[i & 1]
        masks = dict(fmask=(3, 9), tmask=(-2, 1)) if i % 3 == 0 else dict(fmask=(0, 0), tmask=(0, 0)) if i % 3 == 1 else dict(fmask=(120, 128), tmask=(2, 10 ** 6))
        cs.append(MC("impulse", L, mp_impulse(win, **masks), impulse_positions(L)))
    for hop in HOPS[1:]:                                   # every other hop: two tiles, the second interior where the hop allows
        L = hop_length(hop) if hop > 7 else 1300
        cs.append(MC("impulse", L, mp_impulse("hann" if hop % 2 else "rect", hop=hop), impulse_positions(L, hop)))
        cs.append(MC("graded", L, MP(hop=hop), range(2), seed=hop))
    for bk in BANKS:                                       # tones through every filterbank
        mp = mp_tone(bank_name=bk)
        cs.append(MC("tone", TONE_L, mp, tone_bins(mp, tables("rect"))))
    for L in (10440, 10437, 5121, 700):                    # the shipped parameters: graded noise, and the same at amplitude 1
        cs.append(MC("graded", L, MP(fmask=(40, 52), tmask=(5, 9)), range(3), seed=L))
        cs.append(MC("loud", L, MP(), range(2), seed=L + 1))
    for bk in ("m64", "m5", "m4", "low128"):
        cs.append(MC("graded", 5121, MP(bank_name=bk, fmask=(0, 1)), range(2), seed=len(bk)))
    cs.append(MC("graded", 700, MP(fmask=(0, 128)), range(2), seed=9, name="graded[all masked]"))
    return cs


BWD_LENGTHS_320 = (5119, 5120, 5121, 10239, 10240, 10241, 514, 515, 700, 1025, 1537)


def onehot_cells(L, mp):
    """frames straddling a workgroup's rows boundary, at the clip start and at the clip end; a low, a middle and the top band"""
    T, rows = n_frames(L, mp.hop), bwd_rows(mp.hop)
    ts = {0, 1, T - 1, max(T - 2, 0)}
    for n0 in range(rows, L, rows):
        q = n0 - 1 + NC                                    # first padded position of the run that starts at n0
        ts.update(t for t in ((q - 1) // mp.hop, (q - 1) // mp.hop - 1, q // mp.hop + 1) if 0 <= t < T)
    bands = (0, mp.n_mels // 2, mp.n_mels - 1)
    return [(bands[i % 3], t) for i, t in enumerate(sorted(ts))]


def backward_cases():
    cs = []
    for i, L in enumerate(BWD_LENGTHS_320):
        cs.append(MC("graded", L, MP(fmask=(40, 52), tmask=(-3, 2) if i & 1 else (4, 6)), range(2), seed=100 + L, dout="dense"))
        mp = MP(preemph=0.5, log_eps=2.0 ** -7, window="rect", bank_name=("shipped", "m64", "m5")[i % 3])
        cells = onehot_cells(L, mp)
        cs.append(MC("graded", L, mp, range(len(cells)), seed=200 + L, dout=cells))
    for hop in HOPS[1:]:
        rows = bwd_rows(hop)
        for L in ((rows + 1, 2 * rows - 1) if rows <= 6000 else (rows + 1,)):
            cs.append(MC("graded", L, MP(hop=hop), range(2), seed=300 + hop, dout="dense"))
        mp = MP(hop=hop, preemph=0.5, log_eps=2.0 ** -7, window="hann")
        cells = onehot_cells(rows + 2, mp)[:6]
        cs.append(MC("graded", rows + 2, mp, range(len(cells)), seed=400 + hop, dout=cells))
    for bk in ("m64", "m4", "low128"):
        cs.append(MC("loud", 5121, MP(bank_name=bk), range(2), seed=500, dout="dense"))
    cs.append(MC("graded", 5121, MP(fmask=(10, 20), tmask=(3, 8)), range(2), seed=600, dout="nan_masked"))
    return cs


# packed batches: (hop, ldw, lens): full, short and too-short rows in more than one order; 10437 | 10436 are either side of the
# interior test of the second tile, which a packed row reaches because the pitch, not the length, has to be a multiple of four
PACKED = ((320, 10440, (10440, 700, 513, 10437)),
          (320, 10441, (514, 10436, 300, 10441)),
          (320, 10442, (300, 10437, 1025, 5121, 10442)),
          (320, 10443, (10443, 0, 1537, 515)),
          (100, 6004, (5913, 6004, 512, 2500)),
          (333, 7000, (6999, 1, 7000)))


def packed_clip_table(mp, lens):
    """every clip its own filterbank edges and mask bands; empty masks, a negative start and an end past T among them"""
    rows = []
    for b, L in enumerate(lens):
        lo, inv = bank(mp.n_mels, 10.0 * b, 15500.0 - 700.0 * b)
        T = n_frames(L, mp.hop)
        rows.append((lo, inv, 3 * b, (3 * b + 7 * (b % 3)) if b != 1 else 0, (-2, 3, T - 2, 0)[b % 4], (1, 3, T + 5, 0)[b % 4]))
    return rows


def packed_cases():
    cs = []
    for hop, ldw, lens in PACKED:
        cs.append(MC("graded", ldw, MP(hop=hop, tmask=(1, 3)), range(len(lens)), seed=ldw, ldw=ldw, lens=lens, name=f"packed[hop{hop},ldw{ldw}]"))
        cs.append(MC("graded", ldw, MP(hop=hop), range(len(lens)), seed=ldw + 1, ldw=ldw, lens=lens, clip_tab=packed_clip_table(MP(hop=hop), lens),
                     name=f"packed_aug[hop{hop},ldw{ldw}]"))
    return cs


def packed_impulse_case():
    """the last valid sample of a short clip whose row continues with NaN, and the samples around it"""
    lens = (10440, 700, 5121, 1537, 700, 5121, 1537)
    return MC("impulse", 10440, mp_impulse("rect"), [l - 1 - (b > 3) - 512 * (b > 5) for b, l in enumerate(lens)], ldw=10440, lens=lens, name="packed_impulse")


def persist_lds(hop, n_mels):
    span = (FR_PERSIST - 1) * hop + NFFT
    return 2 * (((span + 4) * 4 + 1023) & ~1023) + 4 * 4608 + max(n_mels * (FR_PERSIST + 1) * 4, 2 * NC * 4)


def persist_cases(cus):
    """fixed-length forward cases for PA_MEL_PERSIST=1 (even hops take the persistent form): short clips, both staging forms, and one
    call with more tiles than resident workgroups, so that a workgroup walks from the last tile of one clip into the next clip"""
    cs = [c for c in forward_cases() if c.mp.hop % 2 == 0 and (c.L <= 5121 or c.L == 10440 or c.mp.hop != 320)]
    resident = cus * max(1, 160 * 1024 // persist_lds(100, 128))
    L = 40000
    tiles = -(-n_frames(L, 100) // FR_PERSIST)
    B = -(-resident // tiles) + 3
    cs.append(MC("graded", L, MP(hop=100), range(B), seed=77, name=f"persist_walk[B{B}]"))
    cs.append(MC("graded", L + 2, MP(hop=100), range(2), seed=78, name="persist_lanes"))
    return cs


# ---- which staging path a case reaches (the predicates of mel.hip, from the case alone) ----------------------------------
def fwd_paths(hop, L, Lp=None, fr=FR, persist=False):
    Lp = L if Lp is None else Lp
    span, got = (fr - 1) * hop + NFFT, set()
    if L - 1 <= NC:
        return got
    for f0 in range(0, n_frames(L, hop), fr):
        i0 = f0 * hop - NC
        interior = i0 >= 0 and i0 + span + 4 <= L - 1 and ((i0 | Lp) & 3) == 0
        if persist:
            got.add("dma" if interior else "lanes")
        else:
            got.add("vec16" if interior and span % 4 == 0 and span <= VEC_CAP else "scalar")
    return got


def bwd_paths(hop, L, Lp=None, b=0):
    Lp = L if Lp is None else Lp
    got = set()
    if L - 1 <= NC:
        return got
    for t in range(n_frames(L, hop)):
        i0 = t * hop - NC
        got.add("aligned" if i0 >= 0 and i0 + NFFT + 1 <= L - 1 and ((b * Lp + i0) & 1) == 0 else "reflected")
    return got


def bwd_workgroups(hop, L):
    return -(-L // bwd_rows(hop))


# ---- checkers ------------------------------------------------------------------------------------------------------------
def zero_cells(impl, mp, tabs):
    """what the implementation itself returns for silence: one column [n_mels] (masks off)"""
    q = mp.with_clip((mp.mel_low, mp.inv_mel_delta, 0, 0, 0, 0))
    rc, out = impl.fwd(torch.zeros(1, 700), tabs, q)
    assert rc == PA_OK
    col = out[0, :, 0]
    assert torch.equal(out[0], col[:, None].expand_as(out[0]))
    return col


def check_forward_rows(impl, c, wave, out, rec=None, lens=None, clip_tab=None, zero=None):
    """rows of `out` against the f64 reference: masked cells exactly the constant, silent frames bit-equal to the cells of an all-zero
    clip, every other cell inside its bound.  Returns (worst usage, loose cells, live cells)."""
    tabs = tables(c.mp.window)
    worst, loose, live = 0.0, 0, 0
    for b in range(out.shape[0]):
        L = c.L if lens is None else lens[b]
        if L - 1 <= NC:
            continue
        mp = c.mp.with_clip(clip_tab[b]) if clip_tab else c.mp
        x = wave[b, :L].double()
        f = REF.forward(x, L, mp, tabs)
        T = f["T"]
        got, ref = out[b, :, :T], f["out"]
        bound, _, _ = forward_bounds(f, x, mp, tabs)
        mask = f["mask"].t()
        assert torch.equal(got[mask], torch.full_like(got[mask], mp.mask_const())), f"{c.name} clip {b}: a masked cell is not (0 + out_add) out_scale"
        # silent: the frame is all zero, or the band holds no bin -- the band sum is exactly 0 in any implementation
        silent = ((f["fr"].abs().sum(1) == 0)[None, :] | ((f["W"].abs().sum(1) == 0)[:, None])) & ~mask
        if bool(silent.any()):
            z = zero_cells(impl, mp, tabs) if zero is None or clip_tab else zero
            want = z[:, None].expand(-1, T)
            assert torch.equal(got[silent], want[silent]), f"{c.name} clip {b}: a silent frame differs from the cells of an all-zero clip"
        sel = ~mask & ~silent
        assert bool(torch.isfinite(got).all()), f"{c.name} clip {b}: NaN or inf in the result"
        bad = sel & torch.isfinite(bound) & ((got.double() - ref).abs() > bound)
        if bool(bad.any()):
            i = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{c.name} clip {b} cell (band {i[0]}, frame {i[1]}): got {float(got[i[0], i[1]])!r}, reference "
                                 f"{float(ref[i[0], i[1]])!r}, bound {float(bound[i[0], i[1]]):.3e}; {int(bad.sum())} cells outside")
        worst = max(worst, usage(got[sel], ref[sel], bound[sel]))
        loose += int((bound[sel] > LOOSE).sum())
        live += int(sel.sum())
    _rec(rec, f"fwd.{c.fam}", usage=worst, loose=loose, live=live)
    return worst, loose, live


def check_forward(impl, c, rec=None):
    tabs = tables(c.mp.window)
    wave = case_wave(c)
    rc, out = impl.fwd(wave, tabs, c.mp)
    assert rc == PA_OK, (c.name, rc)
    assert out.shape == (c.B, c.mp.n_mels, c.T)
    zero = zero_cells(impl, c.mp, tabs)
    return check_forward_rows(impl, c, wave, out, rec, zero=zero)


def case_dout(c, T=None, lens=None):
    """dense: graded per frame; one-hot cells: clip b has the single cell c.dout[b]; nan_masked: dense with NaN at every masked cell"""
    T = c.T if T is None else T
    g = torch.Generator().manual_seed(c.seed + 7)
    if isinstance(c.dout, str):
        d = (torch.rand(c.B, c.mp.n_mels, T, generator=g) * 2 - 1) * 2.0 ** ((torch.arange(T) % 5) - 2).float()
        if c.dout == "nan_masked":
            d[:, REF.mask(c.mp, T).t()] = float("nan")
        return d
    d = torch.zeros(c.B, c.mp.n_mels, T)
    for b, (band, t) in enumerate(c.dout):
        d[b, band, t] = 1.0 + 0.25 * b
    return d


def check_backward_rows(impl, c, wave, dout, dw, rec=None, lens=None, clip_tab=None):
    tabs = tables(c.mp.window)
    worst, worst_local, support = 0.0, 0.0, []
    for b in range(dw.shape[0]):
        L = c.L if lens is None else lens[b]
        row = dw[b]
        if L - 1 <= NC:
            assert torch.equal(row, torch.zeros_like(row)), f"{c.name} clip {b}: a too-short clip's gradient is not 0 throughout"
            continue
        assert torch.equal(row[L:], torch.zeros_like(row[L:])), f"{c.name} clip {b}: dwave is not exactly 0 at and behind the clip's end"
        mp = c.mp.with_clip(clip_tab[b]) if clip_tab else c.mp
        x = wave[b, :L].double()
        T = n_frames(L, mp.hop)
        g = dout[b, :, :T]
        ref = ref_backward_autograd(x, L, mp, tabs, g)
        bk = REF.backward(x, L, mp, tabs, torch.nan_to_num(g.double()))
        bound = backward_bounds(bk, x, mp, tabs)
        got = row[:L]
        assert bool(torch.isfinite(got).all()), f"{c.name} clip {b}: NaN or inf in dwave (a guard, or an upstream value at a masked cell, was read)"
        off = bound == 0
        assert torch.equal(got[off], torch.zeros_like(got[off])), f"{c.name} clip {b}: dwave is not exactly 0 outside the support of dout"
        bad = torch.isfinite(bound) & ((got.double() - ref).abs() > bound)
        if bool(bad.any()):
            n = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{c.name} clip {b} sample {n}: got {float(got[n])!r}, reference {float(ref[n])!r}, bound {float(bound[n]):.3e}; "
                                 f"{int(bad.sum())} samples outside")
        worst = max(worst, usage(got, ref, bound))
        lm = local_max(ref)
        sel = lm > 0
        if bool(sel.any()):
            worst_local = max(worst_local, float(((got.double() - ref).abs()[sel] / lm[sel]).max()))
        support.append(int((~off).sum()))
    _rec(rec, f"bwd.{c.fam}.{'dense' if isinstance(c.dout, str) else 'onehot'}", usage=worst, local_rel=worst_local)
    return worst, worst_local, support


def check_backward(impl, c, rec=None):
    tabs = tables(c.mp.window)
    wave, dout = case_wave(c), case_dout(c)
    rc, dw = impl.bwd(wave, tabs, c.mp, dout)
    assert rc == PA_OK, (c.name, rc)
    assert dw.shape == wave.shape
    return check_backward_rows(impl, c, wave, dout, dw, rec)


def packed_wave(c):
    """[B][ldw]: clip b in its first lens[b] samples, NaN behind them"""
    wave = case_wave(c)
    for b, L in enumerate(c.lens):
        wave[b, L:] = float("nan")
        if c.fam == "impulse":
            wave[b, :L] = 0
            if L > 0:
                wave[b, c.clips[b]] = 1.0
    return wave


def check_packed(impl, c, rec=None, backward=True):
    """the packed entries (with the per-clip table: the _aug ones): every row equals the clip transformed alone through the
    fixed-length entry bit for bit, `fill` behind its frames, `fill` / 0 throughout for a too-short row, and meets the bounds"""
    tabs, mp, hop = tables(c.mp.window), c.mp, c.mp.hop
    wave = packed_wave(c)
    T_max = max(n_frames(L, hop) for L in c.lens if L - 1 > NC)
    assert T_max <= n_frames(c.ldw, hop)
    rc, out = impl.fwd_varlen(wave, c.lens, tabs, mp, T_max, FILL, c.clip_tab)
    assert rc == PA_OK, (c.name, rc)
    assert out.shape == (c.B, mp.n_mels, T_max)
    dout = case_dout(c, T_max)
    for b, L in enumerate(c.lens):
        T = n_frames(L, hop) if L - 1 > NC else 0
        assert torch.equal(out[b, :, T:], torch.full_like(out[b, :, T:], FILL)), f"{c.name} clip {b}: the columns behind the clip's frames are not `fill`"
        dout[b, :, T:] = float("nan")                                        # never read, says the header
    check_forward_rows(impl, c, wave, out, rec, lens=c.lens, clip_tab=c.clip_tab)
    alone = {}
    for b, L in enumerate(c.lens):
        if L - 1 <= NC:
            continue
        q = mp.with_clip(c.clip_tab[b]) if c.clip_tab else mp
        T = n_frames(L, hop)
        rc1, o1 = impl.fwd(wave[b:b + 1, :L].contiguous(), tabs, q)
        assert rc1 == PA_OK
        assert torch.equal(out[b, :, :T], o1[0]), f"{c.name} clip {b}: the packed row differs from the clip transformed alone"
        alone[b] = q
    if not backward:
        return
    rc, dw = impl.bwd_varlen(wave, c.lens, tabs, mp, dout, T_max, c.clip_tab)
    assert rc == PA_OK, (c.name, rc)
    check_backward_rows(impl, c, wave, dout, dw, rec, lens=c.lens, clip_tab=c.clip_tab)
    for b, q in alone.items():
        L = c.lens[b]
        T = n_frames(L, hop)
        rc1, d1 = impl.bwd(wave[b:b + 1, :L].contiguous(), tabs, q, dout[b:b + 1, :, :T].contiguous())
        assert rc1 == PA_OK
        assert torch.equal(dw[b, :L], d1[0]), f"{c.name} clip {b}: the packed gradient differs from the clip's own"


def check_impulse_closed_form(c):
    """the reference against the family's closed form: a frame one tap i of which holds the sample has |X[k]|^2 = w[i]^2 in every bin,
    a frame that also holds its mirror image |w[i] + w[i'] exp(-2 pi i k (i' - i) / 1024)|^2"""
    tabs, mp = tables(c.mp.window), c.mp
    w = tabs["window"].double()
    k = torch.arange(NC, dtype=F64)
    for b, s in enumerate(c.clips):
        x = impulse_wave(c.L, [s])[0].double()
        f = REF.forward(x, c.L, mp, tabs)
        hits = torch.nonzero(f["idx"] == s - 1)[:, 0].tolist() if s >= 1 else []
        for t in range(f["T"]):
            taps = [q - t * mp.hop for q in hits if 0 <= q - t * mp.hop < NFFT]
            assert len(taps) <= 2
            X = sum((w[i] * torch.exp(-2j * math.pi * k * i / NFFT) for i in taps), torch.zeros(NC, dtype=torch.complex128))
            assert float((f["P"][t, :NC] - X.abs() ** 2).abs().max()) < 1e-12, (c.name, s, t)


# ---- the old criterion ---------------------------------------------------------------------------------------------------
def old_criterion_accepts(impl):
    """whole-tensor max |got - ref| < 1e-3 on a second of uniform noise at the shipped parameters, forward and (per clip, relative to
    the largest |dwave|) backward: what tests/test_gpu_model.py and tests/test_gpu_wave_grad.py ask of the front end"""
    g = torch.Generator().manual_seed(4242)
    wave = (torch.rand(2, 32000, generator=g) * 2 - 1) * 0.2
    mp, tabs = MP(tmask=(20, 60), fmask=(30, 50)), tables("hann800")
    try:
        _, out = impl.fwd(wave, tabs, mp)
        dout = torch.rand(2, 128, n_frames(32000, 320), generator=g) - 0.5
        _, dw = impl.bwd(wave, tabs, mp, dout)
    except Exception:
        return False
    for b in range(2):
        x = wave[b].double()
        ref = REF.forward(x, 32000, mp, tabs)["out"]
        if not float((out[b].double() - ref).abs().max()) < 1e-3:
            return False
        rdw = ref_backward_autograd(x, 32000, mp, tabs, dout[b])
        if not float((dw[b].double() - rdw).abs().max() / rdw.abs().max()) < 1e-3:
            return False
    return True


# ---- argument checks -----------------------------------------------------------------------------------------------------
ENTRIES = ("fwd", "fwd_varlen", "fwd_varlen_aug", "bwd", "bwd_varlen", "bwd_varlen_aug")
ARG_L = 2000
# (name, what to change in the valid call, expected code).  Pointers are named as in the header; `skip`: entries without that argument.
ARG_FAULTS = (
    ("wave NULL", dict(null="wave"), PA_EINVAL), ("window NULL", dict(null="window"), PA_EINVAL), ("bin_mel NULL", dict(null="bin_mel"), PA_EINVAL),
    ("twiddle NULL", dict(null="twiddle"), PA_EINVAL), ("out / dwave NULL", dict(null="result"), PA_EINVAL), ("params NULL", dict(null="p"), PA_EINVAL),
    ("dout NULL", dict(null="dout"), PA_EINVAL), ("lens NULL", dict(null="lens"), PA_EINVAL), ("clip NULL", dict(null="clip"), PA_EINVAL),
    ("B = 0", dict(B=0), PA_EINVAL),
    ("n_fft = 512", dict(n_fft=512), PA_EUNSUPPORTED), ("n_fft = 2048", dict(n_fft=2048), PA_EUNSUPPORTED),
    ("n_mels = 3", dict(n_mels=3), PA_EUNSUPPORTED), ("n_mels = 129", dict(n_mels=129), PA_EUNSUPPORTED),
    ("hop = 0", dict(hop=0), PA_EUNSUPPORTED), ("hop = 1025", dict(hop=1025), PA_EUNSUPPORTED), ("hop = -320", dict(hop=-320), PA_EUNSUPPORTED),
    ("L = 513", dict(L=513), PA_EUNSUPPORTED), ("L = 1", dict(L=1), PA_EUNSUPPORTED),
    ("n_frames + 1", dict(dframes=1), PA_EINVAL), ("n_frames - 1", dict(dframes=-1), PA_EINVAL),
    ("T_max = 0", dict(T_max=0), PA_EINVAL), ("T_max beyond ldw", dict(T_max_extra=1), PA_EINVAL),
    ("wave 4 bytes off 16-byte alignment", dict(misalign=1), PA_EINVAL), ("wave 8 bytes off 16-byte alignment", dict(misalign=2), PA_EINVAL),
)

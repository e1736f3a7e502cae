#!/usr/bin/env python
"""CPU emulation of the two stages of mel_frontend_bwd_kernel (csrc/mel.hip) that are not the forward's own code run again
(the companion of tools/emulate_mel_bands.py, which is the forward's band stage):

  * the band transpose: dP[k] = u_k dmel[j_k] + (1 - u_k) dmel[j_k - 1], a two-term gather through a zero-padded copy of dmel
    (no filterbank matrix), checked against the dense kaldi filterbank transposed;
  * the one-sided inverse: df[i] = Re sum_{k=0}^{511} G[k] exp(+2 pi i k i / 1024) from ONE 512-point complex transform.  With
    c[n] = df[2n] + i df[2n+1] the spectrum of c is
        H[k] = (G[k] + conj G[512-k]) / 2 + i conj(W^k) (G[k] - conj G[512-k]) / 2      (k = 1..511, W = exp(-2 pi i / 1024))
        H[0] = Re G[0] (1 + i)
    and c = conj(DFT512(conj H)): the forward's radix-8 transform, unchanged, between two conjugations.  No 1/N and no Hermitian
    doubling: this is the adjoint of the forward's one-sided sum, not irfft.

    python tools/emulate_mel_bwd.py        # prints the two residuals and exits non-zero if either is above 1e-12
"""
import sys

import numpy as np

NFFT, NC = 1024, 512


def band_transpose(dmel, j, u, n_mels):
    """dmel [n_mels], j [512] triangle index of bin k (any integer), u [512] up-slope weight -> dP [512]."""
    pad = np.zeros(n_mels + 4)
    pad[2:2 + n_mels] = dmel                                 # pad[x + 2] = dmel[x], zero outside [0, n_mels)
    jc = np.clip(j, -1, n_mels + 1)
    return u * pad[jc + 2] + (1.0 - u) * pad[jc + 1]


def one_sided_inverse(G):
    """G [512] complex (bins 0..511) -> df [1024] real."""
    k = np.arange(NC)
    Gc = np.conj(G[(NC - k) % NC])
    cw = np.exp(2j * np.pi * k / NFFT)                        # conj(W^k)
    H = 0.5 * (G + Gc) + 0.5j * cw * (G - Gc)
    H[0] = G[0].real * (1 + 1j)
    c = np.conj(np.fft.fft(np.conj(H)))
    df = np.empty(NFFT)
    df[0::2], df[1::2] = c.real, c.imag
    return df


def main():
    rng = np.random.default_rng(0)
    worst = 0.0
    for n_mels, fmin, fmax in ((128, 0.0, 15000.0), (40, 300.0, 7000.0), (8, 2000.0, 2600.0)):
        kk = np.arange(NC)
        bin_mel = 1127.0 * np.log1p(kk * (32000 / NFFT) / 700.0)
        lo, hi = 1127.0 * np.log1p(fmin / 700.0), 1127.0 * np.log1p(fmax / 700.0)
        t = (bin_mel - lo) * (n_mels + 1) / (hi - lo)
        j = np.floor(t).astype(np.int64)
        u = t - np.floor(t)
        basis = np.zeros((n_mels, NC))                        # band b: up-slope on triangle b, down-slope on triangle b + 1
        for k in range(NC):
            if 0 <= j[k] < n_mels:
                basis[j[k], k] += u[k]
            if 1 <= j[k] <= n_mels:
                basis[j[k] - 1, k] += 1.0 - u[k]
        dmel = rng.standard_normal(n_mels)
        e = np.abs(band_transpose(dmel, j, u, n_mels) - basis.T @ dmel).max()
        worst = max(worst, e)
        print(f"band transpose, {n_mels:3d} bands [{fmin:.0f}, {fmax:.0f}] Hz: max abs residual {e:.2e}")
    G = rng.standard_normal(NC) + 1j * rng.standard_normal(NC)
    G[0] = G[0].real                                          # X[0] is real in the forward
    i = np.arange(NFFT)
    want = np.real(np.exp(2j * np.pi * np.outer(i, np.arange(NC)) / NFFT) @ G)
    e = np.abs(one_sided_inverse(G) - want).max() / np.abs(want).max()
    worst = max(worst, e)
    print(f"one-sided inverse through one 512-point transform: max rel residual {e:.2e}")
    return 0 if worst < 1e-12 else 1


if __name__ == "__main__":
    sys.exit(main())

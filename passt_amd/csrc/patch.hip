// Patch embedding around the im2col GEMM: gather of the kept patches, positional table, prefix
// tokens, and the backward reductions.  Reference: PatchEmbed.forward (models/passt.py:318-328) and
// PaSST.forward_features :508-564.  "Gather first": Patchout indices (drawn on the host with the
// reference's own torch CPU RNG calls) select the patches BEFORE the projection, so only
// (F-s_f)(T-s_t)-u of the F*T patches are ever embedded.
#include <algorithm>

#include "pa_common.h"

namespace pa {

// one workgroup (P*P threads) per kept patch: cols[(b*Np+p)][i*P+j] = x[b][f*fs+i][t*ts+j]
template <typename T>
__global__ void patch_gather_kernel(const float* __restrict__ x, int F, int Tt, const int32_t* __restrict__ pf,
                                    const int32_t* __restrict__ pt, int Np, int P, int fs, int ts, T* __restrict__ cols) {
    const int p = blockIdx.x, b = blockIdx.y;
    const int i = threadIdx.x / P, j = threadIdx.x % P;
    const int f = pf[p] * fs + i, t = pt[p] * ts + j;
    const float v = x[((int64_t)b * F + f) * Tt + t];
    cols[((int64_t)b * Np + p) * (P * P) + threadIdx.x] = from_f32<T>(v);
}

__global__ void patch_pos_table_kernel(const float* __restrict__ bias, const float* __restrict__ tpos, int Tpe,
                                       const float* __restrict__ fpos, int Fpe, const int32_t* __restrict__ pf,
                                       const int32_t* __restrict__ pt, int Np, int toff, int D, float* __restrict__ table,
                                       const float* __restrict__ cls, const float* __restrict__ dist,
                                       const float* __restrict__ npe, float* __restrict__ tok, int B, int Ntok) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n_table = (int64_t)Np * D, n_tok = (int64_t)B * 2 * D;
    if (i < n_table) {
        const int p = (int)(i / D), d = (int)(i % D);
        table[i] = bias[d] + tpos[(int64_t)d * Tpe + toff + pt[p]] + fpos[(int64_t)d * Fpe + pf[p]];
    } else if (i < n_table + n_tok) {
        const int64_t k = i - n_table;
        const int b = (int)(k / (2 * D)), r = (int)((k / D) % 2), d = (int)(k % D);
        tok[((int64_t)b * Ntok + r) * D + d] = (r == 0 ? cls[d] : dist[d]) + npe[r * D + d];
    }
}

// ---- packed batch of clips of different lengths (eval forward) --------------------------------------------------------------
// Token row r of the packed [M][.] matrices belongs to clip row_clip[r]; row_f[r] >= 0: the patch at grid position (row_f, row_t) of
// that clip; row_f[r] < 0: a prefix token (row_t = 0: cls, 1: dist).  cols gets a zero row under every prefix token, the table the
// token itself, so ONE patch GEMM with the residual epilogue (rrow = orow = m) writes the whole token matrix: 0 * W + table.
// one workgroup (P*P threads) per token row: cols[r][i*P+j] = x[clip][f*fs+i][t*ts+j]
template <typename T>
__global__ void patch_gather_varlen_kernel(const float* __restrict__ x, int B, int F, int Tt, const int32_t* __restrict__ row_clip,
                                           const int32_t* __restrict__ row_f, const int32_t* __restrict__ row_t, int P, int fs, int ts,
                                           T* __restrict__ cols) {
    const int r = blockIdx.x;
    const int i = threadIdx.x / P, j = threadIdx.x % P;
    const int c = row_clip[r], pf = row_f[r];
    float v = 0.f;
    if (pf >= 0) {
        const int f = pf * fs + i, t = row_t[r] * ts + j;
        if ((unsigned)c < (unsigned)B && f < F && (unsigned)t < (unsigned)Tt) v = x[((int64_t)c * F + f) * Tt + t];
    }
    cols[(int64_t)r * (P * P) + threadIdx.x] = from_f32<T>(v);
}

// table[r][d] = bias[d] + tpos[d][row_t] + fpos[d][row_f] (the time embedding is read from offset 0: eval mode), or the prefix
// token + its position row
__global__ void patch_pos_table_varlen_kernel(const float* __restrict__ bias, const float* __restrict__ tpos, int Tpe,
                                              const float* __restrict__ fpos, int Fpe, const int32_t* __restrict__ row_f,
                                              const int32_t* __restrict__ row_t, int M, int D, float* __restrict__ table,
                                              const float* __restrict__ cls, const float* __restrict__ dist,
                                              const float* __restrict__ npe) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)M * D) return;
    const int r = (int)(i / D), d = (int)(i % D);
    const int pf = row_f[r], pt = row_t[r];
    if (pf < 0) table[i] = (pt == 0 ? cls[d] : dist[d]) + npe[(pt == 0 ? 0 : 1) * D + d];
    else table[i] = bias[d] + tpos[(int64_t)d * Tpe + min(pt, Tpe - 1)] + fpos[(int64_t)d * Fpe + min(pf, Fpe - 1)];
}

// gsum[n][d] = sum_b dtok[b][n][d]: 16 bytes per thread, four clips in flight (round 5: the scalar one-clip-at-a-time loop ran
// at 2.9 TB/s)
__global__ __launch_bounds__(256) void batch_sum_kernel(const float* __restrict__ dtok, int B, int64_t per, float* __restrict__ gsum) {
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= per) return;
    if (((per | i) & 3) == 0) {
        float4 s0 = make_float4(0, 0, 0, 0), s1 = s0, s2 = s0, s3 = s0;
        auto acc = [](float4& s, const float4& v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; };
        int b = 0;
        for (; b + 4 <= B; b += 4) {
            const float4 v0 = *(const float4*)(dtok + (int64_t)b * per + i), v1 = *(const float4*)(dtok + (int64_t)(b + 1) * per + i);
            const float4 v2 = *(const float4*)(dtok + (int64_t)(b + 2) * per + i), v3 = *(const float4*)(dtok + (int64_t)(b + 3) * per + i);
            acc(s0, v0); acc(s1, v1); acc(s2, v2); acc(s3, v3);
        }
        for (; b < B; ++b) acc(s0, *(const float4*)(dtok + (int64_t)b * per + i));
        acc(s0, s1); acc(s2, s3); acc(s0, s2);
        *(float4*)(gsum + i) = s0;
        return;
    }
    for (int64_t k = i; k < per && k < i + 4; ++k) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dtok[(int64_t)b * per + k];
        gsum[k] = s;
    }
}

// Parameter gradients of the patch stage from gsum[2 + Np][D]: conv bias (all patches), time / frequency position embeddings
// (the patches of one time / frequency slot), cls / dist tokens and their position rows.  Workgroup = one slot x 16 channels
// x 16 patch groups: every thread scans Np / 16 patches for its slot (the test is uniform over the 16 channel lanes) and the
// partial sums meet in LDS.  (Round 5: one thread per (slot, channel) walking all Np patches was 48 us -- 472 dependent
// L2 round trips on three workgroups for the bias, ~40 per thread for a frequency slot.)
__global__ __launch_bounds__(256) void patch_param_grads_kernel(const float* __restrict__ gsum, int D, const int32_t* __restrict__ pf,
                                         const int32_t* __restrict__ pt, int Np, int toff, int Tpe, int Fpe,
                                         float* __restrict__ d_cls, float* __restrict__ d_dist, float* __restrict__ d_npe,
                                         float* __restrict__ d_bias, float* __restrict__ d_tpos, float* __restrict__ d_fpos,
                                         int accumulate) {
    __shared__ float red[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int slot = blockIdx.y;                       // 0: bias + prefix tokens; 1 .. Tpe: time; Tpe + 1 .. Tpe + Fpe: frequency
    const int d = blockIdx.x * 16 + cx;
    auto put = [&](float* p, float v) { *p = (accumulate ? *p : 0.f) + v; };
    const int32_t* key = slot == 0 ? nullptr : (slot <= Tpe ? pt : pf);
    const int want = slot == 0 ? 0 : (slot <= Tpe ? slot - 1 - toff : slot - 1 - Tpe);
    float s0 = 0.f, s1 = 0.f;
    if (d < D) {
        int p = ry;
        for (; p + 16 < Np; p += 32) {                 // two patches per step: two loads in flight
            const bool m0 = !key || key[p] == want, m1 = !key || key[p + 16] == want;
            if (m0) s0 += gsum[(int64_t)(2 + p) * D + d];
            if (m1) s1 += gsum[(int64_t)(2 + p + 16) * D + d];
        }
        if (p < Np && (!key || key[p] == want)) s0 += gsum[(int64_t)(2 + p) * D + d];
        // (eight keys requested together + unconditional loads of a clamped row times a 0 / 1 weight: 25 us against 21.5)
    }
    red[ry][cx] = s0 + s1;
    __syncthreads();
    if (ry == 0 && d < D) {
        float s = 0.f;
#pragma unroll
        for (int y = 0; y < 16; ++y) s += red[y][cx];
        if (slot == 0) {
            put(d_bias + d, s);
            put(d_cls + d, gsum[d]);
            put(d_dist + d, gsum[D + d]);
            put(d_npe + d, gsum[d]);
            put(d_npe + D + d, gsum[D + d]);
        } else if (slot <= Tpe) {
            put(d_tpos + (int64_t)d * Tpe + (slot - 1), s);
        } else {
            put(d_fpos + (int64_t)d * Fpe + (slot - 1 - Tpe), s);
        }
    }
}

// dpatch[(b*Np+p)][d] = dtok[b][2+p][d]; 8 elements per thread (D % 8 == 0 fast path: two 16-byte loads, one 16-byte
// bf16 store, one row decomposition per vector), scalar otherwise
template <typename T>
__global__ void patch_rows_kernel(const float* __restrict__ dtok, int Ntok, int D, int Np, T* __restrict__ dpatch, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if ((D & 7) == 0) {
        const int dv = D >> 3;
        const int64_t nv = n >> 3;
        for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
            const int64_t row = v / dv;
            const int d = (int)(v - row * dv) * 8;
            const int64_t b = row / Np, p = row - b * Np;
            float x[8];
            load8<float>(dtok + (b * Ntok + 2 + p) * D + d, x);
            store8<T>(dpatch + row * D + d, x);
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int64_t row = i / D;
        const int d = (int)(i % D);
        const int64_t b = row / Np, p = row % Np;
        dpatch[i] = from_f32<T>(dtok[(b * Ntok + 2 + p) * D + d]);
    }
}

// ---- gradient w.r.t. the input spectrogram: fold (col2im) of the kept patches ------------------------------------------------
// grid[gf][gt] = index of the kept patch at that position of the patch grid, -1 where there is none (Patchout, time cut)
// (ONE workgroup: the table has a few thousand cells, and filling and scattering in one launch needs no second kernel boundary)
__global__ __launch_bounds__(1024) void patch_grid_build_kernel(const int32_t* __restrict__ pf, const int32_t* __restrict__ pt, int Np, int Fg,
                                                                int Tg, int32_t* __restrict__ grid) {
    const int cells = Fg * Tg;
    for (int i = threadIdx.x; i < cells; i += blockDim.x) grid[i] = -1;
    __syncthreads();                                 // (workgroup-scope ordering of the global stores above and below)
    for (int p = threadIdx.x; p < Np; p += blockDim.x) {
        const int f = pf[p], t = pt[p];
        if ((unsigned)f < (unsigned)Fg && (unsigned)t < (unsigned)Tg) grid[f * Tg + t] = p;
    }
}

// first / last patch-grid coordinate whose patch [g * stride, g * stride + P) holds pixel coordinate c (hi < lo: none)
__device__ __forceinline__ void cover_range(int c, int P, int stride, int G, int& lo, int& hi) {
    lo = c >= P ? (c - P) / stride + 1 : 0;
    hi = min(c / stride, G - 1);
}

// dx[b][f][t] = sum of dcols[b*Np + slot][(f - gf*fs)*P + (t - gt*ts)] over the kept patches (gf, gt) that hold (f, t), added in
// (gf, gt) order.  One thread = four consecutive elements of the flat dx (one 16-byte store; the flat index keeps the store
// aligned whatever T is).  Four pixels of one row share their patches: the slot is looked up once per patch, and where the four
// columns lie inside the patch at an even offset (always, for even T and tstride) bf16 dcols are read as two 4-byte pairs.
template <typename T>
__global__ __launch_bounds__(256) void patch_fold_kernel(const T* __restrict__ dcols, const int32_t* __restrict__ grid, int Np, int P,
                                                         int fs, int ts, int Fg, int Tg, int F, int Tt, int64_t n, float* __restrict__ dx) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int64_t row0 = i0 / Tt;
    const int t0 = (int)(i0 - row0 * Tt);
    const int PP = P * P;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (t0 + 4 <= Tt) {
        const int f = (int)(row0 % F);
        const int64_t b = row0 / F;
        int flo, fhi, tlo, thi, unused;
        cover_range(f, P, fs, Fg, flo, fhi);
        cover_range(t0, P, ts, Tg, tlo, unused);
        cover_range(t0 + 3, P, ts, Tg, unused, thi);
        for (int gf = flo; gf <= fhi; ++gf) {
            for (int gt = tlo; gt <= thi; ++gt) {
                const int slot = grid[gf * Tg + gt];
                if (slot < 0) continue;
                const int j0 = t0 - gt * ts;
                const T* src = dcols + (b * Np + slot) * PP + (f - gf * fs) * P;
                if constexpr (sizeof(T) == 2) {
                    if (j0 >= 0 && j0 + 4 <= P && !((j0 | P) & 1)) {
                        const bf16x2 lo = *(const bf16x2*)(src + j0), hi = *(const bf16x2*)(src + j0 + 2);
                        v[0] += (float)lo[0]; v[1] += (float)lo[1]; v[2] += (float)hi[0]; v[3] += (float)hi[1];
                        continue;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((unsigned)(j0 + e) < (unsigned)P) v[e] += to_f32<T>(src[j0 + e]);
            }
        }
    } else {                                         // the four elements straddle a row end (T % 4 != 0) or the end of dx
        for (int e = 0; e < 4 && i0 + e < n; ++e) {
            const int64_t row = (i0 + e) / Tt;
            const int t = (int)(i0 + e - row * Tt), f = (int)(row % F);
            const int64_t b = row / F;
            int flo, fhi, tlo, thi;
            cover_range(f, P, fs, Fg, flo, fhi);
            cover_range(t, P, ts, Tg, tlo, thi);
            for (int gf = flo; gf <= fhi; ++gf)
                for (int gt = tlo; gt <= thi; ++gt) {
                    const int slot = grid[gf * Tg + gt];
                    if (slot >= 0) v[e] += to_f32<T>(dcols[(b * Np + slot) * PP + (f - gf * fs) * P + (t - gt * ts)]);
                }
        }
    }
    if (i0 + 4 <= n) {
        *(f32x4*)(dx + i0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
        for (int e = 0; i0 + e < n; ++e) dx[i0 + e] = v[e];
    }
}

// ---- packed batch of clips of different lengths: backward of the patch stage ----------------------------------------------------
// Eval mode has no Patchout, so the packed token matrix is regular per clip: clip b owns rows cu_tok[b] .. cu_tok[b + 1], its cls and
// dist rows first, then Fg x T_eff[b] patch rows in frequency-major order with T_eff[b] = (cu_tok[b + 1] - cu_tok[b] - 2) / Fg.  The
// row of patch (f, t) of clip b is cu_tok[b] + 2 + f * T_eff[b] + t: no grid -> slot table, no index arrays.
__device__ __forceinline__ int clip_cols(const int32_t* __restrict__ cu_tok, int b, int Fg, int& row0) {
    row0 = cu_tok[b];
    return max((cu_tok[b + 1] - row0 - 2) / Fg, 0);
}

// patch_fold_kernel for the packed batch: dx[b][f][t] = sum of dcols[cu_tok[b] + 2 + gf * T_eff[b] + gt][(f - gf*fs)*P + (t - gt*ts)] over
// the clip's patches (gf, gt) that hold (f, t), added in (gf, gt) order.  Every element of dx[B][F][Tt] is written; the columns
// behind a clip's last patch column (its own frames' end, the time cut) have no covering patch and get 0.
template <typename T>
__global__ __launch_bounds__(256) void patch_fold_varlen_kernel(const T* __restrict__ dcols, const int32_t* __restrict__ cu_tok, int P, int fs,
                                                                int ts, int Fg, int F, int Tt, int64_t n, float* __restrict__ dx) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int64_t row0 = i0 / Tt;
    const int t0 = (int)(i0 - row0 * Tt);
    const int PP = P * P;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (t0 + 4 <= Tt) {
        const int f = (int)(row0 % F);
        const int b = (int)(row0 / F);
        int tok0;
        const int Tg = clip_cols(cu_tok, b, Fg, tok0);
        int flo, fhi, tlo, thi, unused;
        cover_range(f, P, fs, Fg, flo, fhi);
        cover_range(t0, P, ts, Tg, tlo, unused);
        cover_range(t0 + 3, P, ts, Tg, unused, thi);
        for (int gf = flo; gf <= fhi; ++gf) {
            for (int gt = tlo; gt <= thi; ++gt) {
                const int j0 = t0 - gt * ts;
                const T* src = dcols + ((int64_t)tok0 + 2 + gf * Tg + gt) * PP + (f - gf * fs) * P;
                if constexpr (sizeof(T) == 2) {
                    if (j0 >= 0 && j0 + 4 <= P && !((j0 | P) & 1)) {
                        const bf16x2 lo = *(const bf16x2*)(src + j0), hi = *(const bf16x2*)(src + j0 + 2);
                        v[0] += (float)lo[0]; v[1] += (float)lo[1]; v[2] += (float)hi[0]; v[3] += (float)hi[1];
                        continue;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((unsigned)(j0 + e) < (unsigned)P) v[e] += to_f32<T>(src[j0 + e]);
            }
        }
    } else {                                         // the four elements straddle a row end (T % 4 != 0) or the end of dx
        for (int e = 0; e < 4 && i0 + e < n; ++e) {
            const int64_t row = (i0 + e) / Tt;
            const int t = (int)(i0 + e - row * Tt), f = (int)(row % F);
            const int b = (int)(row / F);
            int tok0;
            const int Tg = clip_cols(cu_tok, b, Fg, tok0);
            int flo, fhi, tlo, thi;
            cover_range(f, P, fs, Fg, flo, fhi);
            cover_range(t, P, ts, Tg, tlo, thi);
            for (int gf = flo; gf <= fhi; ++gf)
                for (int gt = tlo; gt <= thi; ++gt)
                    v[e] += to_f32<T>(dcols[((int64_t)tok0 + 2 + gf * Tg + gt) * PP + (f - gf * fs) * P + (t - gt * ts)]);
        }
    }
    if (i0 + 4 <= n) {
        *(f32x4*)(dx + i0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
        for (int e = 0; i0 + e < n; ++e) dx[i0 + e] = v[e];
    }
}

// Parameter gradients of the patch stage from the packed dtok[M][D]: workgroup = one slot x 16 channels x 16 row groups, as in
// patch_param_grads_kernel, but the rows of a slot are enumerated from cu_tok (clip after clip, a fixed order) instead of searched:
// slot 0: conv bias = every patch row, plus the cls / dist rows; 1 .. Tpe: the Fg rows of time column t of every clip that has it;
// Tpe + 1 .. Tpe + Fpe: the T_eff rows of frequency row f of every clip.  No atomics: every thread adds its rows in ascending
// order and the 16 partial sums meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void patch_param_grads_varlen_kernel(const float* __restrict__ dtok, int D, const int32_t* __restrict__ cu_tok,
                                                                       int B, int Tpe, int Fpe, float* __restrict__ d_cls, float* __restrict__ d_dist,
                                                                       float* __restrict__ d_npe, float* __restrict__ d_bias, float* __restrict__ d_tpos,
                                                                       float* __restrict__ d_fpos, int accumulate) {
    __shared__ float red[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int slot = blockIdx.y;
    const int d = blockIdx.x * 16 + cx;
    auto put = [&](float* p, float v) { *p = (accumulate ? *p : 0.f) + v; };
    float s0 = 0.f, s1 = 0.f;
    if (d < D) {
        for (int b = 0; b < B; ++b) {
            int tok0;
            const int Tg = clip_cols(cu_tok, b, Fpe, tok0);
            int count, first, step;                    // the slot's rows of this clip: tok0 + 2 + first + j * step, j < count
            if (slot == 0) { count = Fpe * Tg; first = 0; step = 1; }
            else if (slot <= Tpe) { count = slot - 1 < Tg ? Fpe : 0; first = slot - 1; step = Tg; }
            else { count = Tg; first = (slot - 1 - Tpe) * Tg; step = 1; }
            const float* src = dtok + ((int64_t)tok0 + 2 + first) * D + d;
            int j = ry;
            for (; j + 16 < count; j += 32) {          // two rows per step: two loads in flight
                s0 += src[(int64_t)j * step * D];
                s1 += src[(int64_t)(j + 16) * step * D];
            }
            if (j < count) s0 += src[(int64_t)j * step * D];
        }
    }
    red[ry][cx] = s0 + s1;
    __syncthreads();
    if (ry == 0 && d < D) {
        float s = 0.f;
#pragma unroll
        for (int y = 0; y < 16; ++y) s += red[y][cx];
        if (slot == 0) {
            float c = 0.f, t = 0.f;
            for (int b = 0; b < B; ++b) {
                const int tok0 = cu_tok[b];
                if (cu_tok[b + 1] - tok0 >= 2) {
                    c += dtok[(int64_t)tok0 * D + d];
                    t += dtok[((int64_t)tok0 + 1) * D + d];
                }
            }
            put(d_bias + d, s);
            put(d_cls + d, c);
            put(d_dist + d, t);
            put(d_npe + d, c);
            put(d_npe + D + d, t);
        } else if (slot <= Tpe) {
            put(d_tpos + (int64_t)d * Tpe + (slot - 1), s);
        } else {
            put(d_fpos + (int64_t)d * Fpe + (slot - 1 - Tpe), s);
        }
    }
}

// ---- packed batch with Patchout (training): backward of the patch stage through a slot table -----------------------------------------
// With patches dropped a row's grid position no longer follows from its place in the clip, so both kernels walk
// slot[B][Fg][Tg] (int32): the packed row of the kept patch (f, t) of clip b, or -1 (dropped, behind the clip's last column, behind
// the time cut); Tg = the patch columns of the widest clip.  An entry outside [0, M) is treated as -1.

// patch_fold_varlen_kernel with the covering patches looked up in the slot table: dx[b][f][t] = sum of dcols[slot[b][gf][gt]][(f - gf*fs)*P +
// (t - gt*ts)] over the KEPT patches (gf, gt) of clip b that hold (f, t), added in (gf, gt) order.  Every element of dx[B][F][Tt] is
// written; a pixel no kept patch covers gets exactly 0.
template <typename T>
__global__ __launch_bounds__(256) void patch_fold_rows_kernel(const T* __restrict__ dcols, int M, const int32_t* __restrict__ slot, int P,
                                                              int fs, int ts, int Fg, int Tg, int F, int Tt, int64_t n, float* __restrict__ dx) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= n) return;
    const int64_t row0 = i0 / Tt;
    const int t0 = (int)(i0 - row0 * Tt);
    const int PP = P * P;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (t0 + 4 <= Tt) {
        const int f = (int)(row0 % F);
        const int32_t* tab = slot + (row0 / F) * Fg * Tg;
        int flo, fhi, tlo, thi, unused;
        cover_range(f, P, fs, Fg, flo, fhi);
        cover_range(t0, P, ts, Tg, tlo, unused);
        cover_range(t0 + 3, P, ts, Tg, unused, thi);
        for (int gf = flo; gf <= fhi; ++gf) {
            for (int gt = tlo; gt <= thi; ++gt) {
                const int r = tab[gf * Tg + gt];
                if ((unsigned)r >= (unsigned)M) continue;
                const int j0 = t0 - gt * ts;
                const T* src = dcols + (int64_t)r * PP + (f - gf * fs) * P;
                if constexpr (sizeof(T) == 2) {
                    if (j0 >= 0 && j0 + 4 <= P && !((j0 | P) & 1)) {
                        const bf16x2 lo = *(const bf16x2*)(src + j0), hi = *(const bf16x2*)(src + j0 + 2);
                        v[0] += (float)lo[0]; v[1] += (float)lo[1]; v[2] += (float)hi[0]; v[3] += (float)hi[1];
                        continue;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((unsigned)(j0 + e) < (unsigned)P) v[e] += to_f32<T>(src[j0 + e]);
            }
        }
    } else {                                         // the four elements straddle a row end (T % 4 != 0) or the end of dx
        for (int e = 0; e < 4 && i0 + e < n; ++e) {
            const int64_t row = (i0 + e) / Tt;
            const int t = (int)(i0 + e - row * Tt), f = (int)(row % F);
            const int32_t* tab = slot + (row / F) * Fg * Tg;
            int flo, fhi, tlo, thi;
            cover_range(f, P, fs, Fg, flo, fhi);
            cover_range(t, P, ts, Tg, tlo, thi);
            for (int gf = flo; gf <= fhi; ++gf)
                for (int gt = tlo; gt <= thi; ++gt) {
                    const int r = tab[gf * Tg + gt];
                    if ((unsigned)r < (unsigned)M) v[e] += to_f32<T>(dcols[(int64_t)r * PP + (f - gf * fs) * P + (t - gt * ts)]);
                }
        }
    }
    if (i0 + 4 <= n) {
        *(f32x4*)(dx + i0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
        for (int e = 0; i0 + e < n; ++e) dx[i0 + e] = v[e];
    }
}

// patch_param_grads_varlen_kernel for a batch with Patchout: workgroup = one slot x 16 channels x 16 row groups.  Slot 0 (conv bias,
// cls / dist) needs no table: a clip's patch rows are cu_tok[b] + 2 .. cu_tok[b + 1].  A positional slot enumerates its CANDIDATE
// cells of the slot table clip after clip -- time position p: the Fg cells of grid column p - toff[b] (the clip's own random offset
// into the time embedding), frequency row f: the Tg cells of that row -- and adds the rows of the kept ones.  Thread group ry takes
// candidates ry, ry + 16, ... of every clip in ascending order and the 16 partial sums meet in LDS in a fixed order: no atomics,
// bit-identical from run to run.
__global__ __launch_bounds__(256) void patch_param_grads_rows_kernel(const float* __restrict__ dtok, int M, int D, const int32_t* __restrict__ slot,
                                                                     const int32_t* __restrict__ cu_tok, const int32_t* __restrict__ toff, int B,
                                                                     int Tg, int Tpe, int Fpe, float* __restrict__ d_cls, float* __restrict__ d_dist,
                                                                     float* __restrict__ d_npe, float* __restrict__ d_bias, float* __restrict__ d_tpos,
                                                                     float* __restrict__ d_fpos, int accumulate) {
    __shared__ float red[16][17];
    const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
    const int slot_id = blockIdx.y;                    // 0: bias + prefix tokens; 1 .. Tpe: time; Tpe + 1 .. Tpe + Fpe: frequency
    const int d = blockIdx.x * 16 + cx;
    auto put = [&](float* p, float v) { *p = (accumulate ? *p : 0.f) + v; };
    float s0 = 0.f, s1 = 0.f;
    if (d < D) {
        const float* src = dtok + d;
        for (int b = 0; b < B; ++b) {
            if (slot_id == 0) {
                const int lo = max(cu_tok[b] + 2, 0), hi = min(cu_tok[b + 1], M);
                int r = lo + ry;
                for (; r + 16 < hi; r += 32) {         // two rows per step: two loads in flight
                    s0 += src[(int64_t)r * D];
                    s1 += src[(int64_t)(r + 16) * D];
                }
                if (r < hi) s0 += src[(int64_t)r * D];
                continue;
            }
            const int32_t* tab = slot + (int64_t)b * Fpe * Tg;
            int count, step;                           // the slot's candidate cells of this clip: tab[j * step], j < count
            if (slot_id <= Tpe) {
                const int t = slot_id - 1 - toff[b];
                count = (unsigned)t < (unsigned)Tg ? Fpe : 0; step = Tg; tab += count ? t : 0;
            } else {
                count = Tg; step = 1; tab += (slot_id - 1 - Tpe) * Tg;
            }
            int j = ry;
            for (; j + 16 < count; j += 32) {
                const int r0 = tab[j * step], r1 = tab[(j + 16) * step];
                if ((unsigned)r0 < (unsigned)M) s0 += src[(int64_t)r0 * D];
                if ((unsigned)r1 < (unsigned)M) s1 += src[(int64_t)r1 * D];
            }
            if (j < count) {
                const int r0 = tab[j * step];
                if ((unsigned)r0 < (unsigned)M) s0 += src[(int64_t)r0 * D];
            }
        }
    }
    red[ry][cx] = s0 + s1;
    __syncthreads();
    if (ry == 0 && d < D) {
        float s = 0.f;
#pragma unroll
        for (int y = 0; y < 16; ++y) s += red[y][cx];
        if (slot_id == 0) {
            float c = 0.f, t = 0.f;
            for (int b = 0; b < B; ++b) {
                const int tok0 = cu_tok[b];
                if (tok0 >= 0 && cu_tok[b + 1] - tok0 >= 2 && tok0 + 2 <= M) {
                    c += dtok[(int64_t)tok0 * D + d];
                    t += dtok[((int64_t)tok0 + 1) * D + d];
                }
            }
            put(d_bias + d, s);
            put(d_cls + d, c);
            put(d_dist + d, t);
            put(d_npe + d, c);
            put(d_npe + D + d, t);
        } else if (slot_id <= Tpe) {
            put(d_tpos + (int64_t)d * Tpe + (slot_id - 1), s);
        } else {
            put(d_fpos + (int64_t)d * Fpe + (slot_id - 1 - Tpe), s);
        }
    }
}

}  // namespace pa

using namespace pa;

// Order of the argument checks of every patch entry (include/passt_amd.h): NULL pointers and scalars (PA_EINVAL), dtype (PA_EINVAL),
// pointer alignment (PA_EINVAL), then the size limits (PA_EUNSUPPORTED).  Nothing is launched before all of them have passed.
static inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

extern "C" int pa_patch_gather(const float* x, int B, int F, int T, const int32_t* patch_f, const int32_t* patch_t,
                               int Np, int P, int fstride, int tstride, void* cols, int dtype, void* stream) {
    if (!x || !patch_f || !patch_t || !cols || B <= 0 || Np <= 0 || P <= 0 || fstride <= 0 || tstride <= 0 || F < P || T < P) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    if (P * P > 1024) return PA_EUNSUPPORTED;
    dim3 grid((unsigned)Np, (unsigned)B);
    if (dtype == PA_BF16) hipLaunchKernelGGL(patch_gather_kernel<bf16>, grid, dim3(P * P), 0, (hipStream_t)stream, x, F, T, patch_f, patch_t, Np, P, fstride, tstride, (bf16*)cols);
    else if (dtype == PA_F32) hipLaunchKernelGGL(patch_gather_kernel<float>, grid, dim3(P * P), 0, (hipStream_t)stream, x, F, T, patch_f, patch_t, Np, P, fstride, tstride, (float*)cols);
    else return PA_EINVAL;
    return check_launch();
}

extern "C" int pa_patch_pos_table(const float* bias, const float* time_pos, int Tpe, const float* freq_pos, int Fpe,
                                  const int32_t* patch_f, const int32_t* patch_t, int Np, int toff, int D, float* table,
                                  const float* cls, const float* dist, const float* npe, float* tok, int B, int Ntok,
                                  void* stream) {
    if (!bias || !time_pos || !freq_pos || !patch_f || !patch_t || !table || !cls || !dist || !npe || !tok) return PA_EINVAL;
    if (Np <= 0 || D <= 0 || B <= 0 || Tpe <= 0 || Fpe <= 0 || Ntok < 2) return PA_EINVAL;
    const int64_t n = (int64_t)Np * D + (int64_t)B * 2 * D;
    hipLaunchKernelGGL(patch_pos_table_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, bias,
                       time_pos, Tpe, freq_pos, Fpe, patch_f, patch_t, Np, toff, D, table, cls, dist, npe, tok, B, Ntok);
    return check_launch();
}

extern "C" int pa_patch_gather_varlen(const float* x, int B, int F, int T_max, const int32_t* row_clip, const int32_t* row_f,
                                      const int32_t* row_t, int M, int P, int fstride, int tstride, void* cols, int dtype, void* stream) {
    if (!x || !row_clip || !row_f || !row_t || !cols || B <= 0 || F <= 0 || T_max <= 0 || M <= 0 || P <= 0 || fstride <= 0 || tstride <= 0)
        return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    if (P * P > 1024) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)M), block((unsigned)(P * P));
    if (dtype == PA_BF16)
        hipLaunchKernelGGL(patch_gather_varlen_kernel<bf16>, grid, block, 0, (hipStream_t)stream, x, B, F, T_max, row_clip, row_f, row_t, P, fstride,
                           tstride, (bf16*)cols);
    else if (dtype == PA_F32)
        hipLaunchKernelGGL(patch_gather_varlen_kernel<float>, grid, block, 0, (hipStream_t)stream, x, B, F, T_max, row_clip, row_f, row_t, P, fstride,
                           tstride, (float*)cols);
    else return PA_EINVAL;
    return check_launch();
}

extern "C" int pa_patch_pos_table_varlen(const float* bias, const float* time_pos, int Tpe, const float* freq_pos, int Fpe,
                                         const int32_t* row_f, const int32_t* row_t, int M, int D, float* table, const float* cls,
                                         const float* dist, const float* npe, void* stream) {
    if (!bias || !time_pos || !freq_pos || !row_f || !row_t || !table || !cls || !dist || !npe || M <= 0 || D <= 0 || Tpe <= 0 || Fpe <= 0)
        return PA_EINVAL;
    const int64_t n = (int64_t)M * D;
    hipLaunchKernelGGL(patch_pos_table_varlen_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, bias, time_pos, Tpe,
                       freq_pos, Fpe, row_f, row_t, M, D, table, cls, dist, npe);
    return check_launch();
}

extern "C" int pa_patch_bwd(const float* dtok, int B, int Ntok, int D, const int32_t* patch_f, const int32_t* patch_t,
                            int Np, int toff, int Tpe, int Fpe, float* gsum, float* d_cls, float* d_dist, float* d_npe,
                            float* d_bias, float* d_time_pos, float* d_freq_pos, int accumulate, void* dpatch, int dtype,
                            void* stream) {
    // gsum and the six parameter gradients all NULL: only the compaction (frozen network: dpatch feeds the input-gradient GEMM)
    const bool rows_only = !gsum && !d_cls && !d_dist && !d_npe && !d_bias && !d_time_pos && !d_freq_pos;
    if (!dtok || !patch_f || !patch_t || !dpatch || B <= 0 || Np <= 0 || D <= 0 || Tpe <= 0 || Fpe <= 0 || Ntok < Np + 2) return PA_EINVAL;
    if (!rows_only && (!gsum || !d_cls || !d_dist || !d_npe || !d_bias || !d_time_pos || !d_freq_pos)) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    // batch_sum_kernel and patch_rows_kernel move 16-byte vectors of dtok, gsum and dpatch
    if (misaligned(dtok, 16) || misaligned(gsum, 16) || misaligned(dpatch, 16)) return PA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int rc = PA_OK;
    if (!rows_only) {
        const int64_t per = (int64_t)Ntok * D;
        hipLaunchKernelGGL(batch_sum_kernel, dim3((unsigned)cdiv(per, 1024)), dim3(256), 0, st, dtok, B, per, gsum);
        rc = check_launch();
        if (rc) return rc;
        hipLaunchKernelGGL(patch_param_grads_kernel, dim3((unsigned)cdiv(D, 16), (unsigned)(1 + Tpe + Fpe)), dim3(256), 0, st, gsum, D, patch_f,
                           patch_t, Np, toff, Tpe, Fpe, d_cls, d_dist, d_npe, d_bias, d_time_pos, d_freq_pos, accumulate);
        rc = check_launch();
        if (rc) return rc;
    }
    const int64_t total = (int64_t)B * Np * D;
    const int blocks = (int)std::min<int64_t>(cdiv(total, 256), 8192);
    if (dtype == PA_BF16) hipLaunchKernelGGL(patch_rows_kernel<bf16>, dim3(blocks), dim3(256), 0, st, dtok, Ntok, D, Np, (bf16*)dpatch, total);
    else hipLaunchKernelGGL(patch_rows_kernel<float>, dim3(blocks), dim3(256), 0, st, dtok, Ntok, D, Np, (float*)dpatch, total);
    return check_launch();
}

extern "C" int64_t pa_patch_input_bwd_ws_ints(int F, int T, int P, int fstride, int tstride) {
    if (P <= 0 || fstride <= 0 || tstride <= 0 || F < P || T < P) return 0;
    return (int64_t)((F - P) / fstride + 1) * ((T - P) / tstride + 1);
}

extern "C" int pa_patch_input_bwd(const void* dcols, int dtype, int B, int Np, const int32_t* patch_f, const int32_t* patch_t, int P,
                                  int fstride, int tstride, int F, int T, int32_t* grid_ws, float* dx, void* stream) {
    if (!dcols || !patch_f || !patch_t || !grid_ws || !dx || B <= 0 || Np <= 0 || P <= 0 || fstride <= 0 || tstride <= 0 || F < P || T < P)
        return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    // the fold stores 16-byte vectors of dx and reads bf16 dcols in 4-byte pairs
    if (misaligned(dx, 16) || misaligned(dcols, 4)) return PA_EINVAL;
    const int64_t cells = pa_patch_input_bwd_ws_ints(F, T, P, fstride, tstride);
    const int Fg = (F - P) / fstride + 1, Tg = (T - P) / tstride + 1;
    const int64_t n = (int64_t)B * F * T;
    // distinct kept patches fit the grid; int32 indexing of the table and of the launch grid
    if (Np > cells || cells >= ((int64_t)1 << 31) || cdiv(n, 1024) >= ((int64_t)1 << 31)) return PA_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(patch_grid_build_kernel, dim3(1), dim3(1024), 0, st, patch_f, patch_t, Np, Fg, Tg, grid_ws);
    int rc = check_launch();
    if (rc) return rc;
    const dim3 grid((unsigned)cdiv(n, 1024)), block(256);
    if (dtype == PA_BF16)
        hipLaunchKernelGGL(patch_fold_kernel<bf16>, grid, block, 0, st, (const bf16*)dcols, grid_ws, Np, P, fstride, tstride, Fg, Tg, F, T, n, dx);
    else
        hipLaunchKernelGGL(patch_fold_kernel<float>, grid, block, 0, st, (const float*)dcols, grid_ws, Np, P, fstride, tstride, Fg, Tg, F, T, n, dx);
    return check_launch();
}

extern "C" int pa_patch_input_bwd_varlen(const void* dcols, int dtype, const int32_t* cu_tok, int B, int P, int fstride, int tstride, int F,
                                         int T_max, float* dx, void* stream) {
    if (!dcols || !cu_tok || !dx || B <= 0 || P <= 0 || fstride <= 0 || tstride <= 0 || F < P || T_max < P) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    // the fold stores 16-byte vectors of dx and reads bf16 dcols in 4-byte pairs
    if (misaligned(dx, 16) || misaligned(dcols, 4)) return PA_EINVAL;
    const int Fg = (F - P) / fstride + 1;
    const int64_t n = (int64_t)B * F * T_max;
    if (cdiv(n, 1024) >= ((int64_t)1 << 31)) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)cdiv(n, 1024)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PA_BF16)
        hipLaunchKernelGGL(patch_fold_varlen_kernel<bf16>, grid, block, 0, st, (const bf16*)dcols, cu_tok, P, fstride, tstride, Fg, F, T_max, n, dx);
    else
        hipLaunchKernelGGL(patch_fold_varlen_kernel<float>, grid, block, 0, st, (const float*)dcols, cu_tok, P, fstride, tstride, Fg, F, T_max, n, dx);
    return check_launch();
}

extern "C" int pa_patch_bwd_varlen(const float* dtok, int M, int D, const int32_t* cu_tok, int B, int Tpe, int Fpe, float* d_cls, float* d_dist,
                                   float* d_npe, float* d_bias, float* d_time_pos, float* d_freq_pos, int accumulate, void* stream) {
    // all six NULL: nothing to do (frozen network)
    const bool none = !d_cls && !d_dist && !d_npe && !d_bias && !d_time_pos && !d_freq_pos;
    if (!dtok || !cu_tok || M <= 0 || D <= 0 || B <= 0 || Tpe <= 0 || Fpe <= 0) return PA_EINVAL;
    if (none) return PA_OK;
    if (!d_cls || !d_dist || !d_npe || !d_bias || !d_time_pos || !d_freq_pos) return PA_EINVAL;
    hipLaunchKernelGGL(patch_param_grads_varlen_kernel, dim3((unsigned)cdiv(D, 16), (unsigned)(1 + Tpe + Fpe)), dim3(256), 0, (hipStream_t)stream,
                       dtok, D, cu_tok, B, Tpe, Fpe, d_cls, d_dist, d_npe, d_bias, d_time_pos, d_freq_pos, accumulate);
    return check_launch();
}

extern "C" int pa_patch_input_bwd_rows(const void* dcols, int dtype, int M, const int32_t* slot, int B, int Tg, int P, int fstride, int tstride,
                                       int F, int T_max, float* dx, void* stream) {
    if (!dcols || !slot || !dx || M <= 0 || B <= 0 || Tg <= 0 || P <= 0 || fstride <= 0 || tstride <= 0 || F < P || T_max < P) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    // the fold stores 16-byte vectors of dx and reads bf16 dcols in 4-byte pairs
    if (misaligned(dx, 16) || misaligned(dcols, 4)) return PA_EINVAL;
    const int Fg = (F - P) / fstride + 1;
    const int64_t n = (int64_t)B * F * T_max;
    // int32 indexing of the table and of the launch grid
    if ((int64_t)B * Fg * Tg >= ((int64_t)1 << 31) || cdiv(n, 1024) >= ((int64_t)1 << 31)) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)cdiv(n, 1024)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PA_BF16)
        hipLaunchKernelGGL(patch_fold_rows_kernel<bf16>, grid, block, 0, st, (const bf16*)dcols, M, slot, P, fstride, tstride, Fg, Tg, F, T_max, n, dx);
    else
        hipLaunchKernelGGL(patch_fold_rows_kernel<float>, grid, block, 0, st, (const float*)dcols, M, slot, P, fstride, tstride, Fg, Tg, F, T_max, n, dx);
    return check_launch();
}

extern "C" int pa_patch_bwd_rows(const float* dtok, int M, int D, const int32_t* slot, const int32_t* cu_tok, const int32_t* toff, int B, int Tg,
                                 int Tpe, int Fpe, float* d_cls, float* d_dist, float* d_npe, float* d_bias, float* d_time_pos, float* d_freq_pos,
                                 int accumulate, void* stream) {
    // all six NULL: nothing to do (frozen network)
    const bool none = !d_cls && !d_dist && !d_npe && !d_bias && !d_time_pos && !d_freq_pos;
    if (!dtok || !slot || !cu_tok || !toff || M <= 0 || D <= 0 || B <= 0 || Tg <= 0 || Tpe <= 0 || Fpe <= 0) return PA_EINVAL;
    if ((int64_t)B * Fpe * Tg >= ((int64_t)1 << 31)) return PA_EUNSUPPORTED;
    if (none) return PA_OK;
    if (!d_cls || !d_dist || !d_npe || !d_bias || !d_time_pos || !d_freq_pos) return PA_EINVAL;
    hipLaunchKernelGGL(patch_param_grads_rows_kernel, dim3((unsigned)cdiv(D, 16), (unsigned)(1 + Tpe + Fpe)), dim3(256), 0, (hipStream_t)stream,
                       dtok, M, D, slot, cu_tok, toff, B, Tg, Tpe, Fpe, d_cls, d_dist, d_npe, d_bias, d_time_pos, d_freq_pos, accumulate);
    return check_launch();
}

// Batch augmentation on the device: spectrogram mixup (ex_audioset.py:173-177, helpers/mixup.py) and the waveform chain gain,
// pad / truncate, roll and waveform mixup (audioset/dataset.py:73-78, 102-140, 315-329), each for fixed-length and ragged batches.
// Pure HBM streaming kernels.  (The impulse-response convolution in front of the waveform chain is ir_conv.hip.)
#include <algorithm>

#include "pa_common.h"

namespace pa {

// a * l + c * (1 - l) as ONE definite sequence of roundings: the product c * (1 - l), then one fused multiply-add.  It is what the
// compiler's contraction made of mixup_kernel's expression; written out, pa_mixup's 16-byte path and pa_mixup_varlen cannot come to
// differ by how a * b + c happens to be fused in each (the adamw_one story, optim.hip).
__device__ __forceinline__ float mix_one(float a, float l, float c, float oml) {
#pragma clang fp contract(off)
    const float cw = c * oml;
    return __builtin_fmaf(l, a, cw);
}

__global__ void mixup_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm, const float* __restrict__ lam,
                             float* __restrict__ out, int64_t per4) {
    const int b = blockIdx.y;
    const float l = lam[b], oml = 1.f - l;
    const float4* xa = (const float4*)x + (int64_t)b * per4;
    const float4* xb = (const float4*)x + (int64_t)perm[b] * per4;
    float4* o = (float4*)out + (int64_t)b * per4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per4; i += (int64_t)gridDim.x * blockDim.x) {
        const float4 a = xa[i], c = xb[i];
        o[i] = make_float4(mix_one(a.x, l, c.x, oml), mix_one(a.y, l, c.y, oml), mix_one(a.z, l, c.z, oml), mix_one(a.w, l, c.w, oml));
    }
}

// Mixup of a ragged batch, [B][rows][ldt] with clip b valid in its first lens[b] columns: the mixed clip keeps its own length, the
// partner is cut to it or continued with ``pad``, the cells behind it are 0.  One work item = W consecutive elements of one clip (W = 4:
// a 16-byte group of the clip's rows * ldt floats, which is a multiple of 4; W = 1: the scalar path).  With ldt % 4 == 0 a group lies
// in one row; otherwise it may run over a row's end into the next row's first columns (``wraps``; ldt >= W, so at most once).  A
// group with no lane inside the clip is written without a load, one with no lane inside the partner's length loads only the clip's
// own; any other group takes every lane's side by a select on the lane's own column, AFTER the loads -- a value behind a length is
// chosen away, never multiplied by 0, so a NaN there stays there.
template <int W> __global__ void mixup_varlen_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens,
                                                      const int32_t* __restrict__ perm, const float* __restrict__ lam, float pad,
                                                      float* __restrict__ out, int ldt, uint32_t per) {
    typedef float vec __attribute__((ext_vector_type(W)));
    const int b = blockIdx.y, j = perm[b];
    const float l = lam[b], oml = 1.f - l;
    const int ni = min(max(lens[b], 0), ldt), nj = min(max(lens[j], 0), ldt);
    const vec* xa = (const vec*)x + (int64_t)b * per;             // per = rows * ldt / W work items in one clip
    const vec* xb = (const vec*)x + (int64_t)j * per;
    vec* o = (vec*)out + (int64_t)b * per;
    // the column of lane 0 is carried along the grid-stride loop: one division in front of it, an add and a compare inside
    const uint32_t stride = gridDim.x * blockDim.x, i0 = blockIdx.x * blockDim.x + threadIdx.x;
    const int dt = (int)(((uint64_t)stride * W) % (uint32_t)ldt);
    int t0 = (int)(((uint64_t)i0 * W) % (uint32_t)ldt);
    for (uint32_t i = i0; i < per; i += stride, t0 = t0 + dt < ldt ? t0 + dt : t0 + dt - ldt) {
        const bool wraps = W > 1 && t0 + W > ldt;                  // the last lanes are columns 0.. of the next row
        vec r = 0.f;
        if (t0 < ni || (wraps && ni > 0)) {
            const vec a = xa[i];
            vec c = pad;
            if (t0 < nj || (wraps && nj > 0)) c = xb[i];
#pragma unroll
            for (int e = 0; e < W; ++e) {
                const int t = t0 + e < ldt ? t0 + e : t0 + e - ldt;
                const float ce = t < nj ? c[e] : pad;
                const float m = mix_one(a[e], l, ce, oml);
                r[e] = t < ni ? m : 0.f;
            }
        }
        o[i] = r;
    }
}

__global__ void mixup_scalar_kernel(const float* __restrict__ x, const int32_t* __restrict__ perm, const float* __restrict__ lam,
                                    float* __restrict__ out, int64_t per) {
    const int b = blockIdx.y;
    const float l = lam[b];
    const float* xa = x + (int64_t)b * per;
    const float* xb = x + (int64_t)perm[b] * per;
    float* o = out + (int64_t)b * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x)
        o[i] = xa[i] * l + xb[i] * (1.f - l);
}

// Sum of a clip's first n samples by one 1024-thread block, in ONE fixed shape: thread i adds samples i, i + 1024, ... in order, a
// butterfly over each wave's 64 sums, a butterfly over the 16 wave sums.  Valid in thread 0 (in every lane of wave 0).  Nothing at or
// behind xc[n] is read.  Both mean kernels below go through it, so a clip's mean is the same number whichever entry asks for it.
__device__ __forceinline__ float clip_prefix_sum_1024(const float* __restrict__ xc, int64_t n, float* part /* 16 floats of LDS */) {
    // sixteen loads in flight per thread, added in the order of the plain loop (the compiler leaves that loop at one load per wait)
    float s = 0.f;
    int64_t t = threadIdx.x;
    for (; t + 15 * 1024 < n; t += 16 * 1024) {
        float q[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) q[k] = xc[t + k * 1024];
        __builtin_amdgcn_sched_barrier(0);               // every load issued before the first add waits for its operand
#pragma unroll
        for (int k = 0; k < 16; ++k) s += q[k];
    }
    for (; t < n; t += 1024) s += xc[t];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    float v = 0.f;
    if (threadIdx.x < 64) {
        v = threadIdx.x < 16 ? part[threadIdx.x] : 0.f;
        v = wave_sum(v);
    }
    return v;
}

// mean over the L samples of the padded / truncated, gain-scaled clip; one 1024-thread block per clip
__global__ __launch_bounds__(1024) void wave_mean_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ len,
                                                         const float* __restrict__ amp, float* __restrict__ mean, int64_t L) {
    __shared__ float part[16];
    const int b = blockIdx.x;
    const int64_t n = min((int64_t)(len ? len[b] : ldx), L);
    const float v = clip_prefix_sum_1024(x + (int64_t)b * ldx, n, part);
    if (threadIdx.x == 0) mean[b] = v * (amp ? amp[b] : 1.f) / (float)L;
}

__global__ __launch_bounds__(256) void wave_mix_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ len,
                                                       const float* __restrict__ amp, const int32_t* __restrict__ shift,
                                                       const int32_t* __restrict__ partner, const float* __restrict__ lam,
                                                       const float* __restrict__ mean, float* __restrict__ out, int64_t L) {
    const int b = blockIdx.y;
    const int p = partner ? partner[b] : -1;
    auto clip = [&](int c, int64_t t) {             // sample t of clip c after gain, pad/truncate and roll
        int64_t src = t - (shift ? shift[c] : 0);
        src %= L;
        if (src < 0) src += L;
        const int64_t n = min((int64_t)(len ? len[c] : ldx), L);
        return src < n ? x[(int64_t)c * ldx + src] * (amp ? amp[c] : 1.f) : 0.f;
    };
    const float l = p >= 0 ? fmaxf(lam[b], 1.f - lam[b]) : 1.f;
    const float mb = p >= 0 ? mean[b] : 0.f, mp = p >= 0 ? mean[p] : 0.f;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < L; t += (int64_t)gridDim.x * blockDim.x) {
        float v = clip(b, t);
        if (p >= 0) v = (v - mb) * l + (clip(p, t) - mp) * (1.f - l);
        out[(int64_t)b * L + t] = v;
    }
}

// ---- the ragged form (pa_wave_augment_varlen): row b has n = olen[b] samples of its own, and every clip that takes part in it -- the
// row's own and its partner -- is padded / cut, rolled and averaged AT THAT n, as if the fixed path ran with L = n.  A roll splits a
// row into two contiguous runs of its source, so the wrap is resolved once per clip and row (one 32-bit modulo in the prologue) and a
// sample costs a subtract, a compare and a select.  All sample indices are 32-bit.
typedef f32x4 f32x4u __attribute__((aligned(4)));        // a 16-byte load from a 4-byte aligned address (source runs start anywhere)

struct WaveSrc {
    const float* x;    // the clip's row
    int sh, m;         // shift mod n in [0, n); valid samples as the row sees them, min(len, n)
    float amp;
};
__device__ __forceinline__ WaveSrc wave_src(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ len,
                                            const float* __restrict__ amp, const int32_t* __restrict__ shift, int c, int n) {
    const int64_t lc = len ? min(max((int64_t)len[c], (int64_t)0), ldx) : ldx;
    int sh = shift ? shift[c] % n : 0;                    // n >= 1
    sh += sh < 0 ? n : 0;
    return WaveSrc{x + (int64_t)c * ldx, sh, (int)min(lc, (int64_t)n), amp ? amp[c] : 1.f};
}
// sample t, 0 <= t < n, of a clip after gain, pad / truncate to n and roll.  What lies at or behind x[m] is not read.
__device__ __forceinline__ float wave_item1(const WaveSrc& c, int t, int n) {
#pragma clang fp contract(off)
    int s = t - c.sh;
    s += s < 0 ? n : 0;
    float r = 0.f;
    if (s < c.m) r = c.x[s] * c.amp;
    return r;
}
// samples t0 .. t0 + 3 of it, 0 <= t0, t0 + 3 < n
__device__ __forceinline__ f32x4 wave_item4(const WaveSrc& c, int t0, int n) {
#pragma clang fp contract(off)
    int s0 = t0 - c.sh;
    s0 += s0 < 0 ? n : 0;
    f32x4 r = 0.f;
    if (s0 < c.m - 3) {                                   // one run inside the clip; m <= n, so the wrap is not inside the group either
        const f32x4u q = *(const f32x4u*)(c.x + s0);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = q[e] * c.amp;
    } else if (s0 < c.m || s0 > n - 4) {                  // the clip's end or the wrap inside the group: lane by lane
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = e < n - s0 ? s0 + e : s0 - n + e;
            if (s < c.m) r[e] = c.x[s] * c.amp;
        }
    }                                                     // else: four samples of the padding, nothing loaded
    return r;
}

// the two means of a mixed row, (b|b) and (p|b): mean2[2 b + which]; one 1024-thread block each, unmixed rows return at once
__global__ __launch_bounds__(1024) void wave_mean_varlen_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ len,
                                                                const int32_t* __restrict__ olen, const float* __restrict__ amp,
                                                                const int32_t* __restrict__ partner, float* __restrict__ mean2, int B, int L) {
    __shared__ float part[16];
    const int b = blockIdx.x, p = partner[b];
    const int n = min(max(olen[b], 0), L);
    if (p < 0 || p >= B || n < 1) return;                 // the same in every thread of the block
    const int c = blockIdx.y ? p : b;
    const int64_t lc = len ? min(max((int64_t)len[c], (int64_t)0), ldx) : ldx;
    const float v = clip_prefix_sum_1024(x + (int64_t)c * ldx, min(lc, (int64_t)n), part);
    if (threadIdx.x == 0) mean2[2 * b + blockIdx.y] = v * (amp ? amp[c] : 1.f) / (float)n;
}

// One streaming pass: row b of out, [0, L), in 16-byte stores from the row's first 16-byte boundary on (up to three 4-byte stores in
// front of it and behind the last whole group), so a row pitch or offset that breaks the alignment costs the row its edges only.
__global__ __launch_bounds__(256) void wave_mix_varlen_kernel(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ len,
                                                              const int32_t* __restrict__ olen, const float* __restrict__ amp,
                                                              const int32_t* __restrict__ shift, const int32_t* __restrict__ partner,
                                                              const float* __restrict__ lam, const float* __restrict__ mean2,
                                                              float* __restrict__ out, int64_t ldo, int B, int L) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int n = min(max(olen[b], 0), L);
    int p = partner ? partner[b] : -1;
    if (p >= B || n < 1) p = -1;
    const bool mixed = p >= 0;
    WaveSrc cb{x, 0, 0, 0.f}, cp{x, 0, 0, 0.f};
    if (n > 0) cb = wave_src(x, ldx, len, amp, shift, b, n);
    if (mixed) cp = wave_src(x, ldx, len, amp, shift, p, n);
    const float l = mixed ? fmaxf(lam[b], 1.f - lam[b]) : 1.f, oml = 1.f - l;
    const float mb = mixed ? mean2[2 * b] : 0.f, mp = mixed ? mean2[2 * b + 1] : 0.f;
    float* o = out + (int64_t)b * ldo;
    auto one = [&](int t) {
        float v = 0.f;
        if (t < n) {
            v = wave_item1(cb, t, n);
            if (mixed) v = mix_one(v - mb, l, wave_item1(cp, t, n) - mp, oml);
        }
        o[t] = v;
    };
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    const int head = min((int)((4 - (((uintptr_t)o >> 2) & 3)) & 3), L);
    const uint32_t nv = (uint32_t)(L - head) >> 2;
    if (tid < (uint32_t)head) one((int)tid);
    for (uint32_t i = tid; i < nv; i += stride) {
        const int t0 = head + (int)(4 * i);
        f32x4 r = 0.f;
        if (t0 < n - 3) {
            r = wave_item4(cb, t0, n);
            if (mixed) {
                const f32x4 c = wave_item4(cp, t0, n);
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = mix_one(r[e] - mb, l, c[e] - mp, oml);
            }
        } else if (t0 < n) {                              // the row's end inside the group
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e < n - t0) {
                    float v = wave_item1(cb, t0 + e, n);
                    if (mixed) v = mix_one(v - mb, l, wave_item1(cp, t0 + e, n) - mp, oml);
                    r[e] = v;
                }
            }
        }
        *(f32x4*)(o + t0) = r;
    }
    const uint32_t t = (uint32_t)head + 4 * nv + tid;
    if (t < (uint32_t)L) one((int)t);
}

}  // namespace pa

using namespace pa;

extern "C" int pa_mixup(const float* x, const int32_t* perm, const float* lam, float* out, int B, int64_t per_sample, void* stream) {
    if (!x || !perm || !lam || !out || B <= 0 || per_sample <= 0) return PA_EINVAL;
    if (per_sample % 4) {   // e.g. the (B, 527) target matrix: scalar path
        dim3 grid((unsigned)std::min<int64_t>(cdiv(per_sample, 256), 64), (unsigned)B);
        hipLaunchKernelGGL(mixup_scalar_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, perm, lam, out, per_sample);
        return check_launch();
    }
    const int64_t per4 = per_sample / 4;
    dim3 grid((unsigned)std::min<int64_t>(cdiv(per4, 256), 64), (unsigned)B);
    hipLaunchKernelGGL(mixup_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, perm, lam, out, per4);
    return check_launch();
}

extern "C" int pa_mixup_varlen(const float* x, const int32_t* lens, const int32_t* perm, const float* lam, float pad, float* out, int B,
                               int rows, int ldt, void* stream) {
    if (!x || !lens || !perm || !lam || !out || B < 1 || rows < 1 || ldt < 1 || out == x) return PA_EINVAL;
    if ((int64_t)rows * ldt >= ((int64_t)1 << 31)) return PA_EINVAL;       // the kernels index one clip with 32 bits
    // pa_mixup's grid: up to 64 workgroups per clip, grid-stride over the rest.  16-byte groups where a clip is a whole number of them
    // (always with ldt % 4 == 0; with 128 mel rows whatever the frame count) and both buffers are aligned
    if (((int64_t)rows * ldt) % 4 == 0 && ldt >= 4 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0) {
        const uint32_t per4 = (uint32_t)((int64_t)rows * ldt / 4);
        dim3 grid((unsigned)std::min<int64_t>(cdiv((int64_t)per4, 256), 64), (unsigned)B);
        hipLaunchKernelGGL(mixup_varlen_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, lens, perm, lam, pad, out, ldt, per4);
    } else {
        const uint32_t per = (uint32_t)((int64_t)rows * ldt);
        dim3 grid((unsigned)std::min<int64_t>(cdiv((int64_t)per, 256), 64), (unsigned)B);
        hipLaunchKernelGGL(mixup_varlen_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, lens, perm, lam, pad, out, ldt, per);
    }
    return check_launch();
}

extern "C" int pa_wave_augment(const float* x, int B, int64_t ldx, const int32_t* len, const float* amp, const int32_t* shift,
                               const int32_t* partner, const float* lam, float* ws, float* out, int64_t L, void* stream) {
    if (!x || !out || B <= 0 || ldx <= 0 || L <= 0 || (partner && (!lam || !ws))) return PA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (partner) {
        hipLaunchKernelGGL(wave_mean_kernel, dim3(B), dim3(1024), 0, st, x, ldx, len, amp, ws, L);
        const int rc = check_launch();
        if (rc) return rc;
    }
    dim3 grid((unsigned)std::min<int64_t>(cdiv(L, 256 * 4), 1024), (unsigned)B);
    hipLaunchKernelGGL(wave_mix_kernel, grid, dim3(256), 0, st, x, ldx, len, amp, shift, partner, lam, ws, out, L);
    return check_launch();
}

extern "C" int pa_wave_augment_varlen(const float* x, int B, int64_t ldx, const int32_t* len, const int32_t* olen, const float* amp,
                                      const int32_t* shift, const int32_t* partner, const float* lam, float* ws, float* out, int64_t ldo,
                                      int64_t L, void* stream) {
    if (!x || !out || !olen || B < 1 || B > 65535 || ldx < 1 || L < 1 || L > 0x7fffffff || ldo < L || (partner && (!lam || !ws)) || out == x)
        return PA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (partner) {
        hipLaunchKernelGGL(wave_mean_varlen_kernel, dim3(B, 2), dim3(1024), 0, st, x, ldx, len, olen, amp, partner, ws, B, (int)L);
        const int rc = check_launch();
        if (rc) return rc;
    }
    // about 4096 workgroups in all, grid-stride over a row's 16-byte groups
    const int64_t per_row = std::max<int64_t>(4096 / B, 1);
    dim3 grid((unsigned)std::min<int64_t>(cdiv(cdiv(L, 4), 256), per_row), (unsigned)B);
    hipLaunchKernelGGL(wave_mix_varlen_kernel, grid, dim3(256), 0, st, x, ldx, len, olen, amp, shift, partner, lam, ws, out, ldo, B, (int)L);
    return check_launch();
}

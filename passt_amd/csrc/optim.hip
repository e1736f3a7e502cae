// The optimizer side of the training step: AdamW (ex_audioset.py:104-109) in its flat, table and staging forms, the global gradient
// norm / clip factor, plain SGD (model_speed_test, ex_audioset.py:392) and the SWA average, on flat f32 buffers.  Pure HBM streaming
// kernels: float4 grid-stride loops.  (Spectrogram mixup and the waveform augmentation are augment.hip.)
#include <algorithm>
#include <cstring>

#include "pa_common.h"

namespace pa {

// One definite sequence of roundings (no contraction left to the compiler: it fused a * b + c differently in the kernels this is
// inlined into -- pa_adamw and pa_adamw_stage differed by an ulp): the two moment updates are ONE fused multiply-add each, nothing
// else is fused.  pa_adamw, pa_adamw_dev and pa_adamw_stage are bit-identical to each other by construction.
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps,
                                          float wd, float bc1, float bc2_sqrt) {
#pragma clang fp contract(off)
    const float pi = p * (1.f - lr * wd);
    const float gm = (1.f - b1) * g, gv = ((1.f - b2) * g) * g;
    m = __builtin_fmaf(b1, m, gm);
    v = __builtin_fmaf(b2, v, gv);
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    const float step = (lr / bc1) * (m / denom);
    p = pi - step;
}
// Global-norm clipping (pa_adamw_clip / pa_adamw_stage_clip): the gradient entering adamw_one is g * factor, ONE f32 multiplication,
// the factor being a device float (pa_clip_coef writes it: no host sync).  The gradient buffer is not written.  x * 1.0f == x bit for
// bit, so a factor of exactly 1 -- and CLIP = false, which is what every other entry instantiates -- leave today's bits.
template <bool CLIP> __device__ __forceinline__ float clip_g(float g, float gs) {
#pragma clang fp contract(off)
    if constexpr (CLIP) return g * gs;
    else return g;
}
// the hyper-parameters of one launch: [lr, beta1, beta2, eps, weight_decay, 1 - beta1^t, sqrt(1 - beta2^t)], the 7-float row of
// pa_adamw_hyper
struct AdamwHyper { float lr, b1, b2, eps, wd, bc1, bc2_sqrt; };
// adamw_one on one element / on four, the gradient through clip_g: every AdamW loop below is one of these two
template <bool CLIP> __device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const AdamwHyper& h, float gs) {
    adamw_one(p, clip_g<CLIP>(g, gs), m, v, h.lr, h.b1, h.b2, h.eps, h.wd, h.bc1, h.bc2_sqrt);
}
template <bool CLIP>
__device__ __forceinline__ void adamw_four(f32x4& pv, const f32x4& gv, f32x4& mv, f32x4& vv, const AdamwHyper& h, float gs) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = pv[e], me = mv[e], ve = vv[e];
        adamw_elem<CLIP>(pe, gv[e], me, ve, h, gs);
        pv[e] = pe; mv[e] = me; vv[e] = ve;
    }
}
// the hyper-parameters of one launch (by value, or the 7-float row in device memory: a launch whose arguments never change, i.e. one
// that can sit in a captured hipGraph) for table entry ``entry``: with parameter groups (``scales``: one (lr_scale, wd_scale) pair per
// descriptor) lr and weight decay are those of the launch times the entry's pair, so a captured launch follows the schedule through
// the device row while every parameter keeps its own factor
template <bool GROUPS>
__device__ __forceinline__ AdamwHyper adamw_hyper_of(const AdamwHyper& hv, const float* __restrict__ hy_dev, const float2* __restrict__ scales,
                                                     int entry) {
    AdamwHyper h = hv;
    if (hy_dev) { h.lr = hy_dev[0]; h.b1 = hy_dev[1]; h.b2 = hy_dev[2]; h.eps = hy_dev[3]; h.wd = hy_dev[4]; h.bc1 = hy_dev[5]; h.bc2_sqrt = hy_dev[6]; }
    if constexpr (GROUPS) {
        const float2 s = scales[entry];
        h.lr *= s.x;
        h.wd *= s.y;
    }
    return h;
}
// the clip factor of the step: one device float (pa_clip_coef writes it); a null pointer and CLIP = false mean 1
template <bool CLIP> __device__ __forceinline__ float adamw_gscale(const float* __restrict__ gscale) {
    if constexpr (CLIP) return gscale ? *gscale : 1.f;
    else return 1.f;
}

// The flat form (pa_adamw, pa_adamw_dev: CLIP = false; pa_adamw_clip: CLIP = true): 16-byte accesses (n4 = n / 4 when all four pointers
// are 16-byte aligned, else 0) + scalar tail
template <bool CLIP>
__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, int64_t n4, int64_t n, AdamwHyper hv,
                                                         const float* __restrict__ hy_dev, const float* __restrict__ gscale) {
    const AdamwHyper h = adamw_hyper_of<false>(hv, hy_dev, nullptr, 0);
    const float gs = adamw_gscale<CLIP>(gscale);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t0; i < n4; i += stride) {
        f32x4 pv = ((f32x4*)p)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
        adamw_four<CLIP>(pv, ((const f32x4*)g)[i], mv, vv, h, gs);
        ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
    }
    for (int64_t i = n4 * 4 + t0; i < n; i += stride) adamw_elem<CLIP>(p[i], g[i], m[i], v[i], h, gs);
}

// ---- AdamW + weight staging in ONE pass (round 6).  The step used to end with adamw_flat_kernel writing every updated parameter and
// the next forward beginning with stage_weights_kernel reading all of them back to make the GEMM-ready copies (bf16 W[out][in]
// for the forward, bf16 W^T[in][out] for the input gradients): one extra 345 MB read + a launch per step.  Here the optimizer
// launch of a bucket walks a descriptor table of the bucket's parameters: a matrix with copies is processed in 64 x 64 tiles
// (256 B of each row per 16 lanes; the updated values go out as f32, as the straight cast, and -- through an LDS tile -- as the
// transposed cast), everything else in runs of 4096 elements.  Same adamw_one() as adamw_flat_kernel: parameters, moments and both
// copies are bit-identical to adamw_flat_kernel + stage_weights_kernel (tests/test_gpu_model.py).
// Parameters, moments and gradients of the matrix path are touched once per step: non-temporal (CP_NT_ADAMW, pa_common.h).  The
// GEMM-ready copies leave as plain stores (non-temporal: +- 0, profiles/r06_cache_policy.txt).
template <typename V> __device__ __forceinline__ V opt_ld(const V* p) {
    if constexpr (CP_NT_ADAMW) return __builtin_nontemporal_load(p);
    else return *p;
}
template <typename V> __device__ __forceinline__ void opt_st(V* p, const V& v) {
    if constexpr (CP_NT_ADAMW) __builtin_nontemporal_store(v, p);
    else *p = v;
}
template <typename TO> __device__ __forceinline__ void st_bf16x4(TO* p, const f32x4& w) {
    *(bf16x4*)p = bf16x4{(bf16)w[0], (bf16)w[1], (bf16)w[2], (bf16)w[3]};
}

// the last table entry with tile_begin <= bid, found by one wave (the table is short) and handed to the block through LDS
__device__ __forceinline__ int adamw_find_entry(const pa_adamw_stage_desc* __restrict__ descs, int n_desc, int bid, int* s_entry) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        int found = -1;
        for (int e = tid; e < n_desc; e += 64)
            if (descs[e].tile_begin <= bid) found = e;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) found = max(found, __shfl_xor(found, o, 64));
        if (tid == 0) *s_entry = found;
    }
    __syncthreads();
    return *s_entry;
}
// What one workgroup of a table launch works on: its table entry, the entry's hyper-parameters, the four buffers at the entry's offset,
// its work item ``t`` there, and whether all four pointers are 16-byte aligned.  (The entry stays in the table: with a copy of the
// descriptor in here the table kernels take other registers than before.)
struct AdamwItem {
    const pa_adamw_stage_desc* d;
    AdamwHyper h;
    float* pp; const float* gp; float* mp; float* vp;
    int t;
    bool aligned;
};
template <bool GROUPS>
__device__ __forceinline__ AdamwItem adamw_item(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, const pa_adamw_stage_desc* __restrict__ descs, int n_desc,
                                                const float* __restrict__ hy_dev, const AdamwHyper& hv, const float2* __restrict__ scales) {
    __shared__ int s_entry;
    const int bid = blockIdx.x;
    const int entry = adamw_find_entry(descs, n_desc, bid, &s_entry);
    const pa_adamw_stage_desc d = descs[entry];
    AdamwItem w;
    w.d = descs + entry;
    w.h = adamw_hyper_of<GROUPS>(hv, hy_dev, scales, entry);
    w.pp = p + d.offset;
    w.gp = g + d.offset;
    w.mp = m + d.offset;
    w.vp = v + d.offset;
    w.t = bid - d.tile_begin;
    w.aligned = ((((uintptr_t)w.pp | (uintptr_t)w.gp | (uintptr_t)w.mp | (uintptr_t)w.vp) & 15) == 0);
    return w;
}
// a parameter without copies (biases, LayerNorm, positional tables, the f32 head): work item t is a run of 4096 consecutive elements
template <bool CLIP> __device__ __forceinline__ void adamw_run(const AdamwItem& w, float gs) {
    float* pp = w.pp; const float* gp = w.gp; float* mp = w.mp; float* vp = w.vp;
    const int tid = threadIdx.x;
    const int64_t n = (int64_t)w.d->rows * w.d->cols, i0 = (int64_t)w.t * 4096, i1 = min(i0 + 4096, n);
    if (w.aligned) {
        for (int64_t i = i0 + tid * 4; i < i1; i += 1024) {
            if (i + 4 <= i1) {
                f32x4 pv = *(f32x4*)(pp + i), mv = *(f32x4*)(mp + i), vv = *(f32x4*)(vp + i);
                adamw_four<CLIP>(pv, *(const f32x4*)(gp + i), mv, vv, w.h, gs);
                *(f32x4*)(pp + i) = pv; *(f32x4*)(mp + i) = mv; *(f32x4*)(vp + i) = vv;
            } else {
                for (int64_t k = i; k < i1; ++k) adamw_elem<CLIP>(pp[k], gp[k], mp[k], vp[k], w.h, gs);
            }
        }
    } else {
        for (int64_t i = i0 + tid; i < i1; i += 256) adamw_elem<CLIP>(pp[i], gp[i], mp[i], vp[i], w.h, gs);
    }
}

template <typename TO, bool GROUPS, bool CLIP>
__device__ __forceinline__ void adamw_stage_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, const pa_adamw_stage_desc* __restrict__ descs, int n_desc,
                                                 const float* __restrict__ hy_dev, const AdamwHyper& hv, const float2* __restrict__ scales,
                                                 float gs) {
    __shared__ float tile[64][65];
    const AdamwItem w = adamw_item<GROUPS>(p, g, m, v, descs, n_desc, hy_dev, hv, scales);
    const pa_adamw_stage_desc d = *w.d;
    if (!d.dst && !d.dst_t) {
        adamw_run<CLIP>(w, gs);
        return;
    }
    const AdamwHyper& h = w.h;
    float* pp = w.pp; const float* gp = w.gp; float* mp = w.mp; float* vp = w.vp;
    const int tid = threadIdx.x, t = w.t;
    const bool aligned = w.aligned;
    const int tiles_c = (d.cols + 63) >> 6;
    const int r0 = (t / tiles_c) * 64, c0 = (t % tiles_c) * 64;
    TO* dst = (TO*)d.dst;
    TO* dst_t = (TO*)d.dst_t;
    if (((d.rows | d.cols) & 3) == 0 && aligned) {
        // every PaSST weight: 16-byte accesses, 256 contiguous bytes of a row per 16 lanes
        const int lr = tid >> 4, l4 = (tid & 15) * 4;
        // all sixteen loads of the thread's four row pieces first (the stores below would otherwise fence the next piece's loads:
        // the four pointers alias as far as the compiler knows), then the arithmetic and the stores
        f32x4 pv[4], mv[4], vv[4], gv[4];
        bool in[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + lr + 16 * i, c = c0 + l4;
            in[i] = r < d.rows && c < d.cols;
            const int64_t at = in[i] ? (int64_t)r * d.cols + c : 0;
            pv[i] = opt_ld((const f32x4*)(pp + at)); mv[i] = opt_ld((const f32x4*)(mp + at)); vv[i] = opt_ld((const f32x4*)(vp + at)); gv[i] = opt_ld((const f32x4*)(gp + at));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + lr + 16 * i, c = c0 + l4;
            if (in[i]) {
                const int64_t at = (int64_t)r * d.cols + c;
                adamw_four<CLIP>(pv[i], gv[i], mv[i], vv[i], h, gs);
                opt_st((f32x4*)(pp + at), pv[i]); opt_st((f32x4*)(mp + at), mv[i]); opt_st((f32x4*)(vp + at), vv[i]);
                if (dst) {
                    if constexpr (sizeof(TO) == 2) st_bf16x4(dst + at, pv[i]);
                    else *(f32x4*)(dst + at) = pv[i];
                }
            } else {
                pv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[lr + 16 * i][l4 + k] = pv[i][k];
        }
        if (!dst_t) return;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c0 + lr + 16 * i, r = r0 + l4;
            if (c < d.cols && r < d.rows) {
                const f32x4 w = {tile[l4][lr + 16 * i], tile[l4 + 1][lr + 16 * i], tile[l4 + 2][lr + 16 * i], tile[l4 + 3][lr + 16 * i]};
                if constexpr (sizeof(TO) == 2) st_bf16x4(dst_t + (int64_t)c * d.rows + r, w);
                else *(f32x4*)(dst_t + (int64_t)c * d.rows + r) = w;
            }
        }
        return;
    }
    const int tx = tid & 63, ty = tid >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        const bool ok = r < d.rows && c < d.cols;
        float w = 0.f;
        if (ok) {
            const int64_t at = (int64_t)r * d.cols + c;
            adamw_elem<CLIP>(pp[at], gp[at], mp[at], vp[at], h, gs);
            w = pp[at];
            if (dst) dst[at] = from_f32<TO>(w);
        }
        tile[i][tx] = w;
    }
    if (!dst_t) return;
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < d.cols && r < d.rows) dst_t[(int64_t)c * d.rows + r] = from_f32<TO>(tile[tx][i]);
    }
}

// The table form (pa_adamw_stage; GROUPS: pa_adamw_stage_groups; CLIP, with either: pa_adamw_stage_clip)
template <typename TO, bool GROUPS, bool CLIP>
__global__ __launch_bounds__(256) void adamw_table_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, const pa_adamw_stage_desc* __restrict__ descs,
                                                          int n_desc, const float* __restrict__ hy_dev, AdamwHyper hv,
                                                          const float2* __restrict__ scales, const float* __restrict__ gscale) {
    adamw_stage_body<TO, GROUPS, CLIP>(p, g, m, v, descs, n_desc, hy_dev, hv, scales, adamw_gscale<CLIP>(gscale));
}
// parameter groups without staging (pa_adamw_groups): the same table (dst / dst_t are not looked at), every entry as runs of 4096
// elements -- no tile in LDS
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const pa_adamw_stage_desc* __restrict__ descs,
                                                           int n_desc, const float* __restrict__ hy_dev, AdamwHyper hv,
                                                           const float2* __restrict__ scales) {
    adamw_run<false>(adamw_item<true>(p, g, m, v, descs, n_desc, hy_dev, hv, scales), 1.f);
}

// ---- Global gradient norm + gradient accumulation: ONE streaming pass per span of the flat gradient buffer ---------------------
// Partition: a span of n elements is cut into chunks of GN_CHUNK = 4096 consecutive elements counted from the span's first element
// (pa_grad_norm_partials(n) = ceil(n / 4096): a function of n alone); one workgroup of 256 threads owns one chunk and writes one
// partial.  The order of additions inside a chunk depends on the element's index in the chunk only: the chunk's values go through an
// LDS image (element j at buf[shift + j], shift = the chunk's misalignment in elements, so 16-byte global accesses land on 16-byte
// LDS slots; a scalar head and tail), then thread t sums the squares of elements 4 (t + 256 k) + e in the order k = 0..3, e = 0..3
// (elements past the span count as +0: x + 0 == x), the 64 lanes of a wave combine by the xor butterfly (wave_sum), the 4 waves
// as (w0 + w1) + (w2 + w3).  No atomics, no finishing launch: bit-identical from run to run and for the same data at any address.
// Longest chain of roundings per partial: 1 (square) + 15 + 6 + 2 = 24 (DESIGN: the bound tests/test_gpu_grad_clip.py asserts).
// The gradient read is non-temporal although AdamW reads the same bytes again: measured (profiles/grad_clip.txt), not assumed -- the
// pass alone runs at 6.4 against 5.8 TB/s, the pair norm pass + AdamW over 340 MB takes 0.568 against 0.584 ms, and in the step the
// cost of clipping is 0.02 - 0.04 ms lower; a 345 MB gradient buffer does not stay in the 256 MiB Infinity Cache until the optimizer
// comes back to it.  -DPA_GRADNORM_PLAIN builds the plain load for the A/B (tools/bench_grad_clip.py --ab-lib).
constexpr int GN_CHUNK = 4096;
#ifdef PA_GRADNORM_PLAIN
static constexpr bool CP_NT_GRADNORM = false;
#else
static constexpr bool CP_NT_GRADNORM = PA_CP(1);
#endif
template <typename V> __device__ __forceinline__ V gn_ld(const V* p) {
    if constexpr (CP_NT_GRADNORM) return __builtin_nontemporal_load(p);
    else return *p;
}
__global__ __launch_bounds__(256) void grad_accum_sumsq_kernel(const float* __restrict__ g, float* __restrict__ acc, int first, int64_t n,
                                                               float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float buf[GN_CHUNK + 4];
    __shared__ float wsum[4];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * GN_CHUNK;
    const int len = (int)min((int64_t)GN_CHUNK, n - c0);
    const float* gp = g + c0;
    float* ap = acc ? acc + c0 : nullptr;
    const bool rd_acc = ap && !first;
    const int sg = (int)(((uintptr_t)gp >> 2) & 3);
    const bool vec = !ap || (int)(((uintptr_t)ap >> 2) & 3) == sg;       // 16-byte accesses need g and acc equally (mis)aligned
    const int shift = vec ? sg : 0;
    auto one = [&](int j) {
        float r = gn_ld(gp + j);
        if (rd_acc) r = ap[j] + r;
        if (ap) ap[j] = r;
        if (partials) buf[shift + j] = r;
    };
    if (!vec) {
        for (int j = tid; j < len; j += 256) one(j);
    } else {
        const int head = min((4 - shift) & 3, len), nv = (len - head) >> 2;
        if (tid < head) one(tid);
        for (int i = tid; i < nv; i += 256) {
            const int j = head + 4 * i;
            f32x4 r = gn_ld((const f32x4*)(gp + j));
            if (rd_acc) {
                const f32x4 a = *(const f32x4*)(ap + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) r[e] = a[e] + r[e];
            }
            if (ap) *(f32x4*)(ap + j) = r;
            if (partials) *(f32x4*)(buf + shift + j) = r;
        }
        const int j = head + 4 * nv + tid;
        if (j < len) one(j);
    }
    if (!partials) return;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * (tid + 256 * k);
        float x[4];
        if (shift == 0) {
            const f32x4 q = *(const f32x4*)(buf + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = q[e];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = buf[shift + j + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xe = j + e < len ? x[e] : 0.f;      // what lies behind the chunk's end in LDS was never written
            const float sq = xe * xe;
            s = s + sq;
        }
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// total norm and clip factor of one update: one workgroup, fixed order, the partials summed in f64 (thread t takes partials t, t + 256,
// ... in order, then a binary tree over the 256 sums).  The factor is what torch.nn.utils.clip_grad_norm_ computes in f32:
// max_norm / (norm + 1e-6) evaluated as reciprocal(norm + 1e-6f) * max_norm (Tensor.__rdiv__), clamped from above by a comparison, not
// fminf: a NaN norm gives a NaN factor (error_if_nonfinite=False); max_norm = +inf gives exactly 1.
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partials, int n, float max_norm, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < n; i += 256) s = s + (double)partials[i];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float norm = (float)sqrt(red[0]);
        const float r = 1.0f / (norm + 1e-6f);
        const float c = r * max_norm;
        out[0] = norm;
        out[1] = c > 1.0f ? 1.0f : c;
    }
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, int64_t n, float lr) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] -= lr * g[i];
}

__global__ void swa_kernel(float* __restrict__ avg, const float* __restrict__ p, int64_t n4, int64_t n, float inv) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 a = ((f32x4*)avg)[i];
        const f32x4 w = ((const f32x4*)p)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = inv == 1.0f ? w[e] : a[e] + (w[e] - a[e]) * inv;
        ((f32x4*)avg)[i] = a;
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        avg[i] = inv == 1.0f ? p[i] : avg[i] + (p[i] - avg[i]) * inv;
}

}  // namespace pa

using namespace pa;

// ---- AdamW, the host side: one builder of the launch's hyper-parameters, one launcher per kernel form.  The seven entries differ in
// what they take and in the checks that are theirs alone.  With the device row (hyper_dev) the kernels take all seven floats from
// there: the by-value ones, and ``step``, are ignored.
static AdamwHyper adamw_hyper_host(float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float* hyper_dev) {
    if (hyper_dev) return AdamwHyper{lr, beta1, beta2, eps, weight_decay, 1.f, 1.f};
    return AdamwHyper{lr, beta1, beta2, eps, weight_decay, 1.f - powf(beta1, (float)step), sqrtf(1.f - powf(beta2, (float)step))};
}
// blocks of 256 threads for a grid-stride loop over ``work`` items (float4s or elements)
static int stream_blocks(int64_t work) { return (int)std::min<int64_t>(cdiv(std::max<int64_t>(work, 1), 256), 8192); }
// n / 4 where every pointer OR-ed into ``ptrs`` is 16-byte aligned, else 0: the kernels' scalar loops take what is left
static int64_t vec4_count(int64_t n, uintptr_t ptrs) { return (ptrs & 15) == 0 ? n / 4 : 0; }

static int launch_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, int step, const float* hyper_dev, bool clip, const float* gscale_dev, void* stream) {
    if (!p || !g || !m || !v || n <= 0 || (!hyper_dev && step < 1)) return PA_EINVAL;
    const AdamwHyper h = adamw_hyper_host(lr, beta1, beta2, eps, weight_decay, step, hyper_dev);
    const int64_t n4 = vec4_count(n, (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v);
    const dim3 grid(stream_blocks(n4)), block(256);
    if (clip) hipLaunchKernelGGL(adamw_flat_kernel<true>, grid, block, 0, (hipStream_t)stream, p, g, m, v, n4, n, h, hyper_dev, gscale_dev);
    else hipLaunchKernelGGL(adamw_flat_kernel<false>, grid, block, 0, (hipStream_t)stream, p, g, m, v, n4, n, h, hyper_dev, gscale_dev);
    return check_launch();
}

static bool table_args_ok(const float* p, const float* g, const float* m, const float* v, const pa_adamw_stage_desc* descs,
                          const float* scales, int n_desc, int total_items, int step, const float* hyper_dev) {
    return p && g && m && v && descs && !((uintptr_t)scales & 7) && n_desc >= 1 && total_items >= 1 && (hyper_dev || step >= 1);
}
// the table kernel of the copies' dtype, with groups where scales are given, with the clip factor where ``clip``
static int launch_table(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, const float* scales, int n_desc,
                        int total_items, int dtype, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                        const float* hyper_dev, bool clip, const float* gscale_dev, void* stream) {
    if (!table_args_ok(p, g, m, v, descs, scales, n_desc, total_items, step, hyper_dev) || (dtype != PA_BF16 && dtype != PA_F32)) return PA_EINVAL;
    const AdamwHyper h = adamw_hyper_host(lr, beta1, beta2, eps, weight_decay, step, hyper_dev);
    const float2* sc = (const float2*)scales;
    const dim3 grid(total_items), block(256);
#define PA_ADAMW_TABLE(TO, GROUPS, CLIP) \
    hipLaunchKernelGGL((adamw_table_kernel<TO, GROUPS, CLIP>), grid, block, 0, (hipStream_t)stream, p, g, m, v, descs, n_desc, hyper_dev, h, sc, gscale_dev)
    switch ((dtype == PA_BF16 ? 4 : 0) | (sc ? 2 : 0) | (clip ? 1 : 0)) {
        case 0: PA_ADAMW_TABLE(float, false, false); break;
        case 1: PA_ADAMW_TABLE(float, false, true); break;
        case 2: PA_ADAMW_TABLE(float, true, false); break;
        case 3: PA_ADAMW_TABLE(float, true, true); break;
        case 4: PA_ADAMW_TABLE(bf16, false, false); break;
        case 5: PA_ADAMW_TABLE(bf16, false, true); break;
        case 6: PA_ADAMW_TABLE(bf16, true, false); break;
        default: PA_ADAMW_TABLE(bf16, true, true); break;
    }
#undef PA_ADAMW_TABLE
    return check_launch();
}

extern "C" int pa_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int step, void* stream) {
    return launch_flat(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, nullptr, false, nullptr, stream);
}

extern "C" int pa_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* stream) {
    if (!hyper) return PA_EINVAL;
    return launch_flat(p, g, m, v, n, 0.f, 0.f, 0.f, 0.f, 0.f, 0, hyper, false, nullptr, stream);
}

extern "C" int pa_adamw_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int step, const float* hyper_dev, const float* gscale_dev, void* stream) {
    return launch_flat(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, hyper_dev, true, gscale_dev, stream);
}

extern "C" int pa_adamw_stage(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, int n_desc,
                              int total_items, int dtype, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                              const float* hyper_dev, void* stream) {
    return launch_table(p, g, m, v, descs, nullptr, n_desc, total_items, dtype, lr, beta1, beta2, eps, weight_decay, step, hyper_dev, false,
                        nullptr, stream);
}

extern "C" int pa_adamw_stage_groups(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, const float* scales,
                                     int n_desc, int total_items, int dtype, float lr, float beta1, float beta2, float eps,
                                     float weight_decay, int step, const float* hyper_dev, void* stream) {
    if (!scales) return PA_EINVAL;
    return launch_table(p, g, m, v, descs, scales, n_desc, total_items, dtype, lr, beta1, beta2, eps, weight_decay, step, hyper_dev, false,
                        nullptr, stream);
}

extern "C" int pa_adamw_groups(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, const float* scales,
                               int n_desc, int total_items, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                               const float* hyper_dev, void* stream) {
    if (!scales || !table_args_ok(p, g, m, v, descs, scales, n_desc, total_items, step, hyper_dev)) return PA_EINVAL;
    const AdamwHyper h = adamw_hyper_host(lr, beta1, beta2, eps, weight_decay, step, hyper_dev);
    hipLaunchKernelGGL(adamw_groups_kernel, dim3(total_items), dim3(256), 0, (hipStream_t)stream, p, g, m, v, descs, n_desc, hyper_dev, h,
                       (const float2*)scales);
    return check_launch();
}

extern "C" int pa_adamw_stage_clip(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, const float* scales,
                                   int n_desc, int total_items, int dtype, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int step, const float* hyper_dev, const float* gscale_dev, void* stream) {
    return launch_table(p, g, m, v, descs, scales, n_desc, total_items, dtype, lr, beta1, beta2, eps, weight_decay, step, hyper_dev, true,
                        gscale_dev, stream);
}

extern "C" int64_t pa_grad_norm_partials(int64_t n) { return n <= 0 ? 0 : cdiv(n, GN_CHUNK); }

extern "C" int pa_grad_accum_sumsq(const float* g, float* acc, int first, int64_t n, float* partials, void* stream) {
    if (!g || n <= 0 || (!acc && !partials)) return PA_EINVAL;
    const int64_t chunks = cdiv(n, GN_CHUNK);
    if (chunks > 0x7fffffff) return PA_EINVAL;
    hipLaunchKernelGGL(grad_accum_sumsq_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, g, acc, first, n, partials);
    return check_launch();
}

extern "C" int pa_clip_coef(const float* partials, int n_partials, float max_norm, float* out, void* stream) {
    if (!partials || !out || n_partials < 1 || !(max_norm > 0.f)) return PA_EINVAL;
    hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, max_norm, out);
    return check_launch();
}

extern "C" void pa_adamw_hyper(float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* hyper7_host) {
    const AdamwHyper h = adamw_hyper_host(lr, beta1, beta2, eps, weight_decay, step, nullptr);
    static_assert(sizeof(h) == 7 * sizeof(float), "AdamwHyper is the 7-float row");
    memcpy(hyper7_host, &h, sizeof(h));
}

extern "C" int pa_swa_update(float* avg, const float* p, int64_t n, int num_averaged, void* stream) {
    if (!avg || !p || n <= 0 || num_averaged < 0) return PA_EINVAL;
    const int64_t n4 = vec4_count(n, (uintptr_t)avg | (uintptr_t)p);
    // the reference divides by (n + 1); a reciprocal multiply differs by <= 1 ulp of the increment
    hipLaunchKernelGGL(swa_kernel, dim3(stream_blocks(n4)), dim3(256), 0, (hipStream_t)stream, avg, p, n4, n, 1.0f / (float)(num_averaged + 1));
    return check_launch();
}

extern "C" int pa_sgd(float* p, const float* g, int64_t n, float lr, void* stream) {
    if (!p || !g || n <= 0) return PA_EINVAL;
    hipLaunchKernelGGL(sgd_kernel, dim3(stream_blocks(n)), dim3(256), 0, (hipStream_t)stream, p, g, n, lr);
    return check_launch();
}

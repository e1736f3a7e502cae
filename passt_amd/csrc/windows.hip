// Sliding-window inference over long recordings (PaSST.forward_windows): the two kernels around the packed trunk.
//   pa_patch_gather_windows  the packed im2col of pa_patch_gather_varlen with the sequence looked up through a window table: a
//                            window is (recording, first frame, frames) of a longer recording, read in place -- no unfolded copy
//   pa_window_pool           mean / max of every recording's own windows, of the raw values or of their sigmoid, rows in order
// Both are bandwidth-trivial next to the trunk (a window's patches are read once, the pooled rows are a few KB), so they are plain:
// scalar accesses, no alignment assumed anywhere (win_t0 and the pitch are arbitrary), every index checked before it is used.
#include "pa_common.h"

namespace pa {

// one workgroup (P*P threads) per token row: cols[r][i*P+j] = x[win_src[w]][row_f*fs+i][win_t0[w] + row_t*ts + j], w = row_win[r].
// A prefix row (row_f < 0) is zero; so is every element whose frame is not inside the window [win_t0, win_t0 + win_len) or whose
// window / recording / coordinate is outside the arrays (memory safety, not a contract).  The frame index is formed in 64 bits.
template <typename T>
__global__ void patch_gather_windows_kernel(const float* __restrict__ x, int B, int F, int Tt, const int32_t* __restrict__ win_src,
                                            const int32_t* __restrict__ win_t0, const int32_t* __restrict__ win_len, int W,
                                            const int32_t* __restrict__ row_win, const int32_t* __restrict__ row_f,
                                            const int32_t* __restrict__ row_t, int P, int fs, int ts, T* __restrict__ cols) {
    const int r = blockIdx.x;
    const int i = threadIdx.x / P, j = threadIdx.x % P;
    const int w = row_win[r], pf = row_f[r];
    float v = 0.f;
    if (pf >= 0 && (unsigned)w < (unsigned)W) {
        const int c = win_src[w], t0 = win_t0[w], n = win_len[w];
        const int64_t f = (int64_t)pf * fs + i, dt = (int64_t)row_t[r] * ts + j;        // dt: the frame inside the window
        if ((unsigned)c < (unsigned)B && f < F && t0 >= 0 && dt >= 0 && dt < n && t0 + dt < Tt) v = x[((int64_t)c * F + f) * Tt + t0 + dt];
    }
    cols[(int64_t)r * (P * P) + threadIdx.x] = from_f32<T>(v);
}

// what pa_eval_append ranks: f32 1 / (1 + exp(-z)), exp(-z) rounded to f32 once from an f64 evaluation
__device__ __forceinline__ float sigmoid_f32(float z) { return 1.0f / (1.0f + (float)exp(-(double)z)); }

// one thread per (recording, column): the recording's rows offsets[b] .. offsets[b + 1] - 1 in row order, f32.  The max starts from
// the first row; the mean divides by the recording's own count.  An empty recording (the host entry cannot see the offsets) and
// rows outside [0, W) are not read: the empty one gets NaN.
template <bool MAX, bool SIGMOID>
__global__ __launch_bounds__(256) void window_pool_kernel(const float* __restrict__ in, int W, int C, const int32_t* __restrict__ offsets,
                                                          int B, float* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (int64_t)B * C) return;
    const int b = (int)(k / C), c = (int)(k % C);
    const int lo = max(offsets[b], 0), hi = min(offsets[b + 1], W);
    if (lo >= hi) {
        out[k] = __int_as_float(0x7fc00000);
        return;
    }
    auto at = [&](int w) {
        const float v = in[(int64_t)w * C + c];
        return SIGMOID ? sigmoid_f32(v) : v;
    };
    float acc = at(lo);
    for (int w = lo + 1; w < hi; ++w) {
        const float v = at(w);
        if (MAX) acc = (v > acc || v != v) ? v : acc;        // a NaN row makes the maximum NaN, as torch.max does
        else acc += v;
    }
    if (MAX) out[k] = acc;
    else out[k] = acc / (float)(hi - lo);
}

}  // namespace pa

using namespace pa;

extern "C" int pa_patch_gather_windows(const float* x, int B, int F, int T_pitch, const int32_t* win_src, const int32_t* win_t0,
                                       const int32_t* win_len, int W, const int32_t* row_win, const int32_t* row_f, const int32_t* row_t,
                                       int M, int P, int fstride, int tstride, void* cols, int dtype, void* stream) {
    if (!x || !win_src || !win_t0 || !win_len || !row_win || !row_f || !row_t || !cols) return PA_EINVAL;
    if (B <= 0 || F <= 0 || T_pitch <= 0 || W <= 0 || M <= 0 || P <= 0 || fstride <= 0 || tstride <= 0) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    if (P * P > 1024) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)M), block((unsigned)(P * P));
    if (dtype == PA_BF16)
        hipLaunchKernelGGL(patch_gather_windows_kernel<bf16>, grid, block, 0, (hipStream_t)stream, x, B, F, T_pitch, win_src, win_t0, win_len, W,
                           row_win, row_f, row_t, P, fstride, tstride, (bf16*)cols);
    else
        hipLaunchKernelGGL(patch_gather_windows_kernel<float>, grid, block, 0, (hipStream_t)stream, x, B, F, T_pitch, win_src, win_t0, win_len, W,
                           row_win, row_f, row_t, P, fstride, tstride, (float*)cols);
    return check_launch();
}

extern "C" int pa_window_pool(const float* in, int W, int C, const int32_t* offsets, int B, int mode, int act, float* out, void* stream) {
    if (!in || !offsets || !out || W <= 0 || C <= 0 || B <= 0) return PA_EINVAL;
    if (B > W) return PA_EINVAL;                 // more recordings than windows: one of them is empty
    if ((mode != PA_POOL_MEAN && mode != PA_POOL_MAX) || (act != PA_POOL_ACT_NONE && act != PA_POOL_ACT_SIGMOID)) return PA_EINVAL;
    const dim3 grid((unsigned)cdiv((int64_t)B * C, 256)), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (mode == PA_POOL_MAX) {
        if (act == PA_POOL_ACT_SIGMOID) hipLaunchKernelGGL((window_pool_kernel<true, true>), grid, block, 0, st, in, W, C, offsets, B, out);
        else hipLaunchKernelGGL((window_pool_kernel<true, false>), grid, block, 0, st, in, W, C, offsets, B, out);
    } else {
        if (act == PA_POOL_ACT_SIGMOID) hipLaunchKernelGGL((window_pool_kernel<false, true>), grid, block, 0, st, in, W, C, offsets, B, out);
        else hipLaunchKernelGGL((window_pool_kernel<false, false>), grid, block, 0, st, in, W, C, offsets, B, out);
    }
    return check_launch();
}

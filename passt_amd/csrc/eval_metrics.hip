// Validation metrics of the callers (ex_audioset.py:245-291, ex_openmic.py:228-270, ex_fsd50k.py:220-260): per-class average
// precision and ROC-AUC without a sort, as exact integer rank counts per positive sample.
//   pa_eval_append  one validation batch [B][C] -> class-major columns [C][capacity]: an order-preserving u32 key of the score
//                   and a one-byte state per element
//   pa_eval_rank    compact each class's valid positives and negatives, count for every positive the positives / negatives
//                   ranked at or above it, finish AP and AUC in f64
// Everything behind the key is integer arithmetic, so neither the f32 denormal mode nor the order of the counts matters; the
// only floating-point sum (the AP ratios) runs in index order and is bit-identical from run to run.
#include <algorithm>

#include "pa_common.h"

namespace pa {

enum : uint8_t { EV_EXCLUDED = 0, EV_NEG = 1, EV_POS = 2, EV_NAN = 3 };
static constexpr int EV_TILE = 256;        // positives per work item: one per thread
static constexpr int EV_CHUNK = 1024;      // compared keys staged in LDS at a time

// float bits -> u32 whose unsigned order is the float order; -0 folds onto +0 (they compare equal as floats)
__device__ __forceinline__ uint32_t score_key(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// 64 classes x 64 samples per block through LDS: reads run along the classes of a sample (the batch's rows), writes along the
// samples of a class (the buffers' rows).  n0 is arbitrary, so the stores are 4- and 1-byte ones.
template <bool SIGMOID>
__global__ __launch_bounds__(256) void eval_append_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                          const float* __restrict__ mask, int B, int C, int64_t n0, int64_t cap,
                                                          uint32_t* __restrict__ keys, uint8_t* __restrict__ state) {
    __shared__ uint32_t tk[64][65];
    __shared__ uint8_t ts[64][68];
    const int c0 = blockIdx.x * 64, b0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int b = b0 + r, c = c0 + tx;
        if (b < B && c < C) {
            const int64_t i = (int64_t)b * C + c;
            uint32_t bits;
            if constexpr (SIGMOID) {
                // what the reference ranks (ex_audioset.py:238): f32 1 / (1 + exp(-z)), with exp(-z) rounded to f32 ONCE from an f64
                // evaluation (a correctly rounded expf, as a host libm's is), an f32 add and an IEEE f32 division
                const float e = (float)exp(-(double)logits[i]);
                bits = __float_as_uint(1.0f / (1.0f + e));
            } else {
                bits = ((const uint32_t*)logits)[i];          // verbatim: no float instruction sees it
            }
            const bool valid = mask == nullptr || mask[i] > 0.5f;
            const bool isnan = (bits & 0x7fffffffu) > 0x7f800000u;
            tk[r][tx] = score_key(bits);
            ts[r][tx] = !valid ? EV_EXCLUDED : isnan ? EV_NAN : target[i] > 0.5f ? EV_POS : EV_NEG;
        }
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int c = c0 + r, b = b0 + tx;
        if (c < C && b < B) {
            const int64_t o = (int64_t)c * cap + n0 + b;
            keys[o] = tk[tx][r];
            state[o] = ts[tx][r];
        }
    }
}

// One block per class: order-preserving compaction of the valid positives' and the valid negatives' keys (ballot ranks inside a
// wave, the four waves' totals through LDS).  cnt[c] = {P, Nn, a NaN score seen, 0}.
__global__ __launch_bounds__(256) void eval_compact_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ state, int64_t n,
                                                           int64_t cap, uint32_t* __restrict__ pos, uint32_t* __restrict__ neg,
                                                           int32_t* __restrict__ cnt, int64_t* __restrict__ n_pos, int64_t* __restrict__ n_neg) {
    __shared__ int wp[4], wn[4];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t row = (int64_t)c * cap;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int base_p = 0, base_n = 0, seen_nan = 0;
    for (int64_t base = 0; base < n; base += 256) {
        const int64_t i = base + tid;
        const uint8_t st = i < n ? state[row + i] : (uint8_t)EV_EXCLUDED;
        const bool isp = st == EV_POS, isn = st == EV_NEG;
        seen_nan |= st == EV_NAN;
        const uint64_t bp = __ballot(isp), bn = __ballot(isn);
        if (lane == 0) { wp[w] = __popcll(bp); wn[w] = __popcll(bn); }
        __syncthreads();
        int op = 0, on = 0, tp = 0, tn = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k < w) { op += wp[k]; on += wn[k]; }
            tp += wp[k]; tn += wn[k];
        }
        if (isp) pos[row + base_p + op + __popcll(bp & below)] = keys[row + i];
        if (isn) neg[row + base_n + on + __popcll(bn & below)] = keys[row + i];
        base_p += tp; base_n += tn;
        __syncthreads();
    }
    seen_nan = __syncthreads_or(seen_nan);
    if (tid == 0) {
        cnt[4 * c] = base_p; cnt[4 * c + 1] = base_n; cnt[4 * c + 2] = seen_nan != 0; cnt[4 * c + 3] = 0;
        n_pos[c] = base_p; n_neg[c] = base_n;
    }
}

// The work-item map: tile_start[c] = number of 256-positive tiles of the classes in front of c (exclusive scan; tile_start[C] =
// all of them).  One block; C is a few hundred.
__global__ __launch_bounds__(256) void eval_map_kernel(const int32_t* __restrict__ cnt, int C, int32_t* __restrict__ tile_start) {
    __shared__ int s[256];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int c0 = 0; c0 < C; c0 += 256) {
        const int c = c0 + tid;
        const int mine = c < C ? (cnt[4 * c] + EV_TILE - 1) / EV_TILE : 0;
        s[tid] = mine;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = tid >= o ? s[tid - o] : 0;
            __syncthreads();
            s[tid] += v;
            __syncthreads();
        }
        if (c < C) tile_start[c] = carry + s[tid] - mine;
        carry += s[255];
        __syncthreads();
    }
    if (tid == 0) tile_start[C] = carry;
}

// One work item = 256 consecutive positives of one class (one per thread, key in a register) against ALL of that class's
// compacted keys, streamed through LDS 1024 at a time (every lane reads the same four keys: a broadcast).  The cost of a class is
// ceil(P / 256) * (P + Nn) lane-compares: it scales with the positives.  A fixed grid walks the items; the item's class comes
// from a binary search in tile_start.  Per item: the f64 sum of the tile's GEp / (GEp + GEn) in index order, and the integer sum
// of 2 (Nn - GEn) + (GEn - GTn).
__global__ __launch_bounds__(256) void eval_count_kernel(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ neg,
                                                         const int32_t* __restrict__ cnt, const int32_t* __restrict__ tile_start, int C,
                                                         int64_t cap, double* __restrict__ tile_ap, int64_t* __restrict__ tile_num) {
    __shared__ __attribute__((aligned(16))) uint32_t chunk[EV_CHUNK];
    __shared__ double red_ap[EV_TILE];
    __shared__ int64_t red_num[EV_TILE];
    const int tid = threadIdx.x;
    const int total = tile_start[C];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        int lo = 0, hi = C;                       // tile_start[lo] <= item < tile_start[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (tile_start[mid] <= item) lo = mid; else hi = mid;
        }
        const int c = lo, P = cnt[4 * c], Nn = cnt[4 * c + 1];
        const int64_t row = (int64_t)c * cap;
        const int first = (item - tile_start[c]) * EV_TILE, i = first + tid;
        const bool act = i < P;
        const uint32_t k = act ? pos[row + i] : 0xffffffffu;
        uint32_t gep = 0, gen = 0, gtn = 0;
        for (int base = 0; base < P; base += EV_CHUNK) {
            const int m = min(EV_CHUNK, P - base);
            __syncthreads();
            for (int j = tid; j < ((m + 3) & ~3); j += 256) chunk[j] = j < m ? pos[row + base + j] : 0u;      // key 0 is below every stored key
            __syncthreads();
            for (int j = 0; j < m; j += 4) {
                const uint4 q = *(const uint4*)&chunk[j];
                gep += (q.x >= k) + (q.y >= k) + (q.z >= k) + (q.w >= k);
            }
        }
        for (int base = 0; base < Nn; base += EV_CHUNK) {
            const int m = min(EV_CHUNK, Nn - base);
            __syncthreads();
            for (int j = tid; j < ((m + 3) & ~3); j += 256) chunk[j] = j < m ? neg[row + base + j] : 0u;
            __syncthreads();
            for (int j = 0; j < m; j += 4) {
                const uint4 q = *(const uint4*)&chunk[j];
                gen += (q.x >= k) + (q.y >= k) + (q.z >= k) + (q.w >= k);
                gtn += (q.x > k) + (q.y > k) + (q.z > k) + (q.w > k);
            }
        }
        red_ap[tid] = act ? (double)gep / ((double)gep + (double)gen) : 0.0;
        red_num[tid] = act ? 2 * ((int64_t)Nn - gen) + ((int64_t)gen - gtn) : 0;
        __syncthreads();
        if (tid == 0) {
            const int m = min(EV_TILE, P - first);
            double a = 0.0;
            int64_t s = 0;
            for (int j = 0; j < m; ++j) { a += red_ap[j]; s += red_num[j]; }
            tile_ap[item] = a;
            tile_num[item] = s;
        }
        __syncthreads();
    }
}

// One thread per class: the tiles' partial sums in tile order, then the two divisions and scikit-learn's conventions for
// degenerate classes (P = 0: AP 0.0; P = 0 or Nn = 0: AUC NaN) and ours for a NaN score (both NaN).
__global__ __launch_bounds__(256) void eval_finish_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ tile_start,
                                                          const double* __restrict__ tile_ap, const int64_t* __restrict__ tile_num, int C,
                                                          int64_t* __restrict__ auc_num, double* __restrict__ ap, double* __restrict__ auc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int64_t P = cnt[4 * c], Nn = cnt[4 * c + 1];
    double a = 0.0;
    int64_t s = 0;
    for (int t = tile_start[c]; t < tile_start[c + 1]; ++t) { a += tile_ap[t]; s += tile_num[t]; }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool bad = cnt[4 * c + 2] != 0;
    auc_num[c] = s;
    ap[c] = bad ? nan : P > 0 ? a / (double)P : 0.0;
    auc[c] = bad || P == 0 || Nn == 0 ? nan : (double)s / (2.0 * (double)P * (double)Nn);
}

struct EvalWs {
    int64_t pos, neg, cnt, tile_start, tile_ap, tile_num, bytes;
    int64_t max_tiles;
};
static bool eval_ws_layout(int C, int64_t cap, EvalWs& w) {
    if (C < 1 || cap < 1 || cap > 0x7fffffff) return false;
    w.max_tiles = (int64_t)C * cdiv(cap, EV_TILE);
    if (w.max_tiles > 0x7fffffff) return false;
    auto up = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
    int64_t o = 0;
    w.pos = o; o = up(o + (int64_t)C * cap * 4);
    w.neg = o; o = up(o + (int64_t)C * cap * 4);
    w.cnt = o; o = up(o + (int64_t)C * 16);
    w.tile_start = o; o = up(o + ((int64_t)C + 1) * 4);
    w.tile_ap = o; o = up(o + w.max_tiles * 8);
    w.tile_num = o; o = up(o + w.max_tiles * 8);
    w.bytes = o;
    return true;
}

}  // namespace pa

using namespace pa;

extern "C" int pa_eval_append(const float* scores, const float* target, const float* mask, int B, int C, int64_t n0, int64_t capacity,
                              int mode, uint32_t* keys, uint8_t* state, void* stream) {
    if (!scores || !target || !keys || !state || B < 1 || C < 1 || n0 < 0 || capacity < 1 || n0 + B > capacity) return PA_EINVAL;
    if (mode != PA_EVAL_SIGMOID && mode != PA_EVAL_RAW) return PA_EINVAL;
    if (capacity > 0x7fffffff || cdiv(B, 64) > 65535) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)cdiv(C, 64), (unsigned)cdiv(B, 64));
    hipStream_t st = (hipStream_t)stream;
    if (mode == PA_EVAL_SIGMOID)
        hipLaunchKernelGGL(eval_append_kernel<true>, grid, dim3(256), 0, st, scores, target, mask, B, C, n0, capacity, keys, state);
    else
        hipLaunchKernelGGL(eval_append_kernel<false>, grid, dim3(256), 0, st, scores, target, mask, B, C, n0, capacity, keys, state);
    return check_launch();
}

extern "C" int64_t pa_eval_ws_bytes(int C, int64_t capacity) {
    EvalWs w;
    return eval_ws_layout(C, capacity, w) ? w.bytes : 0;
}

extern "C" int pa_eval_rank(const uint32_t* keys, const uint8_t* state, int C, int64_t n, int64_t capacity, void* ws, int64_t* n_pos,
                            int64_t* n_neg, int64_t* auc_num, double* ap, double* auc, void* stream) {
    if (!keys || !state || !ws || !n_pos || !n_neg || !auc_num || !ap || !auc || C < 1 || n < 0 || capacity < 1 || n > capacity)
        return PA_EINVAL;
    EvalWs w;
    if (!eval_ws_layout(C, capacity, w)) return PA_EUNSUPPORTED;
    if (((uintptr_t)ws & 15) != 0) return PA_EINVAL;
    char* base = (char*)ws;
    uint32_t* pos = (uint32_t*)(base + w.pos);
    uint32_t* neg = (uint32_t*)(base + w.neg);
    int32_t* cnt = (int32_t*)(base + w.cnt);
    int32_t* tile_start = (int32_t*)(base + w.tile_start);
    double* tile_ap = (double*)(base + w.tile_ap);
    int64_t* tile_num = (int64_t*)(base + w.tile_num);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_compact_kernel, dim3(C), dim3(256), 0, st, keys, state, n, capacity, pos, neg, cnt, n_pos, n_neg);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(eval_map_kernel, dim3(1), dim3(256), 0, st, cnt, C, tile_start);
    if ((rc = check_launch())) return rc;
    // a fixed grid (the tile counts live on the device: no host sync) walks the items; 8 blocks per CU of a 256-CU chip at most
    const int64_t n_tiles = (int64_t)C * cdiv(std::max<int64_t>(n, 1), EV_TILE);
    const int blocks = (int)std::min<int64_t>(n_tiles, 2048);
    hipLaunchKernelGGL(eval_count_kernel, dim3(blocks), dim3(256), 0, st, pos, neg, cnt, tile_start, C, capacity, tile_ap, tile_num);
    if ((rc = check_launch())) return rc;
    hipLaunchKernelGGL(eval_finish_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, st, cnt, tile_start, tile_ap, tile_num, C, auc_num,
                       ap, auc);
    return check_launch();
}

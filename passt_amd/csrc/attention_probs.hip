// Attention probabilities softmax(q k^T * scale) written out, for gfx950: what a forward hook on the reference's
// blocks[i].attn.attn_drop sees (models/passt.py:348-352).  The fused forward (attention.hip) never lets a score reach
// memory, but it leaves lse = log sum_k exp(score) per query row next to qkv, so a probability is
//   p[q][k] = exp2(s~[q][k] - lse[q] * log2 e),   s~ = q k^T * scale * log2 e
// and any (query tile, key tile) pair stands alone: no online softmax, no second pass, no atomics, no LDS.
//
// One wave = one 32 x 32 tile of one (sequence, head).  Unlike the fused kernels the product is taken in the orientation
// S[q][key] (A operand = Q rows, B operand = K rows), so the accumulator holds 32 consecutive KEYS in 32 consecutive lanes
// (col = lane & 31) and a query row per register: every register is stored as two 128-byte pieces of two output rows,
// straight from the registers.  The Q / K fragments come from global memory directly (each is used by one product).
// The tile itself -- fragment loads, the hi + lo exponent, the f32 score as four short MFMA chains, key lanes at or behind N masked
// before the exponential -- comes from pa_attn_tile.h, which the gradient / CAM and the rollout kernels share.
// Head mean: the wave loops the heads in order and adds the probabilities in f32 registers (deterministic).
// Key lanes at or behind N are never stored; rows are clamped to the sequence's own last query / key row, so the packed form reads
// no row of a neighbour and none behind cu_tok[B].
#include "pa_attn_tile.h"

namespace pa {

// Work item -> (key tile, query tile, sequence x output head), key tile fastest: neighbouring workgroups write neighbouring
// pieces of the same output rows.  VL: sequences packed back to back (cu_tok), N / nq hold max N and the caller's nq; the
// tiles a short sequence does not have return before their first memory access.
template <typename T, bool PRE, bool VL>
__global__ __launch_bounds__(256) void attn_probs_kernel(const T* __restrict__ qkv, int ldqkv, const float* __restrict__ lse,
                                                         float* __restrict__ out, const int32_t* __restrict__ cu_tok,
                                                         const int64_t* __restrict__ out_off, int B, int H, int N, int nq, int nkt,
                                                         int nqt, int head_mean, float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int L = blockIdx.x;
    const int kt = L % nkt;
    L /= nkt;
    const int qt = L % nqt;
    const int z = L / nqt;
    const int Ho = head_mean ? 1 : H, nh = head_mean ? H : 1;
    const int b = z / Ho, h0 = z - b * Ho;

    const SeqGeom g = seq_geom<VL>(b, B, H, N, nq, cu_tok, lse, 0);
    N = g.N;
    nq = g.nq;
    float* out_b = VL ? out + out_off[b] : out + (int64_t)b * Ho * nq * N;
    const int q0 = qt * AT_QT, k0 = kt * AT_KT + wave * 32;
    if (q0 >= nq || k0 >= N) return;                             // (also N <= 0) wave-uniform; the kernel has no barrier

    const int r32 = lane & 31, half = lane >> 5;
    const int qrow = min(q0 + r32, nq - 1), krow = min(k0 + r32, N - 1);
    const bool klive = k0 + r32 < N;
    float sl2, sl2_lo;
    scale_log2e(scale, sl2, sl2_lo);
    const int D = H * AT_HD;
    int qr[16];
    tile_query_rows(qr, q0, nq, lane);

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int hh = 0; hh < nh; ++hh) {
        const int h = h0 + hh;
        const T* base = qkv + g.tok0 * ldqkv + h * AT_HD;         // q of token 0 of this (sequence, head)
        f32x16 p;
        tile_probs<T, PRE>(p, base + (int64_t)qrow * ldqkv, base + D + (int64_t)krow * ldqkv, g.lse_b + (int64_t)h * g.lse_pitch, qr,
                           klive, sl2, sl2_lo, half);
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] += p[i];
    }
    const float mul = head_mean ? 1.0f / (float)H : 1.0f;
    float* o = out_b + ((int64_t)h0 * nq) * N + k0 + r32;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int q = q0 + acc_row(i, lane);
        if (klive && q < nq) o[(int64_t)q * N] = acc[i] * mul;
    }
}

template <typename T>
static int attention_probs_t(const void* qkv, int ldqkv, const float* lse, float* out, const int32_t* cu_tok, const int64_t* out_off,
                             int B, int H, int N, int nq, int head_mean, float scale, int flags, hipStream_t st) {
    const int nqk = nq >= N ? N : nq;
    const int nkt = (int)cdiv(N, AT_KT), nqt = (int)cdiv(nqk, AT_QT);
    const int64_t items = (int64_t)nkt * nqt * B * (head_mean ? 1 : H);
    if (items >= (int64_t)1 << 31) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)items), block(256);
    const bool pre = flags & PA_ATTN_Q_PRESCALED;
#define PA_PROBS_LAUNCH(PRE_, VL_)                                                                                                \
    hipLaunchKernelGGL((attn_probs_kernel<T, PRE_, VL_>), grid, block, 0, st, (const T*)qkv, ldqkv, lse, out, cu_tok, out_off, B, H, \
                       N, nqk, nkt, nqt, head_mean, scale)
    if (cu_tok) {
        if (pre) PA_PROBS_LAUNCH(true, true);
        else PA_PROBS_LAUNCH(false, true);
    } else {
        if (pre) PA_PROBS_LAUNCH(true, false);
        else PA_PROBS_LAUNCH(false, false);
    }
#undef PA_PROBS_LAUNCH
    return check_launch();
}

}  // namespace pa

using namespace pa;

extern "C" int pa_attention_probs(const void* qkv, int ldqkv, const float* lse, float* out, const int32_t* cu_tok, const int64_t* out_off,
                                  int B, int H, int N, int nq, int head_mean, float scale, int dtype, int flags, void* stream) {
    if (!qkv || !lse || !out || B <= 0 || H <= 0 || N <= 0 || nq <= 0 || (flags & ~PA_ATTN_Q_PRESCALED) || (head_mean & ~1))
        return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    if (cu_tok ? !out_off : (out_off != nullptr || nq > N)) return PA_EINVAL;      // the offsets belong to the packed layout
    if (ldqkv < 3 * H * AT_HD) return PA_EINVAL;
    if ((ldqkv * (dtype == PA_BF16 ? 2 : 4)) % 16 != 0) return PA_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PA_BF16) return attention_probs_t<bf16>(qkv, ldqkv, lse, out, cu_tok, out_off, B, H, N, nq, head_mean, scale, flags, st);
    return attention_probs_t<float>(qkv, ldqkv, lse, out, cu_tok, out_off, B, H, N, nq, head_mean, scale, flags, st);
}

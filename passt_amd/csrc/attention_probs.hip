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
// The exponent s~ - lse * log2 e is formed so that the kernel's own error stays at a few f32 ulps of the score: lse * log2 e as
// a hi + lo pair, the cancellation in one fma, and the f32 score summed as four short MFMA chains instead of one long one.
// Head mean: the wave loops the heads in order and adds the probabilities in f32 registers (deterministic).
// Key lanes at or behind N are masked to -inf BEFORE the exponential (exp2(0 - lse * log2 e) overflows for strongly negative
// scores) and are never stored; rows are clamped to the sequence's own last query / key row, so the packed form reads no row of
// a neighbour and none behind cu_tok[B].
//
// KEEP IN STEP: attn_probs_grad_kernel (attention_probs_grad.hip) and attn_rollout_kernel (attention_rollout.hip) form their probability tiles with a copy of this kernel's
// arithmetic, operation for operation, and their tests rest on that: change it in all three files or in none.
#include "pa_mma.h"

namespace pa {

static constexpr int P_HD = 64;                                  // head dim
static constexpr double P_LOG2E_D = 1.4426950408889634;
static constexpr float P_LOG2E = (float)P_LOG2E_D, P_LOG2E_LO = (float)(P_LOG2E_D - (double)P_LOG2E);      // log2 e = hi + lo
static constexpr int P_KT = 128, P_QT = 32;                       // keys / queries per workgroup (4 waves x 32 keys)

// Work item -> (key tile, query tile, sequence x output head), key tile fastest: neighbouring workgroups write neighbouring
// pieces of the same output rows.  VL: sequences packed back to back (cu_tok), N / nq hold max N and the caller's nq; the
// tiles a short sequence does not have return before their first memory access.
template <typename T, bool PRE, bool VL>
__global__ __launch_bounds__(256) void attn_probs_kernel(const T* __restrict__ qkv, int ldqkv, const float* __restrict__ lse,
                                                         float* __restrict__ out, const int32_t* __restrict__ cu_tok,
                                                         const int64_t* __restrict__ out_off, int B, int H, int N, int nq, int nkt,
                                                         int nqt, int head_mean, float scale) {
    using F = typename Frag<T>::type;
    constexpr int NF = P_HD * (int)sizeof(T) / 32;                // 16-byte fragments per lane and row: 4 (bf16) / 8 (f32)
    constexpr int EPC = 16 / (int)sizeof(T);
    constexpr int NC = sizeof(T) == 4 ? 4 : 1;                    // accumulation chains per score (see below)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int L = blockIdx.x;
    const int kt = L % nkt;
    L /= nkt;
    const int qt = L % nqt;
    const int z = L / nqt;
    const int Ho = head_mean ? 1 : H, nh = head_mean ? H : 1;
    const int b = z / Ho, h0 = z - b * Ho;

    int64_t tok0 = (int64_t)b * N;                               // first token row of this sequence in qkv
    const float* lse_b = lse + (int64_t)b * H * nq;              // lse of (head 0, query 0) of this sequence
    int64_t lse_pitch = nq;                                      // floats between two heads
    float* out_b = out;
    if constexpr (VL) {
        const int t0 = cu_tok[b], t1 = cu_tok[b + 1];            // wave-uniform: scalar loads
        const bool all_queries = nq >= N;                        // N is max N here
        N = t1 - t0;
        tok0 = t0;
        if (all_queries) {
            lse_pitch = cu_tok[B];
            lse_b = lse + t0;
        }
        nq = min(nq, N);
        out_b = out + out_off[b];
    } else {
        out_b = out + (int64_t)b * Ho * nq * N;
    }
    const int q0 = qt * P_QT, k0 = kt * P_KT + wave * 32;
    if (q0 >= nq || k0 >= N) return;                             // (also N <= 0) wave-uniform; the kernel has no barrier

    const int r32 = lane & 31, half = lane >> 5;
    const int qrow = min(q0 + r32, nq - 1), krow = min(k0 + r32, N - 1);
    const bool klive = k0 + r32 < N;
    const double sl2d = (double)scale * P_LOG2E_D;                // scale * log2 e as hi + lo floats (used when q is not pre-scaled)
    const float sl2 = (float)sl2d, sl2_lo = (float)(sl2d - (double)sl2);
    const int D = H * P_HD;
    int qr[16];                                                  // the (clamped) query row of every accumulator register
#pragma unroll
    for (int i = 0; i < 16; ++i) qr[i] = min(q0 + acc_row(i, lane), nq - 1);

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int hh = 0; hh < nh; ++hh) {
        const int h = h0 + hh;
        const T* base = qkv + tok0 * ldqkv + h * P_HD;           // q of token 0 of this (sequence, head)
        const float* lse_h = lse_b + (int64_t)h * lse_pitch;
        F qf[NF], kf[NF];
#pragma unroll
        for (int s = 0; s < NF; ++s) {
            const int off = (s * 2 + half) * EPC;
            qf[s] = *(const F*)(base + (int64_t)qrow * ldqkv + off);
            kf[s] = *(const F*)(base + D + (int64_t)krow * ldqkv + off);
        }
        // -lse * log2 e as an unevaluated sum c + cl: |lse| of ~100 leaves a float product half an ulp of ~1e-5 off, which would be
        // the relative error of every probability of the row
        f32x16 c, cl;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float nl = -lse_h[qr[i]];
            c[i] = nl * P_LOG2E;
            cl[i] = fmaf(nl, P_LOG2E, -c[i]) + nl * P_LOG2E_LO;
        }
        // NC independent accumulation chains over the head dim, added pairwise: a chain's rounding errors are half ulps of its
        // own partial sums, so four short f32 chains leave well under half the error of one chain of 32 MFMAs
        f32x16 sc[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            mma32_first<T>(sc[j], qf[j * (NF / NC)], kf[j * (NF / NC)]);
#pragma unroll
            for (int st = 1; st < NF / NC; ++st) mma32<T>(sc[j], qf[j * (NF / NC) + st], kf[j * (NF / NC) + st]);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float s = sc[0][i];
            if constexpr (NC == 4) s = (sc[0][i] + sc[1][i]) + (sc[2][i] + sc[3][i]);
            // s~ - lse * log2 e: the large parts cancel in one fma, the low parts follow
            float a = PRE ? (s + c[i]) + cl[i] : fmaf(s, sl2, c[i]) + fmaf(s, sl2_lo, cl[i]);
            a = klive ? a : -INFINITY;
            acc[i] += __builtin_amdgcn_exp2f(a);
        }
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
    const int nkt = (int)cdiv(N, P_KT), nqt = (int)cdiv(nqk, P_QT);
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
    if (ldqkv < 3 * H * P_HD) return PA_EINVAL;
    if ((ldqkv * (dtype == PA_BF16 ? 2 : 4)) % 16 != 0) return PA_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PA_BF16) return attention_probs_t<bf16>(qkv, ldqkv, lse, out, cu_tok, out_off, B, H, N, nq, head_mean, scale, flags, st);
    return attention_probs_t<float>(qkv, ldqkv, lse, out, cu_tok, out_off, B, H, N, nq, head_mean, scale, flags, st);
}

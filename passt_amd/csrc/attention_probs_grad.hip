// Gradient of the loss with respect to the attention probabilities, written out, for gfx950: what retain_grad() on the input of
// the reference's blocks[i].attn.attn_drop holds after the backward (models/passt.py:348-352).  The fused backward (attention.hip)
// forms dP = dO V^T tile by tile in registers and never lets it reach memory; here a (32 queries x 32 keys) tile of it is
//   g[q][k] = sum_d d_o[q][h*64 + d] * v[k][h*64 + d]
// and stands alone exactly as a tile of the probabilities does (attention_probs.hip): no LDS, no barrier, no atomics.
//
// Same decomposition and orientation as attn_probs_kernel: one wave = one 32 x 32 tile of one (sequence, head), A operand = the
// d_o rows (queries), B operand = the V rows (keys), so 32 consecutive KEYS sit in 32 consecutive lanes and every accumulator
// register is stored as two 128-byte pieces of two output rows.
//   GRAD: out = g.
//   CAM:  out = max(p * g, 0) with p formed exactly as attn_probs_kernel forms it (same PRE handling, hi + lo lse * log2 e, key
//         lanes at or behind N masked before the exponential, the four short f32 chains); with head_mean the wave loops the heads
//         in order and adds max(p * g, 0) in f32 registers: 1 / H of the bytes, and neither full map is ever read back.
// In the source the d_o / V fragments of a head are loaded after its probabilities are final (the Q / K fragments and the score
// chains are dead by then); the compiler hoists those loads, so the CAM instances hold both sets: 137 / 144 VGPRs (bf16, q
// pre-scaled / not) and 218 / 220 (f32) against 116 for the bf16 attn_probs_kernel, GRAD 48 / 92; no scratch, no AGPRs in any
// instance.  The f32 CAM instances therefore run at 2 waves per SIMD (bf16: 3): accepted for a diagnostics path that is bound by
// its output bytes in the per-head modes.
// Rows are clamped to the sequence's own last query / key row, so the packed form reads no row of a neighbour and none behind
// cu_tok[B]; key lanes at or behind N are never stored.
//
// KEEP IN STEP: attn_rollout_kernel (attention_rollout.hip) forms its tiles with a copy of this kernel's
// arithmetic, operation for operation, and their tests rest on that: change it in all three files or in none.
#include "pa_mma.h"

namespace pa {

static constexpr int G_HD = 64;                                  // head dim
static constexpr double G_LOG2E_D = 1.4426950408889634;
static constexpr float G_LOG2E = (float)G_LOG2E_D, G_LOG2E_LO = (float)(G_LOG2E_D - (double)G_LOG2E);      // log2 e = hi + lo
static constexpr int G_KT = 128, G_QT = 32;                       // keys / queries per workgroup (4 waves x 32 keys)

// Work item -> (key tile, query tile, sequence x output head), key tile fastest, as in attn_probs_kernel.  VL: sequences packed
// back to back (cu_tok), N / nq hold max N and the caller's nq.  d_o: row (tok0 + q) of the token matrix, or with `compact` row
// (b * nq + q) of the prefix form (nq = the caller's).
template <typename T, bool PRE, bool VL, bool CAM>
__global__ __launch_bounds__(256) void attn_probs_grad_kernel(const T* __restrict__ qkv, int ldqkv, const float* __restrict__ lse,
                                                              const T* __restrict__ d_o, int ldo, int compact,
                                                              float* __restrict__ out, const int32_t* __restrict__ cu_tok,
                                                              const int64_t* __restrict__ out_off, int B, int H, int N, int nq,
                                                              int nkt, int nqt, int head_mean, float scale) {
    using F = typename Frag<T>::type;
    constexpr int NF = G_HD * (int)sizeof(T) / 32;                // 16-byte fragments per lane and row: 4 (bf16) / 8 (f32)
    constexpr int EPC = 16 / (int)sizeof(T);
    constexpr int NC = sizeof(T) == 4 ? 4 : 1;                    // accumulation chains per product (see attn_probs_kernel)
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
    const int64_t do0 = compact ? (int64_t)b * nq : -1;          // first row of this sequence in the compact d_o
    const float* lse_b = CAM ? lse + (int64_t)b * H * nq : nullptr;      // lse of (head 0, query 0) of this sequence
    int64_t lse_pitch = nq;                                      // floats between two heads
    float* out_b = out;
    if constexpr (VL) {
        const int t0 = cu_tok[b], t1 = cu_tok[b + 1];            // wave-uniform: scalar loads
        const bool all_queries = nq >= N;                        // N is max N here
        N = t1 - t0;
        tok0 = t0;
        if (CAM && all_queries) {
            lse_pitch = cu_tok[B];
            lse_b = lse + t0;
        }
        nq = min(nq, N);
        out_b = out + out_off[b];
    } else {
        out_b = out + (int64_t)b * Ho * nq * N;
    }
    const int q0 = qt * G_QT, k0 = kt * G_KT + wave * 32;
    if (q0 >= nq || k0 >= N) return;                             // (also N <= 0) wave-uniform; the kernel has no barrier

    const int r32 = lane & 31, half = lane >> 5;
    const int qrow = min(q0 + r32, nq - 1), krow = min(k0 + r32, N - 1);
    const bool klive = k0 + r32 < N;
    const double sl2d = (double)scale * G_LOG2E_D;                // scale * log2 e as hi + lo floats (used when q is not pre-scaled)
    const float sl2 = (float)sl2d, sl2_lo = (float)(sl2d - (double)sl2);
    const int D = H * G_HD;
    const T* do_row = d_o + (compact ? do0 + qrow : tok0 + qrow) * (int64_t)ldo;      // this lane's d_o row, head 0
    int qr[16];                                                  // the (clamped) query row of every accumulator register
    if constexpr (CAM) {
#pragma unroll
        for (int i = 0; i < 16; ++i) qr[i] = min(q0 + acc_row(i, lane), nq - 1);
    }

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int hh = 0; hh < nh; ++hh) {
        const int h = h0 + hh;
        const T* base = qkv + tok0 * ldqkv + h * G_HD;           // q of token 0 of this (sequence, head)
        f32x16 p;
        if constexpr (CAM) {
            // the probabilities of this tile, operation for operation those of attn_probs_kernel
            const float* lse_h = lse_b + (int64_t)h * lse_pitch;
            F qf[NF], kf[NF];
#pragma unroll
            for (int s = 0; s < NF; ++s) {
                const int off = (s * 2 + half) * EPC;
                qf[s] = *(const F*)(base + (int64_t)qrow * ldqkv + off);
                kf[s] = *(const F*)(base + D + (int64_t)krow * ldqkv + off);
            }
            f32x16 c, cl;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float nl = -lse_h[qr[i]];
                c[i] = nl * G_LOG2E;
                cl[i] = fmaf(nl, G_LOG2E, -c[i]) + nl * G_LOG2E_LO;
            }
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
                float a = PRE ? (s + c[i]) + cl[i] : fmaf(s, sl2, c[i]) + fmaf(s, sl2_lo, cl[i]);
                a = klive ? a : -INFINITY;
                p[i] = __builtin_amdgcn_exp2f(a);
            }
        }
        // g = d_o v^T of this head, the same chains
        F df[NF], vf[NF];
#pragma unroll
        for (int s = 0; s < NF; ++s) {
            const int off = (s * 2 + half) * EPC;
            df[s] = *(const F*)(do_row + h * G_HD + off);
            vf[s] = *(const F*)(base + 2 * D + (int64_t)krow * ldqkv + off);
        }
        f32x16 gc[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            mma32_first<T>(gc[j], df[j * (NF / NC)], vf[j * (NF / NC)]);
#pragma unroll
            for (int st = 1; st < NF / NC; ++st) mma32<T>(gc[j], df[j * (NF / NC) + st], vf[j * (NF / NC) + st]);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float g = gc[0][i];
            if constexpr (NC == 4) g = (gc[0][i] + gc[1][i]) + (gc[2][i] + gc[3][i]);
            if constexpr (CAM) acc[i] += fmaxf(p[i] * g, 0.f);
            else acc[i] = g;
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
static int attention_probs_grad_t(const void* qkv, int ldqkv, const float* lse, const void* d_o, int ldo, int compact, float* out,
                                  const int32_t* cu_tok, const int64_t* out_off, int B, int H, int N, int nq, int head_mean, int mode,
                                  float scale, int flags, hipStream_t st) {
    const int nqk = nq >= N ? N : nq;
    const int nkt = (int)cdiv(N, G_KT), nqt = (int)cdiv(nqk, G_QT);
    const int64_t items = (int64_t)nkt * nqt * B * (head_mean ? 1 : H);
    if (items >= (int64_t)1 << 31) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)items), block(256);
    const bool pre = flags & PA_ATTN_Q_PRESCALED;
#define PA_PGRAD_LAUNCH(PRE_, VL_, CAM_)                                                                                          \
    hipLaunchKernelGGL((attn_probs_grad_kernel<T, PRE_, VL_, CAM_>), grid, block, 0, st, (const T*)qkv, ldqkv, lse, (const T*)d_o, \
                       ldo, compact, out, cu_tok, out_off, B, H, N, nqk, nkt, nqt, head_mean, scale)
    if (mode == PA_ATTN_PGRAD_GRAD) {                             // no probability is formed: one instance per layout
        if (cu_tok) PA_PGRAD_LAUNCH(false, true, false);
        else PA_PGRAD_LAUNCH(false, false, false);
    } else if (cu_tok) {
        if (pre) PA_PGRAD_LAUNCH(true, true, true);
        else PA_PGRAD_LAUNCH(false, true, true);
    } else {
        if (pre) PA_PGRAD_LAUNCH(true, false, true);
        else PA_PGRAD_LAUNCH(false, false, true);
    }
#undef PA_PGRAD_LAUNCH
    return check_launch();
}

}  // namespace pa

using namespace pa;

extern "C" int pa_attention_probs_grad(const void* qkv, int ldqkv, const float* lse, const void* d_o, int ldo, int do_compact, float* out,
                                       const int32_t* cu_tok, const int64_t* out_off, int B, int H, int N, int nq, int head_mean,
                                       int mode, float scale, int dtype, int flags, void* stream) {
    if (!qkv || !d_o || !out || B <= 0 || H <= 0 || N <= 0 || nq <= 0 || (flags & ~PA_ATTN_Q_PRESCALED) || (head_mean & ~1) ||
        (do_compact & ~1))
        return PA_EINVAL;
    if (mode != PA_ATTN_PGRAD_GRAD && mode != PA_ATTN_PGRAD_CAM) return PA_EINVAL;
    if (mode == PA_ATTN_PGRAD_GRAD ? head_mean != 0 : !lse) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    if (cu_tok ? !out_off : (out_off != nullptr || nq > N)) return PA_EINVAL;      // the offsets belong to the packed layout
    if (ldqkv < 3 * H * G_HD || ldo < H * G_HD) return PA_EINVAL;
    const int es = dtype == PA_BF16 ? 2 : 4;
    if ((ldqkv * es) % 16 != 0 || (ldo * es) % 16 != 0) return PA_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PA_BF16)
        return attention_probs_grad_t<bf16>(qkv, ldqkv, lse, d_o, ldo, do_compact, out, cu_tok, out_off, B, H, N, nq, head_mean, mode,
                                            scale, flags, st);
    return attention_probs_grad_t<float>(qkv, ldqkv, lse, d_o, ldo, do_compact, out, cu_tok, out_off, B, H, N, nq, head_mean, mode, scale,
                                         flags, st);
}

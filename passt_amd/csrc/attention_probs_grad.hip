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
//   CAM:  out = max(p * g, 0) with p the probability tile of pa_attn_tile.h -- the header attn_probs_kernel and the rollout take it
//         from, which also holds the chained product that forms g; with head_mean the wave loops the heads in order and adds
//         max(p * g, 0) in f32 registers: 1 / H of the bytes, and neither full map is ever read back.
// In the source the d_o / V fragments of a head are loaded after its probabilities are final (the Q / K fragments and the score
// chains are dead by then); the compiler hoists those loads, so the CAM instances hold both sets: 137 / 144 VGPRs (bf16, q
// pre-scaled / not) and 218 / 220 (f32; 224 in the fixed layout with q not pre-scaled) against 108 / 123 for the bf16
// attn_probs_kernel, GRAD 48 / 92; no scratch, no AGPRs in any instance.  The f32 CAM instances therefore run at 2 waves per SIMD
// (bf16: 3): accepted for a diagnostics path that is bound by its output bytes in the per-head modes.
// Rows are clamped to the sequence's own last query / key row, so the packed form reads no row of a neighbour and none behind
// cu_tok[B]; key lanes at or behind N are never stored.
#include "pa_attn_tile.h"

namespace pa {

// Work item -> (key tile, query tile, sequence x output head), key tile fastest, as in attn_probs_kernel.  VL: sequences packed
// back to back (cu_tok), N / nq hold max N and the caller's nq.  d_o: row (tok0 + q) of the token matrix, or with `compact` row
// (b * nq + q) of the prefix form (nq = the caller's).  GRAD never touches lse (it may be null).
template <typename T, bool PRE, bool VL, bool CAM>
__global__ __launch_bounds__(256) void attn_probs_grad_kernel(const T* __restrict__ qkv, int ldqkv, const float* __restrict__ lse,
                                                              const T* __restrict__ d_o, int ldo, int compact,
                                                              float* __restrict__ out, const int32_t* __restrict__ cu_tok,
                                                              const int64_t* __restrict__ out_off, int B, int H, int N, int nq,
                                                              int nkt, int nqt, int head_mean, float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int L = blockIdx.x;
    const int kt = L % nkt;
    L /= nkt;
    const int qt = L % nqt;
    const int z = L / nqt;
    const int Ho = head_mean ? 1 : H, nh = head_mean ? H : 1;
    const int b = z / Ho, h0 = z - b * Ho;

    const SeqGeom sg = seq_geom<VL, CAM>(b, B, H, N, nq, cu_tok, lse, compact);
    N = sg.N;
    nq = sg.nq;
    float* out_b = VL ? out + out_off[b] : out + (int64_t)b * Ho * nq * N;
    const int q0 = qt * AT_QT, k0 = kt * AT_KT + wave * 32;
    if (q0 >= nq || k0 >= N) return;                             // (also N <= 0) wave-uniform; the kernel has no barrier

    const int r32 = lane & 31, half = lane >> 5;
    const int qrow = min(q0 + r32, nq - 1), krow = min(k0 + r32, N - 1);
    const bool klive = k0 + r32 < N;
    float sl2, sl2_lo;
    scale_log2e(scale, sl2, sl2_lo);
    const int D = H * AT_HD;
    const T* do_row = d_o + (sg.do0 + qrow) * (int64_t)ldo;      // this lane's d_o row, head 0
    int qr[16];
    if constexpr (CAM) tile_query_rows(qr, q0, nq, lane);

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int hh = 0; hh < nh; ++hh) {
        const int h = h0 + hh;
        const T* base = qkv + sg.tok0 * ldqkv + h * AT_HD;        // q of token 0 of this (sequence, head)
        f32x16 p, g;
        if constexpr (CAM)
            tile_probs<T, PRE>(p, base + (int64_t)qrow * ldqkv, base + D + (int64_t)krow * ldqkv, sg.lse_b + (int64_t)h * sg.lse_pitch,
                               qr, klive, sl2, sl2_lo, half);
        tile_grad<T>(g, do_row + h * AT_HD, base + 2 * D + (int64_t)krow * ldqkv, half);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if constexpr (CAM) acc[i] += fmaxf(p[i] * g[i], 0.f);
            else acc[i] = g[i];
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
    const int nkt = (int)cdiv(N, AT_KT), nqt = (int)cdiv(nqk, AT_QT);
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
    if (ldqkv < 3 * H * AT_HD || ldo < H * AT_HD) return PA_EINVAL;
    const int es = dtype == PA_BF16 ? 2 : 4;
    if ((ldqkv * es) % 16 != 0 || (ldo * es) % 16 != 0) return PA_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PA_BF16)
        return attention_probs_grad_t<bf16>(qkv, ldqkv, lse, d_o, ldo, do_compact, out, cu_tok, out_off, B, H, N, nq, head_mean, mode,
                                            scale, flags, st);
    return attention_probs_grad_t<float>(qkv, ldqkv, lse, d_o, ldo, do_compact, out, cu_tok, out_off, B, H, N, nq, head_mean, mode, scale,
                                         flags, st);
}

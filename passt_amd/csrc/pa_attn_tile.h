// The (32 queries x 32 keys) attention tile behind the maps (attention_probs.hip), their gradients / CAM (attention_probs_grad.hip)
// and the rollout (attention_rollout.hip), for gfx950: ONE copy of the arithmetic.  The three kernels differ in what they do with
// a finished tile (store it, weight and store it, multiply it by row vectors and sum); that they form it from the same operations
// in the same order is what tests/test_gpu_rollout.py's identity test pins bit for bit, and what the rollout's bound rests on.
//
// The fused forward (attention.hip) leaves lse = log sum_k exp(score) per query row next to qkv, so a probability is
//   p[q][k] = exp2(s~[q][k] - lse[q] * log2 e),   s~ = q k^T * scale * log2 e
// and any tile stands alone.  One wave forms one tile in the orientation S[q][key] (A operand = query rows, B operand = key rows):
// 32 consecutive KEYS in 32 consecutive lanes (col = lane & 31), a query row per accumulator register (acc_row).  The fragments
// come from global memory directly (each is used by one product).  Everything here is __forceinline__ and works on registers.
#pragma once
#include "pa_mma.h"

namespace pa {

static constexpr int AT_HD = 64;                                  // head dim
static constexpr double AT_LOG2E_D = 1.4426950408889634;
static constexpr float AT_LOG2E = (float)AT_LOG2E_D, AT_LOG2E_LO = (float)(AT_LOG2E_D - (double)AT_LOG2E);      // log2 e = hi + lo
static constexpr int AT_KT = 128, AT_QT = 32;                     // keys per workgroup (4 waves x 32 keys) / queries per tile

template <typename T>
struct AttnTile {
    using F = typename Frag<T>::type;
    static constexpr int NF = AT_HD * (int)sizeof(T) / 32;        // 16-byte fragments per lane and row: 4 (bf16) / 8 (f32)
    static constexpr int EPC = 16 / (int)sizeof(T);               // elements per fragment
    // accumulation chains per product.  A chain's rounding errors are half ulps of its own partial sums, so four short f32 chains
    // added pairwise leave well under half the error of one chain of 32 MFMAs; the bf16 product is one chain of 4
    static constexpr int NC = sizeof(T) == 4 ? 4 : 1;
};

// Where sequence b lives.  Fixed layout: B sequences of N tokens, lse [(b * H + h) * nq + q].  VL: sequences packed back to back
// (cu_tok: B + 1 token offsets), N / nq come in as max N and the caller's nq and go out as the sequence's own; lse is [H][total]
// when every query was asked for (nq >= max N) and compact as in the fixed layout otherwise.  LSE = false leaves lse alone (it may
// be null: the plain gradient forms no probability, the rollout's finishing kernel no tile).
struct SeqGeom {
    int64_t tok0;              // first token row of the sequence in qkv
    int N, nq;                 // its tokens, its query rows
    int64_t do0;               // its first row in d_o: tok0, or b * (the caller's nq) in the compact form
    const float* lse_b;        // lse of its (head 0, query 0)
    int64_t lse_pitch;         // floats between two heads
};
template <bool VL, bool LSE = true>
__device__ __forceinline__ SeqGeom seq_geom(int b, int B, int H, int N, int nq, const int32_t* __restrict__ cu_tok,
                                            const float* __restrict__ lse, int compact) {
    SeqGeom g;
    g.tok0 = (int64_t)b * N;
    g.do0 = compact ? (int64_t)b * nq : g.tok0;
    g.lse_b = LSE ? lse + (int64_t)b * H * nq : nullptr;
    g.lse_pitch = nq;
    if constexpr (VL) {
        const int t0 = cu_tok[b], t1 = cu_tok[b + 1];            // wave-uniform: scalar loads
        if (LSE && nq >= N) {                                    // every query (N is max N here)
            g.lse_pitch = cu_tok[B];
            g.lse_b = lse + t0;
        }
        N = t1 - t0;
        g.tok0 = t0;
        if (!compact) g.do0 = t0;
        nq = min(nq, N);
    }
    g.N = N;
    g.nq = nq;
    return g;
}

// scale * log2 e as hi + lo floats (used when q is not pre-scaled)
__device__ __forceinline__ void scale_log2e(float scale, float& sl2, float& sl2_lo) {
    const double sl2d = (double)scale * AT_LOG2E_D;
    sl2 = (float)sl2d;
    sl2_lo = (float)(sl2d - (double)sl2);
}

// the query row of every accumulator register of the tile at q0, clamped to the sequence's last query row: loads through it stay
// in bounds (the packed form reads no row of a neighbour), and who stores or sums a row checks q0 + acc_row(i, lane) < nq itself
__device__ __forceinline__ void tile_query_rows(int (&qr)[16], int q0, int nq, int lane) {
#pragma unroll
    for (int i = 0; i < 16; ++i) qr[i] = min(q0 + acc_row(i, lane), nq - 1);
}

// the NF fragments this lane half holds of one 64-element row (rows are 16-byte aligned: the entries check the leading dimensions)
template <typename T>
__device__ __forceinline__ void tile_load(typename AttnTile<T>::F (&f)[AttnTile<T>::NF], const T* __restrict__ row, int half) {
    using F = typename AttnTile<T>::F;
#pragma unroll
    for (int s = 0; s < AttnTile<T>::NF; ++s) f[s] = *(const F*)(row + (s * 2 + half) * AttnTile<T>::EPC);
}

// out = a b^T over the head dim: NC independent chains, summed as (c0 + c1) + (c2 + c3).  The score q k^T and the gradient d_o v^T
template <typename T>
__device__ __forceinline__ void tile_product(f32x16& out, const typename AttnTile<T>::F (&a)[AttnTile<T>::NF],
                                             const typename AttnTile<T>::F (&b)[AttnTile<T>::NF]) {
    constexpr int NF = AttnTile<T>::NF, NC = AttnTile<T>::NC;
    f32x16 ch[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        mma32_first<T>(ch[j], a[j * (NF / NC)], b[j * (NF / NC)]);
#pragma unroll
        for (int st = 1; st < NF / NC; ++st) mma32<T>(ch[j], a[j * (NF / NC) + st], b[j * (NF / NC) + st]);
    }
    if constexpr (NC == 4) {
#pragma unroll
        for (int i = 0; i < 16; ++i) out[i] = (ch[0][i] + ch[1][i]) + (ch[2][i] + ch[3][i]);
    } else {
        out = ch[0];
    }
}

// g = d_o v^T of one head: this lane's d_o and V rows (at the head's first element)
template <typename T>
__device__ __forceinline__ void tile_grad(f32x16& g, const T* __restrict__ do_row, const T* __restrict__ v_row, int half) {
    typename AttnTile<T>::F df[AttnTile<T>::NF], vf[AttnTile<T>::NF];
    tile_load<T>(df, do_row, half);
    tile_load<T>(vf, v_row, half);
    tile_product<T>(g, df, vf);
}

// p = the probabilities of one head's tile.  q_row / k_row: this lane's Q and K rows (at the head's first element), lse_h: the
// head's lse, qr: tile_query_rows, klive: this lane's key is in front of N.  PRE: q already holds q * scale * log2 e.
// The exponent s~ - lse * log2 e is formed so that the kernel's own error stays at a few f32 ulps of the score.
template <typename T, bool PRE>
__device__ __forceinline__ void tile_probs(f32x16& p, const T* __restrict__ q_row, const T* __restrict__ k_row,
                                           const float* __restrict__ lse_h, const int (&qr)[16], bool klive, float sl2, float sl2_lo,
                                           int half) {
    typename AttnTile<T>::F qf[AttnTile<T>::NF], kf[AttnTile<T>::NF];
    tile_load<T>(qf, q_row, half);
    tile_load<T>(kf, k_row, half);
    // -lse * log2 e as an unevaluated sum c + cl: |lse| of ~100 leaves a float product half an ulp of ~1e-5 off, which would be
    // the relative error of every probability of the row
    f32x16 c, cl;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float nl = -lse_h[qr[i]];
        c[i] = nl * AT_LOG2E;
        cl[i] = fmaf(nl, AT_LOG2E, -c[i]) + nl * AT_LOG2E_LO;
    }
    f32x16 s;
    tile_product<T>(s, qf, kf);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        // s~ - lse * log2 e: the large parts cancel in one fma, the low parts follow
        float a = PRE ? (s[i] + c[i]) + cl[i] : fmaf(s[i], sl2, c[i]) + fmaf(s[i], sl2_lo, cl[i]);
        // key lanes at or behind N go to -inf BEFORE the exponential: exp2(0 - lse * log2 e) overflows for strongly negative scores
        a = klive ? a : -INFINITY;
        p[i] = __builtin_amdgcn_exp2f(a);
    }
}

}  // namespace pa

// One step of an attention rollout on a few row vectors, for gfx950: r_out = a * r_in + b_ * (r_in[:, :nq] @ M) with M the head mean of
// a block's attention probabilities (ATTN) or of relu(probabilities * their gradient) (CAM) -- and M never exists.  A row of a product
// of matrices needs no matrix: e_cls^T M_{L-1} ... M_0 is a chain of row-vector x matrix products from the last block down, and each
// r M is formed tile by tile from what the fused attention left (qkv, lse, and d_o for CAM), exactly as attention_probs.hip and
// attention_probs_grad.hip form their tiles; where those store a (32 queries x 32 keys) tile, this kernel multiplies it by r's 32
// entries and sums over the queries.  What reaches memory is nr * N floats per sequence instead of N * N.
//
// Decomposition.  One wave owns 32 consecutive KEYS (col = lane & 31, as in the sibling kernels) and walks a SLICE of the query tiles;
// per tile the head loop adds the H tiles in head order in f32 registers (what the head_mean instances of the sibling kernels add:
// all three take the probability tile and the chained product from pa_attn_tile.h), then for every row vector j
//   t = sum over the 16 accumulator registers of acc[i] * r[j][row(i)]      (one fma chain, register order)
//   t += the other lane half's t                                              (rows 4..7, 12..15, ... live there)
//   part[j] += t                                                              (tiles of the slice in ascending order)
// Rows at or behind nq contribute exactly nothing: the tile itself is formed from rows clamped to nq - 1 (harmless for a store, here
// the last row would be added several times), so r is MASKED to 0 there and the clamp only keeps the loads in bounds.  Key lanes at
// or behind N hold 0 and are never stored.
// A wave per 32 keys alone would be B * ceil(N / 32) waves (38 at B = 1, 1190 tokens), so the queries are cut into S slices of `tps`
// tiles (host: rollout_slices below); slice s of a sequence writes its partial rows to ws[s] and attn_rollout_finish_kernel adds
// them in slice order and applies a, b_ and 1 / H.  S = 1 (always so for nq = 2) finishes in the same kernel and needs no workspace.
// No atomics, no LDS, no barrier: two launches on the same inputs give the same bits, and the result depends on (tps, inputs) only --
// a packed sequence gets what the fixed form gives it alone with the same tps.
//
// Registers (-O3, -amdgpu-mfma-vgpr-form; VGPRs with q pre-scaled / not), fixed layout | packed layout:
//   ATTN  bf16 187 / 205 | 175 / 193     f32 244 / 246 | 232 / 234
//   CAM   bf16 230 / 232 | 218 / 220     f32 236 / 238 | 254 / 256
// no scratch and no AGPRs in any instance; every instance runs at 2 waves per SIMD (the finishing kernel: 10 VGPRs, 8 waves).  The
// sibling kernels need 108 (bf16 probabilities) to 224 (f32 CAM): with a loop over the query tiles around the head loop the
// scheduler hoists the next tile's loads and addresses as far as __launch_bounds__(256) lets it.  Holding the bf16 instances to 3
// waves (amdgpu_waves_per_eu) brings them to 164 - 168 VGPRs but spills 12 - 76 bytes per lane in three of the CAM ones, so the
// bound is left alone: no scratch comes first.  r is loaded behind the head loop, when the fragments and score chains of the tile
// are dead.
#include "pa_attn_tile.h"

namespace pa {

static constexpr int R_MAX_NR = PA_ATTN_ROLLOUT_MAX_ROWS;

// Work item -> (key tile, slice, sequence), key tile fastest.  VL: sequences packed back to back (cu_tok), N / nq hold max N and the
// caller's nq, r / out / ws hold sequence b's (nr, N_b) block at float offset nr * cu_tok[b].  `direct` (S == 1): out is r_out and
// gets a * r_in + b_ * sum / H; otherwise out is the workspace and gets the slice's raw sums at slice pitch `ws_pitch`.
template <typename T, bool PRE, bool VL, bool CAM>
__global__ __launch_bounds__(256) void attn_rollout_kernel(const T* __restrict__ qkv, int ldqkv, const float* __restrict__ lse,
                                                           const T* __restrict__ d_o, int ldo, int compact,
                                                           const float* __restrict__ r_in, float* __restrict__ out,
                                                           const int32_t* __restrict__ cu_tok, int B, int H, int N, int nq, int nr,
                                                           int nkt, int S, int tps, int direct, int64_t ws_pitch, float a, float b_,
                                                           float g_scale, float scale) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int L = blockIdx.x;
    const int kt = L % nkt;
    L /= nkt;
    const int s = L % S;
    const int b = L / S;

    const SeqGeom sg = seq_geom<VL>(b, B, H, N, nq, cu_tok, lse, compact);
    N = sg.N;
    nq = sg.nq;
    const int64_t roff = (int64_t)nr * sg.tok0;                  // this sequence's (nr, N) block in r_in / r_out / a workspace slice
    const int k0 = kt * AT_KT + wave * 32;
    const int t_begin = s * tps, t_end = min(t_begin + tps, (int)cdiv(nq, AT_QT));
    if (t_begin >= t_end || k0 >= N) return;                     // (also N <= 0) wave-uniform; the kernel has no barrier

    const int r32 = lane & 31, half = lane >> 5;
    const int krow = min(k0 + r32, N - 1);
    const bool klive = k0 + r32 < N;
    float sl2, sl2_lo;
    scale_log2e(scale, sl2, sl2_lo);
    const int D = H * AT_HD;

    float part[R_MAX_NR];
#pragma unroll
    for (int j = 0; j < R_MAX_NR; ++j) part[j] = 0.f;

    for (int qt = t_begin; qt < t_end; ++qt) {
        const int q0 = qt * AT_QT;
        const int qrow = min(q0 + r32, nq - 1);
        int qr[16];
        tile_query_rows(qr, q0, nq, lane);

        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int h = 0; h < H; ++h) {
            const T* base = qkv + sg.tok0 * ldqkv + h * AT_HD;    // q of token 0 of this (sequence, head)
            f32x16 p;
            tile_probs<T, PRE>(p, base + (int64_t)qrow * ldqkv, base + D + (int64_t)krow * ldqkv, sg.lse_b + (int64_t)h * sg.lse_pitch,
                               qr, klive, sl2, sl2_lo, half);
            if constexpr (CAM) {
                f32x16 g;
                tile_grad<T>(g, d_o + (sg.do0 + qrow) * (int64_t)ldo + h * AT_HD, base + 2 * D + (int64_t)krow * ldqkv, half);
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] += fmaxf(p[i] * (g[i] * g_scale), 0.f);
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] += p[i];
            }
        }
        // the reduction over this tile's queries.  r is read at the clamped row and masked: a row at or behind nq adds exactly 0
#pragma unroll
        for (int j = 0; j < R_MAX_NR; ++j) {
            if (j < nr) {                                        // wave-uniform
                const float* rj = r_in + roff + (int64_t)j * N;
                float t = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float rv = acc_row(i, lane) < nq - q0 ? rj[qr[i]] : 0.f;
                    t = fmaf(acc[i], rv, t);
                }
                t += __shfl_xor(t, 32, 64);
                part[j] += t;
            }
        }
    }
    if (!klive || half) return;                                  // lanes 0..31 hold the sums of the 32 keys
    const float mul = 1.0f / (float)H;
    const int k = k0 + r32;
#pragma unroll
    for (int j = 0; j < R_MAX_NR; ++j) {
        if (j < nr) {
            const int64_t e = roff + (int64_t)j * N + k;
            if (direct) out[e] = fmaf(b_, part[j] * mul, a * r_in[e]);
            else out[(int64_t)s * ws_pitch + e] = part[j];
        }
    }
}

// r_out = a * r_in + b_ * (sum over the sequence's slices, in slice order) / H.  One thread per (key, row vector, sequence).
template <bool VL>
__global__ __launch_bounds__(256) void attn_rollout_finish_kernel(const float* __restrict__ ws, const float* __restrict__ r_in,
                                                                  float* __restrict__ r_out, const int32_t* __restrict__ cu_tok,
                                                                  int H, int N, int nq, int nr, int tps, int64_t ws_pitch, float a,
                                                                  float b_) {
    const int b = blockIdx.z, j = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const SeqGeom sg = seq_geom<VL, false>(b, 0, H, N, nq, cu_tok, nullptr, 0);
    N = sg.N;
    nq = sg.nq;
    if (k >= N) return;
    const int Sb = (int)cdiv(cdiv(nq, AT_QT), tps);               // the slices this sequence has
    const int64_t e = (int64_t)nr * sg.tok0 + (int64_t)j * N + k;
    float sum = ws[e];
    for (int s = 1; s < Sb; ++s) sum += ws[(int64_t)s * ws_pitch + e];
    r_out[e] = fmaf(b_, sum * (1.0f / (float)H), a * r_in[e]);
}

// CU count of the device this thread launches on (asked of the runtime every time: a host-side attribute read, and a process may
// drive devices of different sizes); 256 where no device answers (the workspace query on a host without one).
static int current_device_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        n = 256;
    }
    return n;
}

// Slices of the query tiles: 8 waves per CU = 2 waves per SIMD, what these instances run at, so one resident round of the device;
// never more slices than tiles, the tiles spread evenly.  Returns S, *tps = query tiles per slice.
static int rollout_slices(int B, int N, int nqk, int slices, int* tps) {
    const int cus = slices > 0 ? 0 : current_device_cus();
    const int64_t nqt = cdiv(nqk, AT_QT);
    int64_t S = slices;
    if (S <= 0) S = ((int64_t)cus * 8) / ((int64_t)B * cdiv(N, 32));
    S = S < 1 ? 1 : (S > nqt ? nqt : S);
    *tps = (int)cdiv(nqt, S);
    return (int)cdiv(nqt, *tps);
}

template <typename T>
static int attention_rollout_t(const void* qkv, int ldqkv, const float* lse, const void* d_o, int ldo, int compact, const float* r_in,
                               float* r_out, float* ws, const int32_t* cu_tok, int64_t total_tok, int B, int H, int N, int nq, int nr,
                               int mode, int slices, float a, float b_, float g_scale, float scale, int flags, hipStream_t st) {
    const int nqk = nq >= N ? N : nq;
    int tps = 1;
    const int S = rollout_slices(B, N, nqk, slices, &tps);
    if (S > 1 && !ws) return PA_EINVAL;
    const int nkt = (int)cdiv(N, AT_KT);
    const int64_t items = (int64_t)nkt * S * B;
    if (items >= (int64_t)1 << 31 || B > 65535) return PA_EUNSUPPORTED;
    const dim3 grid((unsigned)items), block(256);
    const bool pre = flags & PA_ATTN_Q_PRESCALED;
    const int direct = S == 1;
    const int64_t ws_pitch = (int64_t)nr * total_tok;
    float* out = direct ? r_out : ws;
#define PA_ROLL_LAUNCH(PRE_, VL_, CAM_)                                                                                           \
    hipLaunchKernelGGL((attn_rollout_kernel<T, PRE_, VL_, CAM_>), grid, block, 0, st, (const T*)qkv, ldqkv, lse, (const T*)d_o, ldo, \
                       compact, r_in, out, cu_tok, B, H, N, nqk, nr, nkt, S, tps, direct, ws_pitch, a, b_, g_scale, scale)
#define PA_ROLL_LAUNCH_PV(CAM_)                          \
    if (cu_tok) {                                        \
        if (pre) PA_ROLL_LAUNCH(true, true, CAM_);       \
        else PA_ROLL_LAUNCH(false, true, CAM_);          \
    } else {                                             \
        if (pre) PA_ROLL_LAUNCH(true, false, CAM_);      \
        else PA_ROLL_LAUNCH(false, false, CAM_);         \
    }
    if (mode == PA_ATTN_ROLLOUT_CAM) {
        PA_ROLL_LAUNCH_PV(true)
    } else {
        PA_ROLL_LAUNCH_PV(false)
    }
#undef PA_ROLL_LAUNCH_PV
#undef PA_ROLL_LAUNCH
    int rc = check_launch();
    if (rc != PA_OK || direct) return rc;
    const dim3 fgrid((unsigned)cdiv(N, 256), (unsigned)nr, (unsigned)B);
    if (cu_tok)
        hipLaunchKernelGGL((attn_rollout_finish_kernel<true>), fgrid, block, 0, st, ws, r_in, r_out, cu_tok, H, N, nqk, nr, tps, ws_pitch, a,
                           b_);
    else
        hipLaunchKernelGGL((attn_rollout_finish_kernel<false>), fgrid, block, 0, st, ws, r_in, r_out, cu_tok, H, N, nqk, nr, tps, ws_pitch,
                           a, b_);
    return check_launch();
}

}  // namespace pa

using namespace pa;

extern "C" int64_t pa_attention_rollout_ws_floats(int64_t total_tok, int B, int N, int nq, int nr, int slices) {
    if (total_tok <= 0 || B <= 0 || N <= 0 || nq <= 0 || nr < 1 || nr > R_MAX_NR || slices < 0 || total_tok < N) return PA_EINVAL;
    int tps = 1;
    const int S = rollout_slices(B, N, nq >= N ? N : nq, slices, &tps);
    return S > 1 ? (int64_t)S * nr * total_tok : 0;
}

extern "C" int pa_attention_rollout(const void* qkv, int ldqkv, const float* lse, const void* d_o, int ldo, int do_compact,
                                    const float* r_in, float* r_out, float* ws, const int32_t* cu_tok, int64_t total_tok, int B, int H,
                                    int N, int nq, int nr, int mode, int slices, float a, float b_, float g_scale, float scale, int dtype,
                                    int flags, void* stream) {
    if (!qkv || !lse || !r_in || !r_out || B <= 0 || H <= 0 || N <= 0 || nq <= 0 || (flags & ~PA_ATTN_Q_PRESCALED) || (do_compact & ~1) ||
        slices < 0)
        return PA_EINVAL;
    if (nr < 1 || nr > R_MAX_NR || total_tok <= 0) return PA_EINVAL;
    if (r_out < r_in + (int64_t)nr * total_tok && r_in < r_out + (int64_t)nr * total_tok) return PA_EINVAL;      // they share a float
    if (mode != PA_ATTN_ROLLOUT_ATTN && mode != PA_ATTN_ROLLOUT_CAM) return PA_EINVAL;
    if (mode == PA_ATTN_ROLLOUT_CAM ? !d_o : (d_o != nullptr || do_compact)) return PA_EINVAL;
    if (dtype != PA_BF16 && dtype != PA_F32) return PA_EINVAL;
    if (cu_tok ? total_tok < N : (nq > N || total_tok != (int64_t)B * N)) return PA_EINVAL;
    if (ldqkv < 3 * H * AT_HD || (d_o && ldo < H * AT_HD)) return PA_EINVAL;
    const int es = dtype == PA_BF16 ? 2 : 4;
    if ((ldqkv * es) % 16 != 0 || (d_o && (ldo * es) % 16 != 0)) return PA_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PA_BF16)
        return attention_rollout_t<bf16>(qkv, ldqkv, lse, d_o, ldo, do_compact, r_in, r_out, ws, cu_tok, total_tok, B, H, N, nq, nr, mode,
                                         slices, a, b_, g_scale, scale, flags, st);
    return attention_rollout_t<float>(qkv, ldqkv, lse, d_o, ldo, do_compact, r_in, r_out, ws, cu_tok, total_tok, B, H, N, nq, nr, mode, slices,
                                      a, b_, g_scale, scale, flags, st);
}

/* passt_amd.h -- C ABI of libpasst_amd.so, the MI355X (gfx950) implementation of the
 * kkoutini/PaSST training hot path.
 *
 * The reference has no FFI of its own: its hot path is a chain of ATen / torchaudio calls inside
 * two nn.Modules (models/preprocess.py:19 AugmentMelSTFT, models/passt.py:383 PaSST).  This
 * header is the boundary a maintainer binds instead (ctypes stub: INTEGRATION.md); each entry
 * point names the reference call sites (file:line under the reference root) it replaces.
 *
 * Conventions
 *   - plain C types only: raw DEVICE pointers, ints, floats; no torch types.
 *   - the CALLER allocates every output and workspace; the library never allocates or frees
 *     device memory and keeps no pointer after return.
 *   - every call is asynchronous and ordered on `stream` (a hipStream_t passed as void*);
 *     nothing synchronises the device.  Re-entrant: no mutable global state.
 *   - return value: 0 on success, a negative PA_E* code otherwise (never throws);
 *     pa_error_string(code) describes it.
 *   - `dtype` selects the storage/compute type of the "low precision" activations and GEMM
 *     operands: PA_F32 (exact-f32 MFMA, the <=1e-3 parity mode) or PA_BF16 (bf16 MFMA with f32
 *     accumulation, the throughput mode).  The residual stream, LayerNorm statistics, softmax,
 *     master weights and all weight gradients are always f32.
 *   - row-major everywhere; `ld*` are leading dimensions in ELEMENTS.
 */
#ifndef PASST_AMD_H
#define PASST_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_ABI_VERSION 6   /* 2 (round 3): pa_attention_* take flags, pa_attention_bwd workspace query, pa_gemm_args.colscale*;
                            * 3: pa_gemm_nt_splitk*;  4 (round 4): pa_comm_info, pa_adamw_dev / pa_adamw_hyper, PA_GEMM_EPILOGUE_V3;
                            * 5 (round 5): PA_ATTN_BWD_TWO_PASS (pa_attention_bwd defaults to the single-pass kernel where it applies);
                            * 6 (round 6): pa_adamw_stage (optimizer update + GEMM-ready weight copies in one pass) */

enum { PA_F32 = 0, PA_BF16 = 1 };

enum {
    PA_OK = 0,
    PA_EINVAL = -1,   /* bad argument (null pointer, negative size, ...) */
    PA_EUNSUPPORTED = -2, /* shape/dtype outside what the kernels cover */
    PA_ELAUNCH = -3,  /* hipLaunch failed; see pa_last_hip_error() */
    PA_ECOMM = -4     /* RCCL missing or a collective call failed; see pa_comm_last_error() */
};

int pa_abi_version(void);
const char* pa_error_string(int code);
/* hipGetLastError() of the calling thread as text (valid until the next call). */
const char* pa_last_hip_error(void);

/* ------------------------------------------------------------------------------------------
 * Front end: AugmentMelSTFT.forward, models/preprocess.py:57-86 (K1..K8 in SURVEY.md 2.3)
 * pre-emphasis (:59) -> STFT 1024/hop/hann(win) reflect-centred (:60-61) -> power (:62) ->
 * kaldi mel filterbank as a sparse band product (:71-76) -> log(x+eps) (:78) -> SpecAugment
 * frequency/time mask (:80-82) -> (x+4.5)/5 (:84), fused in one kernel.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int32_t n_fft;        /* must be 1024 */
    int32_t hop;          /* 320; any value in [1, 1024] */
    int32_t n_mels;       /* 4 .. 128 */
    int32_t n_frames;     /* T = 1 + (L-1-1+... ) see pa_mel_num_frames */
    float preemph;        /* 0.97: y[n] = x[n+1] - preemph*x[n]  (:46,:59) */
    float mel_low;        /* mel(fmin) = 1127 ln(1+fmin/700) */
    float inv_mel_delta;  /* (n_mels+1) / (mel(fmax) - mel(fmin)) */
    float log_eps;        /* 1e-5 (:78) */
    float out_add;        /* 4.5  (:84) */
    float out_scale;      /* 0.2  (:84) */
    int32_t fmask_start, fmask_end;   /* [start,end) mel rows forced to (0+out_add)*out_scale; empty if start>=end */
    int32_t tmask_start, tmask_end;   /* same along time */
} pa_mel_params;

/* frames produced for a waveform of L samples: 1 + (L-1)/hop  (pre-emphasis shortens by one) */
int pa_mel_num_frames(int L, int hop);
/* wave[B][L] f32 -> out[B][n_mels][n_frames] f32.
 * window[n_fft]  : analysis window already zero-padded/centred to n_fft (:38-40 + torch.stft rule)
 * bin_mel[n_fft/2]: mel value of FFT bin k, 1127 ln(1 + k*sr/n_fft/700) (kaldi.get_mel_banks)
 * twiddle[n_fft/2][2]: (cos, -sin)(2 pi k / n_fft), k = 0..n_fft/2-1
 * Alignment: `wave` must be 16-byte aligned, in all six front-end entry points.  The forward moves the span of an interior tile as
 * 16-byte pieces (vector loads, LDS-DMA in the persistent form) and the backward reads an interior frame as 8-byte pairs; both decide
 * from the element index b * L + i0 (b * ldw + i0 in the packed forms), i.e. relative to `wave`, whether a piece is aligned.  Rows
 * need no alignment of their own: with L (ldw) not a multiple of 4 the tiles of the misaligned rows are staged sample by sample.
 * The tables, out, dout, dwave, lens and clip need their natural 4-byte alignment only.
 * Argument checks, in this order, nothing is launched when one fails: PA_EINVAL for a null pointer or B <= 0 (the packed forms:
 * T_max <= 0, lens == NULL) and for a `wave` off 16-byte alignment; PA_EUNSUPPORTED for n_fft != 1024, n_mels outside [4, 128], hop
 * outside [1, 1024] and L - 1 <= n_fft/2 (the packed forms: ldw - 1 <= n_fft/2); PA_EINVAL for p->n_frames != pa_mel_num_frames(L, hop)
 * (the packed forms: p->n_frames != T_max, or T_max > pa_mel_num_frames(ldw, hop)). */
int pa_mel_frontend_fwd(const float* wave, int B, int L, const float* window, const float* bin_mel,
                        const float* twiddle, float* out, const pa_mel_params* p, void* stream);
/* The same for a batch of clips of different lengths (inference on ragged input; the reference runs such clips one at a time,
 * ex_fsd50k.py:53-56).  wave[B][ldw] f32, clips left-aligned; lens[B] int32 IN DEVICE MEMORY: valid samples of every row
 * (lens[b] <= ldw, lens[b] - 1 > n_fft/2; the caller checks both, the library cannot read them).  Row b of out[B][n_mels][T_max]
 * holds, in its first pa_mel_num_frames(lens[b], hop) columns, exactly what pa_mel_frontend_fwd returns for that clip alone
 * (pre-emphasis and the centred reflect padding end at the clip's own last sample; samples at or behind lens[b] are never read),
 * and `fill` in every column behind them.  p->n_frames must equal T_max = pa_mel_num_frames(max lens, hop) <= pa_mel_num_frames(ldw,
 * hop); the time mask of p applies to every row alike.  A row with lens[b] - 1 <= n_fft/2 is written as `fill` throughout.  One-tile
 * kernel form only (PA_MEL_PERSIST is ignored).  wave, lens, the three tables and out are device memory. */
int pa_mel_frontend_fwd_varlen(const float* wave, int B, int ldw, const int32_t* lens, const float* window, const float* bin_mel,
                               const float* twiddle, float* out, int T_max, float fill, const pa_mel_params* p, void* stream);
/* Gradient of pa_mel_frontend_fwd w.r.t. the waveform: dout[B][n_mels][n_frames] f32 -> dwave[B][L] f32, every element written.
 * The forward saves nothing; the spectrum and the band sums are recomputed from `wave` (same tables, same p -- including the mask
 * ranges of the forward call whose gradient is wanted).  One clip, f32, in the forward's order:
 *   forward   y[n] = x[n+1] - preemph x[n] (n < L-1);  yp = y reflect-padded by n_fft/2;  f_t[i] = yp[t hop + i] w[i];
 *             X_t[k] = sum_i f_t[i] exp(-2 pi i k i / n_fft), k = 0..n_fft/2;  P = |X|^2;  mel[b] = sum_k basis[b][k] P[k]
 *             (column n_fft/2 of the basis is zero);  out = (log(mel + log_eps) + out_add) out_scale, the constant out_add out_scale
 *             in masked rows / columns
 *   backward  1. dmel[b][t] = dout[b][t] out_scale / (mel[b][t] + log_eps); 0 at masked positions (dout is not read into the result
 *                there) and, in the varlen form, at every frame at or behind the clip's own frame count
 *             2. dP[k] = u_k dmel[j_k] + (1 - u_k) dmel[j_k - 1]   (j_k, u_k: triangle index and up-slope weight of bin k; bands
 *                outside [0, n_mels) count as 0): the transpose of the forward's band sums, a two-term gather
 *             3. G[k] = 2 dP[k] X[k] (k < n_fft/2), G[n_fft/2] = 0
 *             4. df_t[i] = Re sum_{k=0}^{n_fft/2-1} G[k] exp(+2 pi i k i / n_fft): the one-sided sum, no 1/N, no Hermitian doubling
 *                (the adjoint of the forward's sum, not irfft)
 *             5. dyp[t hop + i] += df_t[i] w[i], summed per sample over the frames in ascending t
 *             6. dy[m] = dyp[m + n_fft/2] + dyp[n_fft/2 - m] (1 <= m <= n_fft/2) + dyp[n_fft/2 + 2 (L-2) - m] (L-2-n_fft/2 <= m <= L-3)
 *             7. dwave[n] = dy[n-1] - preemph dy[n],  dy[-1] = dy[L-1] = 0
 * No floating-point atomics: the result is bit-repeatable and does not depend on the launch geometry.  The overlap-add happens inside
 * the workgroups, so no workspace is needed: `workspace` / `workspace_bytes` are reserved (pass NULL / 0) and ignored.
 * Same argument checks and error codes as pa_mel_frontend_fwd. */
int pa_mel_frontend_bwd(const float* wave, int B, int L, const float* window, const float* bin_mel, const float* twiddle,
                        const float* dout, float* dwave, void* workspace, int64_t workspace_bytes, const pa_mel_params* p, void* stream);
/* Gradient of pa_mel_frontend_fwd_varlen: wave[B][ldw], lens[B] (device), dout[B][n_mels][T_max] -> dwave[B][ldw].  Row b equals, in its
 * first lens[b] samples, what pa_mel_frontend_bwd returns for that clip alone (steps 6 and 7 at the clip's own end; frames at or behind
 * the clip's frame count and samples at or behind lens[b] are never read) and is exactly 0 at and behind lens[b] (a row with lens[b] - 1
 * <= n_fft/2: 0 throughout).  Equal lengths = ldw give pa_mel_frontend_bwd's result bit for bit. */
int pa_mel_frontend_bwd_varlen(const float* wave, int B, int ldw, const int32_t* lens, const float* window, const float* bin_mel,
                               const float* twiddle, const float* dout, int T_max, float* dwave, void* workspace, int64_t workspace_bytes,
                               const pa_mel_params* p, void* stream);
/* Training-time augmentation of a ragged batch (additive to ABI 6).  In the reference every clip that is processed alone gets its own
 * fmin / fmax jitter and its own two SpecAugment bands (models/preprocess.py:63-64, 80-82), the time band drawn against the clip's own
 * frame count.  One entry of this table per clip carries that draw: 24 bytes, the six per-clip fields of pa_mel_params. */
typedef struct {
    float mel_low;        /* mel(fmin) of this clip */
    float inv_mel_delta;  /* (n_mels+1) / (mel(fmax) - mel(fmin)) of this clip */
    int32_t fmask_start, fmask_end;   /* [start,end) mel rows of this clip forced to (0+out_add)*out_scale; empty if start>=end */
    int32_t tmask_start, tmask_end;   /* same along time (start may be negative) */
} pa_mel_clip_params;
/* pa_mel_frontend_fwd_varlen / pa_mel_frontend_bwd_varlen with clip[B] IN DEVICE MEMORY: row b is transformed with clip[b].mel_low /
 * .inv_mel_delta and masked with clip[b]'s two bands; p->mel_low, p->inv_mel_delta, p->fmask_* and p->tmask_* are ignored, everything
 * else in *p holds.  Row b equals, in its first pa_mel_num_frames(lens[b], hop) columns (its first lens[b] samples), what
 * pa_mel_frontend_fwd (pa_mel_frontend_bwd) returns for that clip alone with clip[b]'s six values in its pa_mel_params; the columns
 * behind them hold `fill`, never the mask constant (dwave: exactly 0 at and behind lens[b]).  A table whose entries all repeat *p's six
 * values gives the _varlen entry points' results bit for bit.  The library cannot read the table: the caller guarantees finite mel_low
 * and inv_mel_delta > 0 in every entry, as it guarantees lens.  Same argument checks and error codes as the _varlen entry points, plus
 * PA_EINVAL for clip == NULL. */
int pa_mel_frontend_fwd_varlen_aug(const float* wave, int B, int ldw, const int32_t* lens, const float* window, const float* bin_mel,
                                   const float* twiddle, float* out, int T_max, float fill, const pa_mel_params* p,
                                   const pa_mel_clip_params* clip, void* stream);
int pa_mel_frontend_bwd_varlen_aug(const float* wave, int B, int ldw, const int32_t* lens, const float* window, const float* bin_mel,
                                   const float* twiddle, const float* dout, int T_max, float* dwave, void* workspace, int64_t workspace_bytes,
                                   const pa_mel_params* p, const pa_mel_clip_params* clip, void* stream);

/* ------------------------------------------------------------------------------------------
 * Parameter staging (no reference counterpart: AMP autocast casts weights per op)
 * ------------------------------------------------------------------------------------------ */
/* Casts to bf16 everywhere in this library round to nearest even; NaN stays NaN, the largest finite f32 rounds to inf, f32 subnormals
 * round like any other value (to +-0 or a bf16 subnormal) -- bit for bit what torch's CPU cast gives (tests/patch_cases.py, tie family).
 * out[i] = (dtype) in[i].  `in` needs only its natural 4-byte alignment: a pointer off 16 bytes (a parameter at an arbitrary offset of a
 * flat buffer) is read with scalar loads instead of 16-byte vectors; `out` is written element by element. */
int pa_convert_f32(const float* in, void* out, int64_t n, int dtype, void* stream);
/* out[m][d] = (dtype)(rowscale[m] * in[m][d]), in [M][D] f32, D % 4 == 0: the copy of a gradient that enters a branch carrying a
 * stochastic-depth row factor (DropPath, models/helpers/vit_helpers.py:203-222 as Block applies it to the MLP branch,
 * models/passt.py:378-379) -- where the head's gradient enters the last block.  With dtype PA_F32 `out` is a second f32 buffer.
 * rowscale NULL: pa_convert_f32 over M * D elements.  With a rowscale, `in` and `out` must be 16-byte aligned (four columns per access;
 * PA_EINVAL otherwise, nothing launched); rowscale itself is read one float per row. */
int pa_convert_f32_rowscale(const float* in, const float* rowscale, void* out, int M, int D, int dtype, void* stream);
/* out[i] = (float) in[i], in of `dtype` (the bf16 gradient wire of the data-parallel reducer, passt_amd/ddp.py).  Either pointer off
 * 16 bytes: scalar accesses instead of vectors. */
int pa_convert_to_f32(const void* in, int dtype, float* out, int64_t n, void* stream);
/* Batched form of the two calls below, for refreshing every GEMM-ready weight copy after an optimizer
 * step in ONE launch: entry e reads src[rows][cols] (f32, contiguous) and writes, where non-NULL,
 * dst[rows][cols] (straight cast) and dst_t[cols][rows] (transposed), both of `dtype` and contiguous.
 * `descs` is an array of n_desc entries in DEVICE memory; tile_begin is the running count of 64x64 tiles
 * (ceil(rows/64)*ceil(cols/64) per entry, in order); total_tiles is their sum.
 * Alignment: none required beyond the element's own.  An entry takes the vector path (16-byte loads, 4-element stores) when rows and
 * cols are multiples of 4, src is 16-byte aligned and dst / dst_t (where given) are aligned to 4 elements (8 bytes in bf16, 16 in
 * f32); any other entry is moved element by element -- the table lives in device memory, so the kernel decides, per entry. */
typedef struct pa_stage_desc {
    const float* src;
    void* dst;
    void* dst_t;
    int32_t rows, cols;
    int32_t tile_begin;
    int32_t reserved;
} pa_stage_desc;
int pa_stage_weights(const pa_stage_desc* descs, int n_desc, int total_tiles, int dtype, void* stream);
/* in[R][C] (ld = ldi) of dtype in_dtype -> out[C][ldo] of dtype out_dtype, out[c][r] = in[r][c];
 * columns r in [R, ldo) of out are zero-filled (K-padding for the weight-gradient GEMM), whole 64-column tiles behind R included.
 * Element accesses only: no alignment beyond the element's own. */
int pa_transpose(const void* in, int in_dtype, int R, int C, int ldi, void* out, int out_dtype,
                 int ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm: nn.LayerNorm in Block (models/passt.py:369,373,378-379; eps 1e-6 :426), final norm
 * (:450,:570) and head.0 (:463, eps 1e-5).  K15 in SURVEY.md.
 * ------------------------------------------------------------------------------------------ */
/* x[M][D] f32 -> y[M][D] (dtype), mean[M], rstd[M] f32 (saved for backward; may be NULL). */
int pa_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* y, int dtype,
                     float* mean, float* rstd, int M, int D, float eps, void* stream);
/* dx[M][D] = (dres ? dres : 0) + LN'(dy); optional dx_lp (dtype) copy of dx for the next GEMM.
 * dgamma/dbeta[D] are OVERWRITTEN (or accumulated when accumulate != 0).
 * dcolsum[D] (optional): column sums of the OUTPUT dx -- the bias gradient of the Linear whose output fed
 * this LayerNorm through the residual stream (proj.bias for norm2, the previous block's fc2.bias for norm1),
 * fused here because the kernel already reduces over rows.
 * ws: f32 workspace of pa_layernorm_bwd_ws_floats(M, D) elements. */
int64_t pa_layernorm_bwd_ws_floats(int M, int D);
int pa_layernorm_bwd(const void* dy, int dtype, const float* x, const float* gamma,
                     const float* mean, const float* rstd, const float* dres, float* dx,
                     void* dx_lp, float* dgamma, float* dbeta, float* dcolsum, int accumulate, float* ws,
                     int M, int D, void* stream);
/* The same without the finishing launch (ABI 5): dx / dx_lp are complete, the parameter gradients stay as
 * pa_layernorm_bwd_rows(M) partial rows ws[row][3][D] = {dgamma | dbeta | column sums of dx}; the caller reduces them with
 * pa_reduce_partials_batched (PA_REDUCE_ROWS, pitch 3 D) -- together with the block's other finishing reductions. */
int pa_layernorm_bwd_rows(int M);
int pa_layernorm_bwd_partial(const void* dy, int dtype, const float* x, const float* gamma,
                             const float* mean, const float* rstd, const float* dres, float* dx,
                             void* dx_lp, float* ws, int M, int D, void* stream);
/* Both with a second optional addend: dx = (dres ? dres : 0) + (dres2 ? dres2 : 0) + LN'(dy).  dres2 is a gradient injected into
 * the residual stream at this LayerNorm's input (a loss on a block's output tokens): it enters before the 16-bit copy and the
 * column sums are formed, so dx_lp and dcolsum (the bias gradient of the Linear behind that output) include it.  With dres2 NULL
 * the results are bit-identical to pa_layernorm_bwd / pa_layernorm_bwd_partial. */
int pa_layernorm_bwd2(const void* dy, int dtype, const float* x, const float* gamma,
                      const float* mean, const float* rstd, const float* dres, const float* dres2, float* dx,
                      void* dx_lp, float* dgamma, float* dbeta, float* dcolsum, int accumulate, float* ws,
                      int M, int D, void* stream);
int pa_layernorm_bwd2_partial(const void* dy, int dtype, const float* x, const float* gamma,
                              const float* mean, const float* rstd, const float* dres, const float* dres2, float* dx,
                              void* dx_lp, float* ws, int M, int D, void* stream);

/* The four calls above with a per-row factor on the branch the gradient enters (stochastic depth: DropPath,
 * models/helpers/vit_helpers.py:203-233, applied to both branches of a Block, models/passt.py:372, 378-379): rowscale[M] f32 is
 * keep / (1 - p) of the clip the row belongs to.  dx (f32) stays the residual gradient, unscaled; the copy is
 * dx_lp[m][:] = (dtype)(rowscale[m] * dx[m][:]) -- with dtype PA_F32 a second f32 buffer, which must not be dx -- and the third
 * column sum (dcolsum: the branch's bias gradient) is the sum of the scaled rows.  dres2 may be NULL (the one-addend forms).
 * dx, dgamma and dbeta are bit-identical to the call without a factor; rowscale NULL IS that call. */
int pa_layernorm_bwd_rowscale(const void* dy, int dtype, const float* x, const float* gamma, const float* mean,
                              const float* rstd, const float* dres, const float* dres2, const float* rowscale, float* dx,
                              void* dx_lp, float* dgamma, float* dbeta, float* dcolsum, int accumulate, float* ws, int M,
                              int D, void* stream);
int pa_layernorm_bwd_partial_rowscale(const void* dy, int dtype, const float* x, const float* gamma, const float* mean,
                                      const float* rstd, const float* dres, const float* dres2, const float* rowscale,
                                      float* dx, void* dx_lp, float* ws, int M, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * GEMM  C[M][N] = A[M][K] * B[N][K]^T  (both operands K-contiguous), MFMA, f32 accumulation.
 * Replaces every nn.Linear of the path: qkv (models/passt.py:345), proj (:359), fc1+GELU
 * (:285-286), fc2 (:288), the patch-embed conv as an im2col GEMM (:323) and, with transposed
 * operands, all their input/weight gradients (autograd mm / addmm backward; K26).
 * ------------------------------------------------------------------------------------------ */
enum {
    PA_EPI_STORE = 0,      /* out_lp = acc + bias                                   */
    PA_EPI_GELU = 1,       /* out_lp = acc + bias ; out_lp2 = gelu_erf(out_lp)      */
    PA_EPI_RESID = 2,      /* out_f32[orow] = acc + bias + resid[rrow]  (f32 residual stream) */
    PA_EPI_DGELU = 3,      /* out_lp = acc * gelu_erf'(aux)                         */
    PA_EPI_PARTIAL = 4     /* split-K: out_f32[z][M][N] = partial sums (no bias)    */
};
/* PA_EPI_PARTIAL, pa_gemm_nt: slab z starts at out_f32 + z * M * ldo32 and holds the product over K steps [z * per, (z + 1) * per),
 * per = ceil(steps / split_k), a step being 128 bytes of K (64 bytes for tune 9); a slab whose range is empty (ceil-divided slices:
 * e.g. 4 steps in 3 slices of 2) is written as zeros.  tune 13 / 19 have the fused epilogues only: PA_EPI_PARTIAL is PA_EINVAL. */
typedef struct {
    int32_t dtype;         /* PA_F32 / PA_BF16: type of A, B, aux, out_lp, out_lp2 */
    int32_t epilogue;
    int32_t M, N, K;       /* K*sizeof(dtype) must be a multiple of 128 bytes */
    int32_t lda, ldb;
    const void* A;
    const void* B;
    const float* bias;     /* [N] or NULL */
    const float* resid;    /* PA_EPI_RESID: f32 [*][ldr] */
    int32_t ldr;
    /* PA_EPI_RESID row remap (patch-embed writes token rows and adds a per-patch table):
     * if row_mod > 0: rrow = m % row_mod, orow = (m / row_mod) * out_batch_rows + out_row_off + m % row_mod
     * else rrow = orow = m. */
    int32_t row_mod, out_batch_rows, out_row_off;
    const void* aux;       /* PA_EPI_DGELU: pre-activation [M][ldaux] (dtype) */
    int32_t ldaux;
    float* out_f32;        /* PA_EPI_RESID / PA_EPI_PARTIAL */
    int32_t ldo32;
    void* out_lp;
    int32_t ldolp;
    void* out_lp2;
    int32_t ldolp2;
    int32_t split_k;       /* PA_EPI_PARTIAL: number of K slices (grid.z); else must be 1 */
    int32_t tune;          /* 0 = library heuristic (tile quantisation x measured rates).  Forcing a variant
                            * (benchmarking / autotuning), pa_gemm_nt bf16: 1 = 128x128 tile, 4 waves, 2 workgroups/CU;
                            * 2 = 256x256 lockstep; 6 / 7 / 8 = role-split 256x256 / 192x256 / 128x256 (8 waves,
                            * staggered wave groups); 9 = 128x256, 4 waves, 64-byte stages, 2 workgroups/CU (slower: DESIGN.md 4.1).
                            * 17 / 18 = 7 / 8 with three A slots (A requested two K-tiles ahead; what 0 picks for them).
                            * 3 = 192x128, 4 waves, 80 KiB: 2 workgroups/CU (first-generation epilogue; with PA_GEMM_BLOCKED_PRE: epilogue
                            * v2 + blocked pre-activation; PA_NT_MLP_2WG=1 makes 0 pick it for the large MLP-epilogue GEMMs);
                            * 13 / 19 = 3 / 9 with epilogue v2 and row-major outputs (round 6, A/B: profiles/r06_gemm_variants_epi13.txt).
                            * pa_gemm_tn bf16: 1 = 128x128, otherwise role-split 256x256.  pa_gemm_tn_batched: tune of the
                            * FIRST problem = 2 orders the work items problem-major instead of slice-major (A/B only). */
    /* PA_EPI_DGELU only, optional: colsum_out[n] = (colsum_accumulate ? colsum_out[n] : 0) + sum_m out[m][n] (of the
     * f32 values, before rounding) -- the bias gradient of the Linear whose pre-activation is `aux` (fc1.bias),
     * reduced inside the epilogue instead of by a separate pass over out_lp.  colsum_ws: f32 workspace of
     * pa_gemm_colsum_ws_floats(M, N) elements.  NULL colsum_out: not computed. */
    float* colsum_out;
    float* colsum_ws;
    int32_t colsum_accumulate;
    int32_t reserved;      /* flags: 0, or PA_GEMM_BLOCKED_PRE (bits 0..7 are ignored by the product library) */
    /* PA_EPI_STORE only: out_lp[m][n] = (acc + bias[n]) * colscale for the columns n < colscale_n (a multiple of 64; 0 = off),
     * one rounding.  The qkv Linear writes q * head_dim^-0.5 * log2(e) this way for pa_attention_*(PA_ATTN_Q_PRESCALED). */
    int32_t colscale_n;
    float colscale;
} pa_gemm_args;
/* PA_EPI_GELU: out_lp (the pre-activation) is written, PA_EPI_DGELU: aux (the same tensor) is read, in the library's
 * blocked layout instead of row-major -- 4 KiB blocks of 32 rows x 64 columns in MFMA accumulator order, which both
 * epilogues move with contiguous 16-byte-per-lane accesses and no LDS transposition.  The buffer is opaque to the caller:
 * pa_gemm_blocked_pre_elems(M, N) elements (rows padded to whole tiles), ldolp / ldaux ignored.  Only for shapes where
 * pa_gemm_blocked_pre_ok(M, N, K) returns 1 (bf16, tune = 0); otherwise pa_gemm_nt returns PA_EUNSUPPORTED. */
#define PA_GEMM_BLOCKED_PRE 0x100
/* pa_gemm_nt, role-split kernels: one work item per workgroup (hardware dispatch) instead of the persistent form, for callers
 * that run another kernel next to the GEMMs -- the gradient all-reduce of data-parallel training (ex_audioset.py:488-489): a
 * persistent launch whose workgroups cannot all be resident at once takes twice as long.  Same results. */
#define PA_GEMM_NO_PERSIST 0x400
/* pa_gemm_nt, bf16 role-split kernels: run this call with the LDS-free epilogue (round 4: accumulators computed transposed,
 * rows loaded / stored straight from the registers) instead of the default one that transposes the output tile through LDS.
 * Bit-identical results; measured slower in the training step (partial-line stores), kept for A/B measurements and the
 * equality test.  PA_EPILOGUE_V3=1 in the environment selects it process-wide. */
#define PA_GEMM_EPILOGUE_V3 0x1000
/* PA_EPI_DGELU with colsum_out (ABI 5): leave the column sums as partial rows in colsum_ws (one per wave tile) and skip the
 * finishing launch; pa_gemm_last_colsum_rows() (the calling thread's last such call) says how many rows were written, the caller
 * reduces them with pa_reduce_partials_batched (PA_REDUCE_ROWS, pitch N).  colsum_out must still be non-NULL (it is not written). */
#define PA_GEMM_COLSUM_DEFER 0x2000
int pa_gemm_blocked_pre_ok(int M, int N, int K);
int64_t pa_gemm_blocked_pre_elems(int M, int N);
int64_t pa_gemm_colsum_ws_floats(int M, int N);
/* Memory policy (round 6, csrc/pa_common.h CP_*): the bf16 outputs (out_lp, out_lp2), the blocked pre-activation and the epilogue
 * operand rows (resid, aux) of the bf16 role-split kernels are written / read NON-TEMPORALLY, as is the A operand of PA_EPI_RESID
 * calls: they are complete and visible at the end of the launch like any other result; a consumer simply finds them in HBM rather
 * than in the Infinity Cache.  A library built with -DPA_NO_CACHE_POLICY uses the default policy everywhere (same results). */
int pa_gemm_nt(const pa_gemm_args* a, void* stream);
/* The same product for problems too small to fill the chip (few output tiles, long K: the [M][768] outputs of fc2 / the
 * fc1 and qkv input gradients at ESC-50 batch sizes, ex_esc50.py:40; the prefix-only tail of the last block): K is cut into
 * pa_gemm_nt_splitk_plan(...) slices whose f32 partial tiles go to the caller's workspace `ws` (at least
 * pa_gemm_nt_splitk_ws_floats(...) floats) and one elementwise pass applies the epilogue.  PA_EPI_STORE / PA_EPI_RESID
 * (row_mod == 0), bf16, tune == 0; whenever the plan is 1 slice -- or ws is NULL / too small -- this IS pa_gemm_nt(a).
 * Results differ from pa_gemm_nt only in the order of the f32 partial sums. */
int pa_gemm_nt_splitk_plan(int M, int N, int K, int epilogue, int dtype);
int64_t pa_gemm_nt_splitk_ws_floats(int M, int N, int K, int epilogue, int dtype);
int pa_gemm_nt_splitk(const pa_gemm_args* a, float* ws, int64_t ws_floats, void* stream);
/* PA_EPI_RESID (row_mod == 0) with a per-row factor on the product: out_f32[m][n] = resid[m][n] + rowscale[m] * (acc + bias[n]),
 * rowscale[M] f32 -- the branch of a Block under stochastic depth, x + drop_path(branch) (DropPath, models/helpers/vit_helpers.py:
 * 203-233; models/passt.py:378-379), with rowscale[m] = keep / (1 - p) of row m's clip.  Kernel instantiations of their own (the
 * generic epilogue in bf16 and f32, the role-split epilogues v2 and v3, PA_GEMM_NO_PERSIST, the split-K finishing pass): a row
 * whose factor is 0 leaves resid as it is, a factor of 1 gives pa_gemm_nt's result bit for bit, and out_f32 may be resid.
 * a->tune other than 1 / 6 / 7 / 8 / 17 / 18 is ignored.  rowscale NULL IS pa_gemm_nt / pa_gemm_nt_splitk.
 * PA_EINVAL: another epilogue or the row remap with a factor. */
int pa_gemm_nt_rowscale(const pa_gemm_args* a, const float* rowscale, void* stream);
int pa_gemm_nt_splitk_rowscale(const pa_gemm_args* a, const float* rowscale, float* ws, int64_t ws_floats, void* stream);
/* Weight gradient  C[a->M][a->N] = sum_{m < a->K} A[m][a->M]^T B[m][a->N]  (A = dY, B = X, both row-major
 * [tokens][features] read IN PLACE, no transposed copies).  epilogue must be PA_EPI_PARTIAL: split-K over
 * the token axis, out_f32[split_k][M][N] partial slabs, finished by pa_reduce_partials (deterministic).
 * Optional (bf16 role-split kernel only, i.e. tune != 1): colsum_ws != NULL asks for the column sums of A as well --
 * colsum_ws[split_k][a->M] partial sums over each slice's tokens (the bias gradient of the Linear whose output
 * gradient is A: nn.Linear, models/passt.py:345), computed by one extra MFMA per phase in the tiles of the first
 * B-column block instead of a separate pass over A; finish with pa_reduce_partials(colsum_ws, split_k, a->M, ...).
 * colsum_out / colsum_accumulate are ignored here.
 * Slab z starts at out_f32 + z * a->M * ldo32 and holds the tokens of steps [z * per, (z + 1) * per), per = ceil(steps / split_k), a
 * step being PA_TN_STEP_ROWS tokens in the bf16 role-split kernel, 64 with bf16 tune = 1 and 32 in f32; an empty range gives zeros.
 * PA_EUNSUPPORTED: another epilogue, lda / ldb off 16 bytes, ldo32 % 4, a->N % 8, a->M not a multiple of one 16-byte vector of
 * `dtype` (8 bf16 / 4 f32) or either below it, colsum_ws with f32 or tune = 1. */
int pa_gemm_tn(const pa_gemm_args* a, void* stream);
/* Up to PA_TN_BATCH_MAX bf16 weight-gradient problems in ONE launch (e.g. the four Linears of a transformer block,
 * once all their operands exist): the work items of all problems share one grid, so there is no drain / prologue
 * between problems and items of different length pack onto the CUs.  Same arguments and results as n calls of
 * pa_gemm_tn; `a` is a HOST array.  When all problems use the same split_k the items are dealt slice-major with
 * every XCD owning a contiguous run, so the tiles sharing a dY / X panel of a token slice share an L2. */
#define PA_TN_BATCH_MAX 4
/* tokens the bf16 role-split weight-gradient kernel consumes per pipeline stage: a K slice of pa_gemm_tn /
 * pa_gemm_tn_batched is ceil(ceil(K / PA_TN_STEP_ROWS) / split_k) such steps (callers sizing split_k use it) */
#ifndef PA_TN_STEP_ROWS
#define PA_TN_STEP_ROWS 48
#endif
int pa_gemm_tn_step_rows(void);    /* the value the library was built with */
int pa_gemm_tn_batched(const pa_gemm_args* a, int n, void* stream);
/* The same launch with UNEQUAL token slices (problems that all have the same token count a->K): every 256 x 256 tile's
 * steps = ceil(K / PA_TN_STEP_ROWS) token steps are cut into n_long slices of long_steps steps (slabs 0 .. n_long - 1) and
 * one short slice of the steps - n_long * long_steps >= 1 that are left (slab n_long).  split_k of every problem must be
 * n_long + 1, the number of slabs out_f32 (and colsum_ws) hold; finish with pa_reduce_partials(_batched) as before.  The
 * long items of all tiles are launched first, slice-major with every XCD owning a contiguous run; the short items follow in
 * an XCD-contiguous order of their own and fill the CUs the first dispatch wave left free.  Results differ from
 * pa_gemm_tn_batched only in the grouping of the f32 partial sums.
 * PA_EINVAL: n_long < 1, long_steps < 1, n_long * long_steps >= steps (the short slice is never empty), split_k != n_long + 1.
 * PA_EUNSUPPORTED: token counts that differ between the problems (and whatever pa_gemm_tn_batched does not support). */
int pa_gemm_tn_batched_plan(const pa_gemm_args* a, int n, int n_long, int long_steps, void* stream);
/* Row gather / scatter and strided zero fill (prefix-token path of the last block):
 * gather: out[i] = in[idx[i]]; scatter: out[idx[i]] = in[i]; rows of row_bytes bytes (multiple of 4).  in and out must be 4-byte
 * aligned (PA_EINVAL otherwise); rows move as 16-byte vectors when row_bytes, in and out are all multiples of 16, as 4-byte words
 * otherwise.  idx[i] in [0, rows) is the caller's duty and is NOT checked; scatter: distinct idx (a repeated one leaves either row). */
int pa_gather_rows(const void* in, const int32_t* idx, int n_idx, int64_t row_bytes, void* out, void* stream);
int pa_scatter_rows(const void* in, const int32_t* idx, int n_idx, int64_t row_bytes, void* out, void* stream);
/* Gradient of the last block's full-rows output: dx[M][D] = (add0 ? add0 : 0) + (add1 ? add1 : 0) + scatter(rows[n_idx][D] at
 * idx), f32, plus the copy dx_lp (dtype; optional) in the same pass.  idx: strictly ascending rows in [0, M); a row idx does not
 * name gets the addends only (exactly 0 when both are NULL).  Replaces pa_zero2d + pa_scatter_rows + an add.  D % 4 == 0
 * (PA_EUNSUPPORTED); rows, add0, add1, dx and dx_lp must be 16-byte aligned where given (float4 columns; PA_EINVAL otherwise, nothing
 * launched).  idx in range and ascending is the caller's duty and is not checked. */
int pa_tail_inject(const float* rows, const int32_t* idx, int n_idx, const float* add0, const float* add1, float* dx,
                   void* dx_lp, int dtype, int M, int D, void* stream);
/* zero `rows` rows of width_bytes at pitch_bytes; the bytes of the pitch gap are not touched.  Any alignment: 16-byte stores when ptr,
 * pitch and width are multiples of 16 and pitch != width, the runtime's memset (1-D when pitch == width, else 2-D) otherwise. */
int pa_zero2d(void* ptr, int64_t pitch_bytes, int64_t width_bytes, int64_t rows, void* stream);
/* out[i] = (accumulate ? out[i] : 0) + sum_z partial[z][i], i < n */
int pa_reduce_partials(const float* partial, int splits, int64_t n, float* out, int accumulate,
                       void* stream);
/* the same for up to PA_REDUCE_BATCH_MAX reductions in one launch (`d` is a HOST array).  Two forms (ABI 5):
 *   mode PA_REDUCE_SLABS (0): out[i] (+)= sum_{z < splits} partial[z * n + i], i < n -- few slices of a long vector (the split-K
 *                             slabs of the weight gradients); 16-byte accesses, one thread per four outputs;
 *   mode PA_REDUCE_ROWS  (1): out[c] (+)= sum_{r < splits} partial[r * pitch + c], c < n -- MANY short rows (the per-workgroup
 *                             partial rows of pa_layernorm_bwd_partial, the per-wave-tile rows of a deferred PA_EPI_DGELU column
 *                             sum): 16 columns x 16 row groups per workgroup, four loads in flight per thread.
 * One launch per transformer block finishes all of its parameter gradients: four weight gradients + qkv.bias (slabs), two
 * LayerNorms' dgamma | dbeta and the bias gradient each of them carries, fc1.bias (rows). */
#define PA_REDUCE_BATCH_MAX 12
#define PA_REDUCE_SLABS 0
#define PA_REDUCE_ROWS 1
typedef struct pa_reduce_desc {
    const float* partial;
    float* out;
    int64_t n;
    int32_t splits;
    int32_t accumulate;
    int64_t pitch;         /* PA_REDUCE_ROWS: floats between two rows of `partial` (SLABS: ignored, the slices are dense) */
    int32_t mode;
    int32_t reserved;
} pa_reduce_desc;
int pa_reduce_partials_batched(const pa_reduce_desc* d, int n, void* stream);
int pa_gemm_last_colsum_rows(void);
/* out[r] = (accumulate ? out[r] : 0) + sum_c in[r][c], c < C  (bias gradients from dY^T) */
int pa_rowsum(const void* in, int dtype, int R, int C, int ld, float* out, int accumulate,
              void* stream);
/* out[c] = (accumulate ? out[c] : 0) + sum_r in[r][c] for a tall [R][C] matrix of `dtype` (bias gradients
 * straight from dY); ws: f32 workspace of pa_colsum_ws_floats(R, C) elements. */
int64_t pa_colsum_ws_floats(int R, int C);
int pa_colsum(const void* in, int dtype, int R, int C, int ld, float* out, int accumulate, float* ws,
              void* stream);
/* out[c] = (accumulate ? out[c] : 0) + sum_r in[r][c]  -- f32 in, small R (head/LN partials) */
int pa_colsum_f32(const float* in, int R, int C, int ld, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention: Attention.forward, models/passt.py:343-361 minus the two Linears (K17-K19):
 * softmax((Q K^T) * scale) V per (batch, head), flash-style (scores never reach HBM), head_dim 64.
 * q/k/v are read in place from the qkv GEMM output [B*N][3*H*64] ([q|k|v] x head x 64, the
 * reshape of :345); o is written token-major [B*N][H*64] (the transpose+reshape of :358).
 *
 * nq (1..N): only the first nq queries of every sequence are produced -- N for a normal block; 2 for the LAST
 * block, whose output is only ever read at the cls/dist rows (models/passt.py:570-574).  o, d_o, lse and delta are
 * then COMPACT: o[(b*nq + q)][H*64], lse[(b*H + h)*nq + q].  K and V always span all N tokens.
 *
 * flags: 0, or PA_ATTN_Q_PRESCALED: the q third of qkv holds q * scale * log2(e) (the qkv GEMM wrote it so:
 * pa_gemm_args.colscale_n / colscale, one rounding).  The kernels then take "score - row reference" straight from the
 * matrix pipe (no multiply-add per score); o, lse and every gradient are the same quantities as without the flag
 * (dqkv's q third is the gradient with respect to the UNSCALED q).  The same flag must be given to fwd and bwd.
 *
 * Leading dimensions are in elements.  Every entry of this section refuses one below its row width with PA_EINVAL before anything is
 * launched -- ldqkv, lddqkv < 3*H*64, ldo < H*64 (o and d_o share ldo) -- and one whose rows are not 16-byte aligned with
 * PA_EUNSUPPORTED.  Gap columns of a padded leading dimension are neither read nor written.
 * ------------------------------------------------------------------------------------------ */
#define PA_ATTN_Q_PRESCALED 1
/* pa_attention_bwd only (ABI 5).  bf16 + PA_ATTN_Q_PRESCALED + nq == N <= 512 can run as ONE kernel (one workgroup per
 * (sequence, head): S / dP / exp formed once, dQ contracted over all keys through an LDS transposition buffer; `delta` is then not
 * touched) instead of the dQ kernel followed by the dK/dV kernel: same quantities, both deterministic.  By default the library
 * picks the single pass when B * H >= 512 (two rounds of 256 CUs).  PA_ATTN_BWD_TWO_PASS forces the kernel pair,
 * PA_ATTN_BWD_SINGLE_PASS the single kernel wherever it applies (elsewhere it is ignored).
 * PA_ATTN_BWD_SINGLE_PASS_W16 (ABI 6): the single kernel in its sixteen-wave form (1024 threads, four waves per SIMD, one
 * 32-key block per wave) wherever the single pass applies -- same quantities; measured against the eight-wave form in
 * profiles/r06_attention_w16.txt. */
#define PA_ATTN_BWD_TWO_PASS 2
#define PA_ATTN_BWD_SINGLE_PASS 4
#define PA_ATTN_BWD_SINGLE_PASS_W16 8
/* PA_EINVAL: ldqkv < 3*H*64 or ldo < H*64 (as well as a NULL pointer, a size <= 0, nq > N, an unknown flag or dtype). */
int pa_attention_fwd(const void* qkv, int ldqkv, void* o, int ldo, float* lse, int B, int H, int N, int nq,
                     float scale, int dtype, int flags, void* stream);
/* Forward over PACKED sequences of different lengths (ragged batches; backward: pa_attention_bwd_varlen).  The B sequences lie back to back
 * in qkv: sequence b owns token rows cu_tok[b] .. cu_tok[b+1] - 1, N_b = cu_tok[b+1] - cu_tok[b] >= 1; cu_tok is B + 1 int32 IN
 * DEVICE MEMORY with cu_tok[0] = 0, non-decreasing, and max_N >= every N_b (it only sizes the launch: cdiv(max_N, 128) query blocks
 * per (sequence, head), the ones a short sequence does not have return at once).  Every sequence gets bit for bit what
 * pa_attention_fwd(B = 1, N = N_b) computes for it alone: same tile loop, same tail instances; the K / V rows staged for a
 * sequence's last tile are clamped to ITS last row, so no row of a neighbour and no row at or behind cu_tok[B] is ever read (qkv
 * needs no slack after its last row).
 *   nq >= max_N: every query.  o is packed like qkv's rows, o[cu_tok[b] + q][H*64]; lse is head-major over the packed rows,
 *                lse[h * cu_tok[B] + cu_tok[b] + q]  (H * cu_tok[B] floats).
 *   nq <  max_N: the first min(nq, N_b) queries of every sequence, COMPACT as in pa_attention_fwd: o[(b*nq + q)][H*64],
 *                lse[(b*H + h)*nq + q]  (nq = 2: the last block's prefix rows); rows q >= N_b are not written.
 * flags as pa_attention_fwd.  qkv, o, lse, cu_tok are device memory.  PA_EINVAL: ldqkv < 3*H*64 or ldo < H*64. */
int pa_attention_fwd_varlen(const void* qkv, int ldqkv, void* o, int ldo, float* lse, const int32_t* cu_tok, int B, int H,
                            int max_N, int nq, float scale, int dtype, int flags, void* stream);
/* The attention probabilities themselves, softmax((Q K^T) * scale), f32: what the fused forward never writes (a forward hook on the
 * reference's attn_drop sees them, models/passt.py:348-352).  qkv, ldqkv, nq, scale, dtype (PA_F32 / PA_BF16) and flags
 * (PA_ATTN_Q_PRESCALED) are those of the pa_attention_fwd / pa_attention_fwd_varlen call that wrote `lse`, which is read in the layout
 * that call left: lse[(b*H + h)*nq + q] (fixed, or packed with nq < max_N) or lse[h*cu_tok[B] + cu_tok[b] + q] (packed, nq >= max_N).
 * A probability is exp2(score * log2 e - lse * log2 e) with the score from the matrix pipe: every (32 queries x 32 keys) tile stands
 * alone -- no second pass, no atomics, deterministic.  Ho = head_mean ? 1 : H output planes per sequence; head_mean (0 / 1) averages
 * the H heads in f32 registers, in head order.
 *   cu_tok == NULL (out_off must be NULL): B sequences of N tokens, out[((b*Ho + h)*nq + q)*N + k], nq <= N.
 *   cu_tok != NULL: packed sequences as in pa_attention_fwd_varlen, N = max_N; sequence b lies dense at out[out_off[b]] as
 *     [Ho][min(nq, N_b)][N_b]; out_off: B int64 offsets in device memory.  Tail tiles are clamped to the sequence's own last row (no
 *     row of a neighbour and none at or behind cu_tok[B] is read) and every sequence gets bit for bit what the fixed form gives it
 *     alone at B = 1.
 * Every element of the output is written and nothing else.  Key lanes at or behind N_b are masked before the exponential.
 * PA_EINVAL: ldqkv < 3*H*64. */
int pa_attention_probs(const void* qkv, int ldqkv, const float* lse, float* out, const int32_t* cu_tok, const int64_t* out_off,
                       int B, int H, int N /* max_N when cu_tok != NULL */, int nq, int head_mean, float scale, int dtype, int flags,
                       void* stream);
/* The gradient of the loss with respect to those probabilities, f32: what the fused backward forms tile by tile in registers and
 * never writes (retain_grad() on the input of the reference's attn_drop holds it after the backward).  A sibling of
 * pa_attention_probs: same arguments with the same meaning, same work decomposition, same clamping, same two output layouts, every
 * element of the output written and nothing else, no LDS / barrier / atomics, bit-repeatable.  Per (32 x 32) tile and head
 *   g[q][k] = sum_d d_o[q][h*64 + d] * v[k][h*64 + d]      (f32 accumulation)
 * d_o, ldo: the output gradient of the fused attention as the block's pa_attention_bwd / pa_attention_bwd_varlen call reads it
 * (dtype of qkv, ldo >= H*64 elements).  do_compact = 0: d_o's rows are qkv's token rows and only the rows q < nq of a sequence are
 * read; do_compact = 1: the compact prefix form d_o[(b*nq + q)][H*64].
 *   mode PA_ATTN_PGRAD_GRAD: out = g.  head_mean must be 0; lse is not read and may be NULL.
 *   mode PA_ATTN_PGRAD_CAM:  out = max(p * g, 0) with p formed exactly as pa_attention_probs forms it from qkv and lse; with
 *     head_mean = 1 the mean over the heads of that, added in f32 registers in head order.
 * PA_EINVAL: ldqkv < 3*H*64 or ldo < H*64. */
#define PA_ATTN_PGRAD_GRAD 0
#define PA_ATTN_PGRAD_CAM 1
int pa_attention_probs_grad(const void* qkv, int ldqkv, const float* lse, const void* d_o, int ldo, int do_compact, float* out,
                            const int32_t* cu_tok, const int64_t* out_off, int B, int H, int N /* max_N when cu_tok != NULL */, int nq,
                            int head_mean, int mode, float scale, int dtype, int flags, void* stream);
/* One step of an attention rollout on nr row vectors per sequence, without the attention map (additive: the ABI version stays 6):
 *   r_out[b][j][k] = a * r_in[b][j][k] + b_ * sum_{q < nq_b} r_in[b][j][q] * M_b[q][k]        j < nr, k < N_b
 *   mode PA_ATTN_ROLLOUT_ATTN: M = (1/H) sum_h P_h                          P_h = softmax(q_h k_h^T * scale), formed from qkv and lse
 *   mode PA_ATTN_ROLLOUT_CAM:  M = (1/H) sum_h max(P_h * (g_scale * G_h), 0)     G_h = d_o_h v_h^T
 * Every (32 queries x 32 keys) tile of P is formed as pa_attention_probs forms it, of G as pa_attention_probs_grad forms it, the heads
 * added in head order in f32 registers; the tile is multiplied by r_in's 32 entries and summed over its queries in registers, so no
 * element of M reaches memory.  a = b_ = 0.5 is a step of attention rollout (Abnar & Zuidema), a = b_ = 1 with CAM a step of the
 * gradient-weighted rollout (Chefer et al.); applied from the last block down to the first to one-hot start rows it gives those rows
 * of the rolled-out matrix.  qkv, ldqkv, lse, nq, scale, dtype, flags mean what they mean for pa_attention_probs; d_o, ldo, do_compact
 * what they mean for pa_attention_probs_grad (ATTN: d_o must be NULL, do_compact 0).  Query rows at or behind nq_b = min(nq, N_b)
 * contribute exactly nothing, key columns at or behind N_b are neither summed nor written.
 *   r_in, r_out: f32, nr * total_tok floats each that share no float (PA_EINVAL).  cu_tok == NULL: [B][nr][N], total_tok = B * N.  cu_tok != NULL: packed sequences as in
 *     pa_attention_fwd_varlen, N = max_N, total_tok = cu_tok[B]; sequence b's block is (nr, N_b) at float offset nr * cu_tok[b].  No
 *     row of a neighbour and none at or behind cu_tok[B] is read.  1 <= nr <= PA_ATTN_ROLLOUT_MAX_ROWS.
 *   slices: 0 = the query tiles are cut into S slices chosen from B, N and the device's CU count; > 0 = that many (capped at the
 *     number of query tiles; tests, A/B).  Each slice's partial rows go to `ws` and a finishing kernel adds them in slice order; S = 1
 *     (always so for nq <= 32) finishes in the one launch.  ws: pa_attention_rollout_ws_floats(same arguments) floats, may be NULL
 *     when that is 0.  No atomics: launches on the same inputs are bit-identical, and a sequence's result depends on its own inputs
 *     and the number of query tiles per slice only.
 *   PA_EINVAL: ldqkv < 3*H*64, or (with d_o) ldo < H*64. */
#define PA_ATTN_ROLLOUT_ATTN 0
#define PA_ATTN_ROLLOUT_CAM 1
#define PA_ATTN_ROLLOUT_MAX_ROWS 4
int64_t pa_attention_rollout_ws_floats(int64_t total_tok, int B, int N /* max_N when packed */, int nq, int nr, int slices);
int pa_attention_rollout(const void* qkv, int ldqkv, const float* lse, const void* d_o, int ldo, int do_compact, const float* r_in,
                         float* r_out, float* ws, const int32_t* cu_tok, int64_t total_tok, int B, int H,
                         int N /* max_N when cu_tok != NULL */, int nq, int nr, int mode, int slices, float a, float b_, float g_scale,
                         float scale, int dtype, int flags, void* stream);
/* number of floats of pa_attention_bwd's `delta` workspace */
int64_t pa_attention_bwd_ws_floats(int B, int H, int nq);
/* dqkv[B*N][3*H*64] from d_o[B*nq][H*64]; lse from the forward; delta: f32 workspace of pa_attention_bwd_ws_floats()
 * (per-query scalars the dQ kernel hands to the dK/dV kernel: -rowsum(dO*O), then -lse*log2 e).  The K and V thirds
 * of dqkv are written for all N tokens, the Q third only for rows q < nq (the caller zeroes the rest: pa_zero2d).
 * PA_EINVAL: ldqkv or lddqkv < 3*H*64, ldo < H*64. */
int pa_attention_bwd(const void* qkv, int ldqkv, const void* o, const void* d_o, int ldo,
                     const float* lse, float* delta, void* dqkv, int lddqkv, int B, int H, int N, int nq,
                     float scale, int dtype, int flags, void* stream);
/* ---- attention dropout (additive: the ABI version stays 6) ----
 * Dropout on the attention probabilities (the reference's attn_drop, models/passt.py:343-361) inside the fused forward and backward.
 * The mask is a pure function of a 64-bit seed and the element's position (csrc/pa_dropout.h).  t = round(256 p), 1 <= t <= 255: the
 * rate actually applied is p_eff = t / 256, keep = 1 - p_eff, kept probabilities are scaled by 1 / keep.  Element (site, s = b*H + h,
 * query q, key k), q and k the indices inside the sequence:
 *     R    = philox4x32_10(counter = (k >> 2, q >> 2, s, site), key = (seed[0], seed[1]))   (multipliers D2511F53 / CD9E8D57,
 *     byte = (R[q & 3] >> (8 * (k & 3))) & 0xff                                               key increments 9E3779B9 / BB67AE85)
 *     kept <=> byte >= t
 * site: the caller's name for the dropout site (the block index; values >= 65536 are reserved).
 * pa_attention_fwd_dropout: pa_attention_fwd's arguments and layouts (nq < N included) plus seed (TWO words in DEVICE memory: no host
 *   value enters the kernel, the launch can be captured in a graph), site and t.  lse and the row sum are those of the undropped
 *   softmax, bit-identical to pa_attention_fwd on the same operands; a dropped probability is selected to zero in front of the P V
 *   product and o = acc / (l * keep): a row whose keys are all dropped is exactly 0.
 * pa_attention_bwd_dropout: pa_attention_bwd's arguments plus the same three; o and lse from pa_attention_fwd_dropout with the same
 *   seed / site / t.  With D = kept / keep: dP = D (dO V^T), dS = P (dP - delta), delta = rowsum(dO o) from the stored o,
 *   dV = (P D)^T dO, dQ / dK from dS (a dropped element has dS = -P delta, not 0).  Always the dQ + dK/dV kernel pair; the
 *   PA_ATTN_BWD_* form flags are accepted and ignored, the result is bit-identical whichever are given.  Workspace and the Q third
 *   of rows q >= nq as for pa_attention_bwd.
 * PA_EINVAL before anything is launched: seed == NULL, t outside 1..255, and everything the plain entries refuse.  The packed
 * (_varlen) entries have their dropout form below (pa_attention_fwd_varlen_dropout / pa_attention_bwd_varlen_dropout).
 * pa_attention_dropout_mask: HOST only, touches no device: keep_out[(s*nq + q)*N + k] = 1 (kept) or 0 for s < BH, q < nq, k < N,
 *   from the same rule the kernels compile.  PA_EINVAL: keep_out == NULL, BH / nq / N <= 0, nq > N, t outside 1..255. */
int pa_attention_fwd_dropout(const void* qkv, int ldqkv, void* o, int ldo, float* lse, int B, int H, int N, int nq, float scale, int dtype,
                             int flags, const uint32_t* seed, uint32_t site, int t, void* stream);
int pa_attention_bwd_dropout(const void* qkv, int ldqkv, const void* o, const void* d_o, int ldo, const float* lse, float* delta,
                             void* dqkv, int lddqkv, int B, int H, int N, int nq, float scale, int dtype, int flags,
                             const uint32_t* seed, uint32_t site, int t, void* stream);
int pa_attention_dropout_mask(uint32_t seed0, uint32_t seed1, uint32_t site, int BH, int nq, int N, int t, uint8_t* keep_out);
/* Backward over PACKED sequences of different lengths: the backward of pa_attention_fwd_varlen, same cu_tok / max_N / nq meaning, same
 * layouts.  nq >= max_N: o / d_o are packed like qkv's rows and lse is [H][cu_tok[B]]; nq < max_N (the last block's nq = 2): o / d_o /
 * lse are compact as in pa_attention_bwd, o[(b*nq + q)][H*64], lse[(b*H + h)*nq + q].  ws: f32 workspace of
 * pa_attention_bwd_varlen_ws_floats(cu_tok[B], B, H, nq) floats (enough for either layout); the dQ kernel leaves the two planes
 * -rowsum(dO*O) and -lse*log2 e in it, in lse's layout (plane pitch H * cu_tok[B], resp. B * H * nq), for the dK/dV kernel.
 * Every row [0, cu_tok[B]) of dqkv is written in all three thirds (with nq < max_N the Q third of the rows q >= nq is written as zero:
 * no pa_zero2d by the caller) and nothing at or behind row cu_tok[B].  Always the dQ + dK/dV kernel pair -- the single pass needs one
 * N <= 512 for the whole launch; the PA_ATTN_BWD_* flags are accepted and ignored.  cdiv(nq, 128) query blocks and cdiv(max_N, 128)
 * key blocks are launched per (sequence, head); those a short sequence does not have return before their first memory access, and
 * tail tiles (K / V as well as Q / dO) are clamped to the sequence's own last row: no row of a neighbour is read.  Equal lengths
 * reproduce pa_attention_bwd(..., PA_ATTN_BWD_TWO_PASS) bit for bit.  PA_EINVAL: ldqkv or lddqkv < 3*H*64, ldo < H*64. */
int64_t pa_attention_bwd_varlen_ws_floats(int64_t total_tokens, int B, int H, int nq);
int pa_attention_bwd_varlen(const void* qkv, int ldqkv, const void* o, const void* d_o, int ldo, const float* lse, float* ws,
                            void* dqkv, int lddqkv, const int32_t* cu_tok, int B, int H, int max_N, int nq, float scale, int dtype,
                            int flags, void* stream);
/* ---- attention dropout on PACKED sequences (additive: the ABI version stays 6) ----
 * pa_attention_fwd_varlen / pa_attention_bwd_varlen with the dropout of pa_attention_fwd_dropout / pa_attention_bwd_dropout: the packed
 * entries' arguments, layouts (nq >= max_N: packed o / d_o and lse[H][cu_tok[B]]; nq < max_N: the compact form), workspace
 * (pa_attention_bwd_varlen_ws_floats) and writes, plus seed (two words in device memory), site and t with the meaning above.  The mask
 * rule is unchanged; for element (site, s, q, k) of packed sequence b, s = b*H + h with b the sequence's index in the batch, and q, k
 * are the positions INSIDE the sequence (0 .. N_b - 1), not token rows of the packed buffer.  The rule does not depend on N, so
 * sequence b gets bit for bit the mask -- and, the tile loop being the same, the o / lse / dqkv -- that pa_attention_fwd_dropout /
 * pa_attention_bwd_dropout give sequence b of a batch of B >= b + 1 sequences of N_b tokens under the same seed / site / t;
 * pa_attention_dropout_mask(seed0, seed1, site, (b + 1)*H, nq_b, N_b, t, .) restates it in its planes s = b*H .. b*H + H - 1.  lse is
 * that of the undropped softmax, bit-identical to pa_attention_fwd_varlen's on the same operands.  The backward is always the dQ + dK/dV
 * kernel pair (PA_ATTN_BWD_* form flags accepted and ignored).
 * PA_EINVAL before anything is launched: seed == NULL, t outside 1..255, site >= 65536, and everything pa_attention_fwd_varlen /
 * pa_attention_bwd_varlen refuse. */
int pa_attention_fwd_varlen_dropout(const void* qkv, int ldqkv, void* o, int ldo, float* lse, const int32_t* cu_tok, int B, int H,
                                    int max_N, int nq, float scale, int dtype, int flags, const uint32_t* seed, uint32_t site, int t,
                                    void* stream);
int pa_attention_bwd_varlen_dropout(const void* qkv, int ldqkv, const void* o, const void* d_o, int ldo, const float* lse, float* ws,
                                    void* dqkv, int lddqkv, const int32_t* cu_tok, int B, int H, int max_N, int nq, float scale,
                                    int dtype, int flags, const uint32_t* seed, uint32_t site, int t, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch embedding + positional terms + Patchout: PatchEmbed.forward (models/passt.py:318-328) and
 * PaSST.forward_features :508-564 (K10-K14).  Gather-first: only the patches that survive
 * structured/unstructured Patchout are embedded.
 *
 * Argument checks of every entry of this section, in this order, and NOTHING is launched or written before all have passed:
 *   1. NULL pointers and scalar ranges                                   PA_EINVAL
 *   2. dtype (PA_F32 / PA_BF16)                                          PA_EINVAL
 *   3. pointer alignment, where the entry states one                     PA_EINVAL
 *   4. size limits (P * P > 1024, Np above the grid, int32 indexing)     PA_EUNSUPPORTED
 * Index ranges.  Index arrays live in device memory and the host cannot see them.  UNCHECKED, the caller's duty -- an index out of
 * range reads or writes out of bounds: patch_f[p] in [0, Fpe) / [0, Fg), patch_t[p] in [0, Tg) and toff + patch_t[p] < Tpe in
 * pa_patch_gather, pa_patch_pos_table and pa_patch_bwd; cu_tok ascending with cu_tok[B] = M; toff[b] + column < Tpe for every
 * named slot of pa_patch_bwd_rows.  TOLERATED by the kernels: pa_patch_gather_varlen reads 0 for a coordinate outside x (and for a
 * row_clip outside [0, B)); pa_patch_input_bwd ignores (patch_f, patch_t) pairs outside the grid; the slot table of the two _rows
 * entries may hold anything, an entry outside [0, M) counts as -1.  pa_patch_pos_table_varlen clamps row_t / row_f to the last
 * embedding column: that is a memory-safety net, NOT a contract -- the table row of an out-of-range position is unspecified, and the
 * backward entries do not mirror the clamp (they would drop such a row from d_time_pos / d_freq_pos).
 * Alignment.  x, cols, the tables and every parameter gradient are accessed element by element: no requirement beyond the
 * element's own.  The vector accesses and what they need are stated per entry below (pa_patch_bwd, the three folds).
 * ------------------------------------------------------------------------------------------ */
/* im2col of the kept patches: x[B][1][F][T] f32 -> cols[B*Np][P*P] (dtype).
 * patch_f[Np], patch_t[Np]: grid coordinates (frequency row, time column) of kept patch p.
 * PA_EINVAL: F < P, T < P, a non-positive stride, B, Np or P. */
int pa_patch_gather(const float* x, int B, int F, int T, const int32_t* patch_f,
                    const int32_t* patch_t, int Np, int P, int fstride, int tstride, void* cols,
                    int dtype, void* stream);
/* table[p][D] = bias + time_pos[:, toff + patch_t[p]] + freq_pos[:, patch_f[p]]   (f32)
 * time_pos is [D][Tpe], freq_pos is [D][Fpe] (the reference's (1,D,1,Tpe)/(1,D,Fpe,1) params).
 * in f32 as (bias + time_pos) + freq_pos.  Also writes the two prefix tokens: tok[b][0] = cls + npe[0], tok[b][1] = dist + npe[1]
 * (tok is [B][Ntok][D]; no other row of it is touched).  PA_EINVAL: non-positive Np, D, B, Tpe or Fpe, Ntok < 2. */
int pa_patch_pos_table(const float* bias, const float* time_pos, int Tpe, const float* freq_pos,
                       int Fpe, const int32_t* patch_f, const int32_t* patch_t, int Np, int toff,
                       int D, float* table, const float* cls, const float* dist, const float* npe,
                       float* tok, int B, int Ntok, void* stream);
/* backward of the above given dtok[B][Ntok][D] f32: gsum[Ntok][D] = sum_b dtok (ws), then
 * d_cls, d_dist, d_npe[2][D], d_bias[D], d_time_pos[D][Tpe], d_freq_pos[D][Fpe] (all overwritten
 * or accumulated), and dcols_src: the patch rows of dtok compacted to [B*Np][D] (dtype) for the
 * weight-gradient GEMM.  gsum and the six parameter gradients all NULL: only dpatch is produced (frozen network, where dpatch
 * feeds the input-gradient GEMM of pa_patch_input_bwd).  Deterministic (no atomics; the summation order is fixed but unspecified).
 * PA_EINVAL: non-positive B, Np, D, Tpe or Fpe, Ntok < Np + 2, only some of the seven NULL, an unknown dtype -- refused before
 * anything is launched -- and dtok, gsum or dpatch off 16-byte alignment (16-byte vectors of all three). */
int pa_patch_bwd(const float* dtok, int B, int Ntok, int D, const int32_t* patch_f,
                 const int32_t* patch_t, int Np, int toff, int Tpe, int Fpe, float* gsum,
                 float* d_cls, float* d_dist, float* d_npe, float* d_bias, float* d_time_pos,
                 float* d_freq_pos, int accumulate, void* dpatch, int dtype, void* stream);
/* gradient w.r.t. the input spectrogram: the fold (col2im) of the kept patches, mirror image of pa_patch_gather.
 * dcols[B*Np][P*P] (dtype) = dpatch[B*Np][D] . W[D][P*P] (one pa_gemm_nt, PA_EPI_STORE, with the transposed conv weight) ->
 * dx[B][1][F][T] f32 with dx[b][f][t] = sum over the kept patches p that cover the pixel of dcols[b*Np+p][(f - patch_f[p]*fstride)*P +
 * (t - patch_t[p]*tstride)].  EVERY element of dx is written: a pixel no kept patch covers gets 0 (dropped Patchout patches, the
 * strip behind the last patch row / column, the frames behind the time cut, the gaps of a stride larger than P).  Gather form: one
 * output pixel adds its <= ceil(P/fstride) * ceil(P/tstride) patches in a fixed order (frequency row, then time column), no
 * atomics -- the result does not depend on the launch geometry.  grid_ws: int32 workspace of pa_patch_input_bwd_ws_ints() entries;
 * the call builds the grid -> slot table in it ([(F-P)/fstride+1][(T-P)/tstride+1], -1 = no kept patch there); (patch_f, patch_t)
 * pairs must be distinct, pairs outside the grid are ignored.  Spectrogram only: there is no gradient w.r.t. a waveform.
 * Alignment (this entry and its _varlen and _rows forms): dx 16-byte aligned (one 16-byte store per four elements of the flat dx),
 * dcols 4-byte aligned (bf16 dcols are read in pairs where P and the offset into the patch row are even); PA_EINVAL otherwise. */
int64_t pa_patch_input_bwd_ws_ints(int F, int T, int P, int fstride, int tstride);
int pa_patch_input_bwd(const void* dcols, int dtype, int B, int Np, const int32_t* patch_f, const int32_t* patch_t, int P,
                       int fstride, int tstride, int F, int T, int32_t* grid_ws, float* dx, void* stream);
/* Packed batch of clips of different lengths (eval forward of PaSST.forward(x, lengths), models/passt.py:513-526 per clip).  The token
 * matrix has M = sum_b (2 + Np_b) rows, clip after clip, each clip's cls and dist rows first.  Per token row r three int32 arrays
 * IN DEVICE MEMORY: row_clip[r] (row of x), row_f[r] / row_t[r] = grid coordinates of the patch, or row_f[r] = -1 for a prefix row with
 * row_t[r] = 0 (cls) / 1 (dist).
 * pa_patch_gather_varlen: x[B][1][F][T_max] f32 (clips left-aligned, anything behind a clip's own frames is never addressed by its
 *   rows) -> cols[M][P*P] (dtype), im2col of the row's patch; a prefix row is all zeros.  Coordinates outside x read as 0.
 * pa_patch_pos_table_varlen: table[M][D] f32 = bias + time_pos[:, row_t] + freq_pos[:, row_f] (time offset 0: eval, :519-521), and
 *   on a prefix row cls + npe[0] / dist + npe[1] -- the rows cu_tok[b] + {0, 1} of the packed matrix.
 * One pa_gemm_nt(cols, W, PA_EPI_RESID, resid = table, row_mod = 0) then writes all M token rows (a prefix row is 0 * W + table). */
int pa_patch_gather_varlen(const float* x, int B, int F, int T_max, const int32_t* row_clip, const int32_t* row_f,
                           const int32_t* row_t, int M, int P, int fstride, int tstride, void* cols, int dtype, void* stream);
int pa_patch_pos_table_varlen(const float* bias, const float* time_pos, int Tpe, const float* freq_pos, int Fpe,
                              const int32_t* row_f, const int32_t* row_t, int M, int D, float* table, const float* cls,
                              const float* dist, const float* npe, void* stream);
/* Backward of the packed patch stage (eval: no Patchout).  The packed token matrix is regular per clip -- cls, dist, then Fg x T_eff[b]
 * patches in frequency-major order with T_eff[b] = (cu_tok[b+1] - cu_tok[b] - 2) / Fg -- so the row of patch (f, t) of clip b is
 * cu_tok[b] + 2 + f * T_eff[b] + t and both entry points need cu_tok (B + 1 int32 in device memory) only.
 * pa_patch_input_bwd_varlen: the fold.  dcols[M][P*P] (dtype) = dtok[M][D] . W[D][P*P] over ALL M rows (one pa_gemm_nt; the rows under
 *   the prefix tokens are never read here) -> dx[B][1][F][T_max] f32, Fg = (F - P) / fstride + 1.  Gather form as pa_patch_input_bwd:
 *   one thread per four consecutive elements, the covering patches added in (frequency row, time column) order, no atomics.  EVERY
 *   element of dx is written; it is exactly 0 at and behind frame (T_eff[b] - 1) * tstride + P of clip b (the clip's own end, the
 *   time cut) and behind the last patch row.
 * pa_patch_bwd_varlen: d_cls, d_dist, d_npe[2][D], d_bias[D], d_time_pos[D][Tpe], d_freq_pos[D][Fpe] (overwritten or accumulated)
 *   from dtok[M][D] f32, M = cu_tok[B], Fg = Fpe.  Deterministic: a slot's rows are enumerated clip after clip in a fixed order, no
 *   atomics.  All six NULL (frozen network): nothing is launched.  (The patch weight gradient is one weight-gradient GEMM of dtok
 *   against the packed cols: their prefix rows are zero.) */
int pa_patch_input_bwd_varlen(const void* dcols, int dtype, const int32_t* cu_tok, int B, int P, int fstride, int tstride, int F,
                              int T_max, float* dx, void* stream);
int pa_patch_bwd_varlen(const float* dtok, int M, int D, const int32_t* cu_tok, int B, int Tpe, int Fpe, float* d_cls, float* d_dist,
                        float* d_npe, float* d_bias, float* d_time_pos, float* d_freq_pos, int accumulate, void* stream);
/* Backward of the packed patch stage WITH Patchout (training on a packed batch: every clip keeps its own patches and, in front of a
 * time embedding longer than the clip, its own random offset into it, models/passt.py:513-553 per clip).  A row's grid position no
 * longer follows from its place in the clip, so both entry points walk a slot table IN DEVICE MEMORY: slot[B][Fg][Tg] int32 = the
 * packed row of the kept patch (f, t) of clip b, -1 where there is none (dropped, behind the clip's last column, behind the time cut);
 * Tg = the patch columns of the widest clip.  An entry outside [0, M) counts as -1.  The forward needs no new entry point:
 * pa_patch_gather_varlen takes the kept patches' coordinates per row, pa_patch_pos_table_varlen takes row_t + the clip's offset.
 * pa_patch_input_bwd_rows: the fold.  dcols[M][P*P] (dtype) -> dx[B][1][F][T_max] f32, Fg = (F - P) / fstride + 1.  Gather form as
 *   pa_patch_input_bwd: one output element adds the KEPT patches that cover it, found through the slot table, in (frequency row, time
 *   column) order, no atomics.  EVERY element of dx is written; it is exactly 0 where no kept patch covers it.
 * pa_patch_bwd_rows: d_cls, d_dist, d_npe[2][D], d_bias[D], d_time_pos[D][Tpe], d_freq_pos[D][Fpe] (overwritten or accumulated) from
 *   dtok[M][D] f32; cu_tok: B + 1 row offsets, toff: B time-embedding offsets (int32, device memory), Fg = Fpe.  Time position p
 *   collects grid column p - toff[b] of every clip b.  Deterministic: a positional slot enumerates its rows through the slot table
 *   in a fixed order (clip, then frequency row, then column), no atomics.  All six NULL (frozen network): nothing is launched. */
int pa_patch_input_bwd_rows(const void* dcols, int dtype, int M, const int32_t* slot, int B, int Tg, int P, int fstride, int tstride,
                            int F, int T_max, float* dx, void* stream);
int pa_patch_bwd_rows(const float* dtok, int M, int D, const int32_t* slot, const int32_t* cu_tok, const int32_t* toff, int B, int Tg,
                      int Tpe, int Fpe, float* d_cls, float* d_dist, float* d_npe, float* d_bias, float* d_time_pos, float* d_freq_pos,
                      int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Head: final norm on the two prefix tokens, their mean, head LayerNorm + Linear
 * (models/passt.py:570-574, 583-585, 463-464; K23-K24) and the BCE loss of the caller
 * (ex_audioset.py:184-186; K25).
 * ------------------------------------------------------------------------------------------ */
/* x[B][Ntok][D] f32 (last block output). feat[B][D], hn[B][D] (LN_1e-5(feat)), and saved
 * statistics stats[B][6] = (mean0, rstd0, mean1, rstd1, meanh, rstdh). */
int pa_head_pre_fwd(const float* x, int B, int Ntok, int D, const float* norm_g,
                    const float* norm_b, float eps_norm, const float* hg, const float* hb,
                    float eps_head, float* feat, float* hn, float* stats, void* stream);
/* logits[B][C] = hn[B][D] W[C][D]^T + b  (small f32 GEMM, any C) */
int pa_linear_f32_fwd(const float* x, const float* W, const float* b, float* y, int B, int C, int D,
                      void* stream);
/* dx[B][D] = dy[B][C] W[C][D]; dW[C][D] (+)= dy^T x; db[C] (+)= colsum(dy).  dW = db = NULL: dx only (frozen network). */
int pa_linear_f32_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW,
                      float* db, int accumulate, int B, int C, int D, void* stream);
/* backward of pa_head_pre_fwd: dhn[B][D] (+ optional dfeat[B][D]) -> dx[B][Ntok][D] (rows 0,1
 * written, all other rows ZEROED), and per-batch partials part[B][4][D] =
 * (d_hg, d_hb, d_norm_g, d_norm_b) to be column-summed by the caller with pa_colsum_f32. */
int pa_head_pre_bwd(const float* dhn, const float* dfeat, const float* x, const float* feat, int B,
                    int Ntok, int D, const float* norm_g, const float* hg, const float* stats, float* dx,
                    float* part, void* stream);
/* loss[0] = mean BCE-with-logits; dlogits = grad_scale * d loss / d logits.  ws: >= 1 + ceil(B*C/256) floats */
int pa_bce_fwd_bwd(const float* logits, const float* target, int B, int C, float grad_scale,
                   float* loss, float* dlogits, float* ws, void* stream);

/* ESC-50 caller (ex_esc50.py:159-165): loss[0] = mean_b [ lam_b CE(z_b, target_b) + (1-lam_b) CE(z_b, target2_b) ];
 * target2 / lam may be NULL (plain cross entropy).  Targets are class indices.  ws: >= B floats. */
int pa_ce_mixup_fwd_bwd(const float* logits, const int32_t* target, const int32_t* target2, const float* lam,
                        int B, int C, float grad_scale, float* loss, float* dlogits, float* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-step glue of the caller ("next" rows)
 * ------------------------------------------------------------------------------------------ */
/* ex_audioset.py:175-177 / helpers/mixup.py: out[b] = x[b]*lam[b] + x[perm[b]]*(1-lam[b]) */
int pa_mixup(const float* x, const int32_t* perm, const float* lam, float* out, int B,
             int64_t per_sample, void* stream);
/* Spectrogram mixup of a ragged batch (additive to ABI 6).  x, out: [B][rows][ldt] f32, clip b valid in its first lens[b] columns
 * of every row; lens (int32, clamped to [0, ldt] in the kernel), perm (int32, entries in [0, B)) and lam (f32) are device arrays of
 * B entries.  The mixed clip keeps its own length; its partner j = perm[b] is cut to it, or continued with the constant ``pad``
 * (the spectrogram of silence) when it is shorter -- pad_or_truncate at the spectrogram level:
 *   t <  lens[b]:  out[b][r][t] = x[b][r][t] * lam[b] + (t < lens[j] ? x[j][r][t] : pad) * (1 - lam[b])
 *   t >= lens[b]:  out[b][r][t] = 0.0f exactly
 * One streaming pass: 16-byte accesses where ldt % 4 == 0 and x and out are 16-byte aligned -- and, beyond that, wherever a clip is a
 * whole number of 16-byte groups (rows * ldt % 4 == 0, ldt >= 4: 128 mel rows of any frame count) -- a group that straddles lens[b],
 * lens[j] or a row's end being resolved per lane; 4-byte accesses otherwise.  What x holds at or behind a clip's own length is never used: such a
 * value is chosen away, not multiplied by zero, so a NaN or Inf there does not reach out.  Every element of out is written, nothing
 * else.  The arithmetic is one multiplication and one fused multiply-add, fmaf(x[b], lam, c * (1 - lam)), the same as pa_mixup's
 * 16-byte path: with every lens[b] == ldt and ldt % 4 == 0 the result equals pa_mixup(per_sample = rows * ldt) bit for bit.
 * PA_EINVAL, nothing launched: a NULL pointer, B, rows or ldt < 1, rows * ldt >= 2^31, or out == x (the partner's row is read while
 * other rows are written). */
int pa_mixup_varlen(const float* x, const int32_t* lens, const int32_t* perm, const float* lam, float pad, float* out, int B,
                    int rows, int ldt, void* stream);
/* Waveform-side augmentation of one batch, ahead of the front end.  What the reference's data
 * pipeline does per clip on CPU workers, in its order: gain (audioset/dataset.py:102-112, amp = 10^(dB/20)),
 * pad_or_truncate to L samples (:73-78), roll (:315-329: out[t] = in[(t - shift) mod L]) and waveform mixup
 * (MixupDataset.__getitem__ :123-137: both clips mean-centred, w = max(lam, 1 - lam), out = w a + (1 - w) b).
 * The random parameters are drawn by the caller (host RNG, reference order).
 *   x: [B][ldx] f32 raw clips; len[b] valid samples (NULL: ldx); amp[b] (NULL: 1); shift[b] (NULL: 0);
 *   partner[b] >= 0: mix clip b with clip partner[b] using lam[b]; < 0: not mixed (NULL: no mixing at all).
 *   out: [B][L] f32 (the (B, 1, L) batch the training step takes); ws: f32 workspace of B floats.
 * The reference's last `x - x.mean()` of a mix is omitted: the mean of two centred signals is f32 rounding
 * noise (< 1e-7 of the amplitude). */
int pa_wave_augment(const float* x, int B, int64_t ldx, const int32_t* len, const float* amp, const int32_t* shift,
                    const int32_t* partner, const float* lam, float* ws, float* out, int64_t L, void* stream);
/* The same augmentation of a ragged batch (additive to ABI 6): row b of out has n_b = olen[b] samples of its own, and every clip
 * gets what it would get alone -- pa_wave_augment run with L = n_b on the pair (b, partner[b]).  "Clip c as row b sees it" is gain,
 * pad_or_truncate(n_b), roll(shift[c]), in that order:
 *   m            = min(len[c], n_b)
 *   s(t)         = (t - shift[c]) mod n_b                       true modulo: any sign, |shift| may exceed n_b
 *   item(c|b)[t] = s(t) < m ? x[c][s(t)] * amp[c] : 0           0 <= t < n_b
 *   mean(c|b)    = (amp[c] / n_b) * sum_{s < m} x[c][s]
 *   not mixed (partner[b] < 0, or partner == NULL):  out[b][t] = item(b|b)[t]
 *   mixed, p = partner[b], l = max(lam[b], 1 - lam[b]):
 *                out[b][t] = (item(b|b)[t] - mean(b|b)) * l + (item(p|b)[t] - mean(p|b)) * (1 - l)
 *   n_b <= t < L:  out[b][t] = 0.0f exactly
 * The partner is cut to n_b or continued with zeros, rolled by ITS shift modulo n_b and centred by ITS mean over n_b samples (on a
 * ragged batch a partner's mean depends on who mixes it in, so a mixed row has two means of its own).  partner[b] == b is legal; a
 * partner's item is always its unmixed item (out is never an input); n_b = 0 gives a zero row.  As in pa_wave_augment the
 * reference's last `x - x.mean()` is omitted.
 *   x [B][ldx] f32; len (NULL: ldx), olen, shift (NULL: 0), partner (NULL: nothing mixed) int32 and amp (NULL: 1), lam f32 are DEVICE
 *   arrays of B entries.  len is clamped to [0, ldx] and olen to [0, L] in the kernel; a partner[b] >= B is taken as "not mixed".
 *   x[c][s] with s >= len[c] or s >= n_b is never read: a value there is chosen away, not multiplied by zero.
 *   out [B][ldo] f32, ldo >= L: exactly out[b][0:L) is written for every row.  ws: f32 workspace of 2 * B floats (the two means of
 *   every mixed row; needed with partner only).
 * Two launches with a partner array (means: one 1024-thread block per mixed row and operand, each summing in pa_wave_augment's
 * order -- thread i takes samples i, i + 1024, ..., then two 64-lane butterflies; unmixed rows cost nothing), one without.  The
 * mix pass resolves every wrap once per row (shift mod n_b), so a roll is two contiguous source runs and no sample pays a division;
 * sample indices are 32-bit; 16-byte stores from each row's first 16-byte boundary on, 4-byte stores on the at most three elements
 * in front and behind, decided per row, so any ldo and any out pointer are legal.  Arithmetic per mixed sample: x * amp, the two
 * subtractions, (item(p|b) - mean) * (1 - l), then ONE fused multiply-add -- five roundings, none of them left to the compiler.
 * PA_EINVAL, nothing launched: x, out or olen NULL; B, ldx or L < 1; B > 65535; L > 2^31 - 1; ldo < L; partner without lam and ws;
 * out == x. */
int pa_wave_augment_varlen(const float* x, int B, int64_t ldx, const int32_t* len, const int32_t* olen, const float* amp,
                           const int32_t* shift, const int32_t* partner, const float* lam, float* ws, float* out, int64_t ldo,
                           int64_t L, void* stream);
/* Device-impulse-response augmentation, the first branch of pydub_augment (audioset/dataset.py:103-112, same body in esc50 /
 * fsd50k / openmic): scipy.signal.convolve(waveform, ir, 'full') with one IR of a bank, then pad_or_truncate to L.  Causal, no
 * delay compensation; the tail behind the clip is kept, up to L.  Overlap-save FFT tiles held in registers and LDS (ir_conv.hip);
 * its output and len_out are the raw clips and lengths pa_wave_augment takes.  Additive to ABI 6.
 *
 * pa_ir_conv_plan: host only.  The transform geometry used for a bank whose longest IR has max_taps taps (1..PA_IR_MAX_TAPS):
 *   *fft_n points per tile (4096 up to 1024 taps, 16384 above), *hop = new output samples per tile (fft_n - max_taps + 1 rounded
 *   down to a multiple of 64).  Either pointer may be NULL.  PA_EINVAL outside the range.
 * pa_ir_bank_floats: host only.  Size of `spectra` in floats (0 for arguments out of range).
 * pa_ir_bank_prepare: once per bank and device.  irs [n_ir][ld_ir] f32, row i valid for ir_len[i] taps (NULL: ld_ir), the rest of
 *   the row never read.  ld_ir IS the bank's max_taps (1..PA_IR_MAX_TAPS): it fixes the geometry, and the same value goes to
 *   pa_wave_ir_convolve.  spectra (DEVICE memory, 8-byte aligned, pa_ir_bank_floats(n_ir, ld_ir) floats) is opaque: the
 *   twiddle table of the transform followed by the IRs' spectra in the order the convolve kernel consumes them.  One host-to-
 *   device copy of the table is enqueued on `stream` ahead of the launch, so this entry is not for a captured graph.
 * pa_wave_ir_convolve:
 *   out[b][t] = sum_k h_b[k] * x[b][t-k]   for 0 <= t < len_out[b] = min(len[b] + taps_b - 1, L);   out[b][t] = 0 for len_out[b] <= t < L
 *   x [B][ldx] f32, len[b] valid samples (clamped to 0..ldx; NULL: ldx); x[b][len[b]:] is never read.  h_b = IR ir_idx[b] of the
 *   bank, taps_b = ir_len[ir_idx[b]].  ir_idx[b] < 0 (or ir_idx == NULL): out[b][:min(len[b], L)] is a bit-exact copy of x, zeros
 *   behind, len_out[b] = min(len[b], L).  ir_idx[b] >= n_ir or a tap count outside 1..max_taps in the DEVICE arrays never causes
 *   an access outside the buffers: such a clip is a pass-through as well.  An empty clip (len[b] = 0) gives zeros, len_out[b] = 0.
 *   out [B][ldo] f32, ldo >= L; only out[b][0:L) is written.  len_out [B] int32 may be NULL.  A row's result does not depend on
 *   B or on the row's position in the batch.
 *   PA_EINVAL (before any launch): x, out or spectra NULL; B, L, ldx or n_ir <= 0; B > 65535; L > 2^31 - 1; ldo < L; max_taps
 *   outside 1..PA_IR_MAX_TAPS; ir_idx without ir_len; spectra not 8-byte aligned. */
#define PA_IR_MAX_TAPS 8192
int pa_ir_conv_plan(int max_taps, int* fft_n, int* hop);
int64_t pa_ir_bank_floats(int n_ir, int max_taps);
int pa_ir_bank_prepare(const float* irs, int n_ir, int ld_ir, const int32_t* ir_len, float* spectra, void* stream);
int pa_wave_ir_convolve(const float* x, int B, int64_t ldx, const int32_t* len, const int32_t* ir_idx, const float* spectra,
                        const int32_t* ir_len, int n_ir, int max_taps, float* out, int64_t ldo, int64_t L, int32_t* len_out,
                        void* stream);
/* torch.optim.AdamW (ex_audioset.py:104-109) on one flat f32 parameter buffer */
int pa_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
             float beta2, float eps, float weight_decay, int step, void* stream);
/* The same update with the step's scalars in DEVICE memory: hyper = 7 floats [lr, beta1, beta2, eps, weight_decay,
 * 1 - beta1^step, sqrt(1 - beta2^step)] (pa_adamw_hyper fills a HOST array of 7 with exactly what pa_adamw computes from its
 * by-value arguments; the caller copies it to the device).  The launch's arguments are then the same every step, so it can be
 * part of a captured hipGraph (passt_amd.train.TrainStep(graph=True)). */
int pa_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* stream);
void pa_adamw_hyper(float lr, float beta1, float beta2, float eps, float weight_decay, int step, float* hyper7_host);
/* AdamW of one bucket of the flat buffers AND the GEMM-ready copies of its weight matrices in ONE launch (ABI 6): what
 * pa_adamw followed by pa_stage_weights produce -- parameters, moments and copies bit-identical -- without reading the updated
 * parameters back (torch.optim.AdamW, ex_audioset.py:104-109; the copies have no reference counterpart: AMP autocast casts the
 * weights per op).  `descs` (DEVICE memory, n_desc entries, in work-item order) lists every parameter of the bucket:
 *   offset      element offset of the parameter in p / g / m / v
 *   rows, cols  its shape as a row-major matrix (a parameter without copies: rows = 1, cols = numel)
 *   dst, dst_t  where non-NULL: the straight cast [rows][cols] and the transposed cast [cols][rows] of `dtype`, contiguous
 *   tile_begin  running count of work items: ceil(rows/64)*ceil(cols/64) tiles of 64x64 for a parameter with a copy,
 *               ceil(numel/4096) runs for one without;  total_items = their sum (= the grid).
 * hyper_dev == NULL: the step's scalars by value, as pa_adamw;  else the 7 device floats of pa_adamw_dev (by-value ones ignored). */
typedef struct pa_adamw_stage_desc {
    int64_t offset;
    void* dst;
    void* dst_t;
    int32_t rows, cols;
    int32_t tile_begin;
    int32_t reserved;
} pa_adamw_stage_desc;
int pa_adamw_stage(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, int n_desc, int total_items,
                   int dtype, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   const float* hyper_dev, void* stream);
/* Parameter groups (torch.optim.AdamW param_groups: layer-wise learning-rate decay, no weight decay on biases / norms / position
 * tables) in the same one launch per bucket.  `scales` (DEVICE memory, 8-byte aligned, n_desc pairs of floats, parallel to `descs`):
 * entry i is updated with lr * scales[2 i] and weight_decay * scales[2 i + 1], lr and weight_decay being the launch's own -- by value
 * or, with hyper_dev, the device row's, so a captured launch keeps following the schedule.  A pair of ones is bit-identical to
 * pa_adamw_stage; lr_scale = 0 leaves the parameter (and its copies' values) unchanged while its moments still advance.
 * pa_adamw_stage_groups: pa_adamw_stage with `scales`.  pa_adamw_groups: the plain form -- the same table, no copies written (dst /
 * dst_t are not looked at: every entry counts ceil(rows * cols / 4096) work items in tile_begin / total_items). */
int pa_adamw_stage_groups(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, const float* scales,
                          int n_desc, int total_items, int dtype, float lr, float beta1, float beta2, float eps, float weight_decay,
                          int step, const float* hyper_dev, void* stream);
int pa_adamw_groups(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, const float* scales, int n_desc,
                    int total_items, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    const float* hyper_dev, void* stream);
/* Global-norm gradient clipping and gradient accumulation (Lightning's trainer.gradient_clip_val / trainer.accumulate_grad_batches,
 * ex_audioset.py:36; torch.nn.utils.clip_grad_norm_) without a host sync.  Additive to ABI 6.
 *
 * pa_grad_norm_partials(n): host only; the number of f32 partial sums a span of n elements produces: ceil(n / 4096), a function of n
 *   alone (not of the grid, the CU count or the alignment); 0 for n <= 0.
 * pa_grad_accum_sumsq: ONE streaming pass over a span of n gradients.
 *   acc != NULL:      acc[i] = first ? g[i] : acc[i] + g[i] (one f32 addition; with `first` acc is never read: it may hold NaN)
 *   partials != NULL: partials[k] = sum of the squares of elements [4096 k, min(4096 (k + 1), n)) of the RESULT (acc, or g when acc is
 *                     NULL), pa_grad_norm_partials(n) floats.
 *   One workgroup per chunk, the order of the additions a function of the element's index in the chunk only: the same bits from run to
 *   run and for the same data at another address or alignment; no atomics, no finishing launch.  Every addend is >= 0, so a partial's
 *   relative error is at most gamma_24 = 24 u / (1 - 24 u), u = 2^-24.  16-byte accesses where g (and acc, which must then
 *   share g's misalignment) allow, a scalar head and tail otherwise; nothing outside [0, n) is read or written.
 *   PA_EINVAL: g NULL, n <= 0, acc and partials both NULL.
 * pa_clip_coef: one workgroup; out[0] = (float)sqrt(sum of the n_partials partials, in f64, fixed order) -- the total L2 norm;
 *   out[1] = the clip factor in f32 exactly as torch forms it: c = reciprocal(out[0] + 1e-6f) * max_norm (torch evaluates
 *   max_norm / tensor as tensor.reciprocal() * max_norm), factor = c > 1 ? 1 : c.  A NaN norm gives a NaN factor
 *   (clip_grad_norm_(error_if_nonfinite=False)); max_norm = +inf gives exactly 1.  PA_EINVAL: max_norm <= 0 or NaN, n_partials < 1.
 * pa_adamw_clip: pa_adamw (hyper_dev == NULL: scalars by value) / pa_adamw_dev (hyper_dev: the 7 device floats) with the factor.
 * pa_adamw_stage_clip: pa_adamw_stage / pa_adamw_stage_groups / pa_adamw_groups with the factor: `scales` may be NULL (no groups),
 *   table entries may omit their copies.
 *   gscale_dev: ONE device float; the gradient entering the update is g * *gscale_dev (one f32 multiplication).  The gradient buffer
 *   itself is NOT written: after a clipped step g (p.grad, TrainStep.flat_g) still holds the UNCLIPPED values -- on purpose, unlike
 *   torch's in-place clip_grad_norm_: it saves a 345 MB write per step.  gscale_dev == NULL and a factor of exactly 1.0f are
 *   bit-identical to the entries without it (parameters, both moments, both copies). */
int64_t pa_grad_norm_partials(int64_t n);
int pa_grad_accum_sumsq(const float* g, float* acc, int first, int64_t n, float* partials, void* stream);
int pa_clip_coef(const float* partials, int n_partials, float max_norm, float* out, void* stream);
int pa_adamw_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, const float* hyper_dev, const float* gscale_dev, void* stream);
int pa_adamw_stage_clip(float* p, const float* g, float* m, float* v, const pa_adamw_stage_desc* descs, const float* scales,
                        int n_desc, int total_items, int dtype, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int step, const float* hyper_dev, const float* gscale_dev, void* stream);
/* torch.optim.SGD lr only (ex_audioset.py:392 model_speed_test) */
int pa_sgd(float* p, const float* g, int64_t n, float lr, void* stream);
/* Stochastic weight averaging step on flat buffers (helpers/swa_callback.py:246-268, update_parameters + avg_fn):
 * num_averaged == 0: avg = p;  else avg += (p - avg) / (num_averaged + 1).  The caller increments the count. */
int pa_swa_update(float* avg, const float* p, int64_t n, int num_averaged, void* stream);

/* ------------------------------------------------------------------------------------------
 * Validation metrics (ex_audioset.py:245-291, ex_openmic.py:228-270): per-class average precision and ROC-AUC on the device,
 * sort-free, as exact integer rank counts per positive sample.  For one class, over the valid samples (P positives, Nn
 * negatives), with GEp_i / GEn_i = the positives / negatives whose score is >= that of positive i and GTn_i = the negatives
 * whose score is greater:
 *   AP  = (1 / P) sum_i GEp_i / (GEp_i + GEn_i)
 *   AUC = sum_i (2 (Nn - GEn_i) + (GEn_i - GTn_i)) / (2 P Nn)
 * which is what scikit-learn's average_precision_score / roc_auc_score return, ties included.
 *
 * pa_eval_append: one batch scores[B][C], target[B][C] (positive when > 0.5), mask[B][C] (valid when > 0.5; NULL = all valid)
 *   goes, transposed, into columns n0 .. n0 + B of the class-major buffers keys[C][capacity] (u32) and state[C][capacity] (u8).
 *   mode PA_EVAL_SIGMOID ranks the f32 1 / (1 + exp(-z)) of the logits, PA_EVAL_RAW the values as given.  The key is the score's
 *   bit pattern made order-preserving (-0 equals +0); the state is 0 excluded, 1 negative, 2 positive, 3 a valid sample whose
 *   score is NaN.  Any B, C >= 1 and any n0 with n0 + B <= capacity; columns outside n0 .. n0 + B are not touched.
 * pa_eval_rank: the first n columns of every class -> n_pos[C], n_neg[C], auc_num[C] (the AUC numerator above) as int64 and
 *   ap[C], auc[C] as f64.  P = 0: ap 0.0; P = 0 or Nn = 0: auc NaN; a class with a NaN-scored valid sample: ap and auc NaN
 *   (that sample is in neither count).  n = 0 is allowed.  The integers are exact; the f64 sum of the AP terms runs in a fixed order
 *   (sample order inside a run of 256 positives, the runs in order), so equal inputs give equal bits.  ws: pa_eval_ws_bytes(C, capacity) bytes, 16-byte aligned; 0 from the query = a
 *   shape the entry refuses (capacity >= 2^31, or C * ceil(capacity / 256) >= 2^31).  Nothing is read at or behind column n.
 * PA_EINVAL: NULL pointers (mask excepted), B or C < 1, n0 < 0, n < 0, n0 + B or n > capacity, an unknown mode. */
#define PA_EVAL_SIGMOID 0
#define PA_EVAL_RAW 1
int pa_eval_append(const float* scores, const float* target, const float* mask, int B, int C, int64_t n0, int64_t capacity, int mode,
                   uint32_t* keys, uint8_t* state, void* stream);
int64_t pa_eval_ws_bytes(int C, int64_t capacity);
int pa_eval_rank(const uint32_t* keys, const uint8_t* state, int C, int64_t n, int64_t capacity, void* ws, int64_t* n_pos,
                 int64_t* n_neg, int64_t* auc_num, double* ap, double* auc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sliding-window inference over long recordings (PaSST.forward_windows).  A window is (recording, first frame, frames) of a
 * recording longer than the time embedding; all windows of all recordings run as ONE packed batch, a window taking the place a
 * clip has in the packed entries above.  Three int32 arrays of W entries IN DEVICE MEMORY describe the windows: win_src[w] (row of
 * x), win_t0[w] (first frame, ANY value >= 0: no multiple of the stride, no alignment), win_len[w] (frames).
 * pa_patch_gather_windows: x[B][1][F][T_pitch] f32 (recordings left-aligned; T_pitch may be odd, nothing is assumed aligned) ->
 *   cols[M][P*P] (dtype): cols[r][i*P+j] = x[win_src[w]][row_f[r]*fstride+i][win_t0[w] + row_t[r]*tstride + j], w = row_win[r].
 *   row_win plays row_clip's role (cu_tok and the prefix rows index windows); row_f / row_t mean what they mean in
 *   pa_patch_gather_varlen, a prefix row (row_f < 0) is all zeros.  An element is read only if its frame lies in
 *   [win_t0[w], win_t0[w] + win_len[w]) -- what lies behind a window, and so behind a recording's length, is never addressed; an
 *   element outside it, outside x, or of a window / recording index outside its array reads as 0.  pa_patch_pos_table_varlen,
 *   the patch GEMM, the packed attention and the tail then run unchanged on the M rows.
 *   PA_EINVAL: NULL pointers, a size or stride < 1, an unknown dtype; PA_EUNSUPPORTED: P * P > 1024.
 * pa_window_pool: in[W][C] f32 (per-window rows), offsets[B + 1] int32 IN DEVICE MEMORY (recording b owns rows offsets[b] ..
 *   offsets[b + 1] - 1, ascending, offsets[0] = 0, offsets[B] = W) -> out[B][C] f32.  mode PA_POOL_MEAN: the rows are added in row
 *   order in f32 and divided by the recording's own count; PA_POOL_MAX: the maximum, started from the first row.  act
 *   PA_POOL_ACT_SIGMOID pools the f32 1 / (1 + exp(-z)) of pa_eval_append instead of the values.  No atomics, one thread per
 *   output: equal inputs give equal bits.  A recording with one window gets that row's values exactly.
 *   PA_EINVAL: NULL pointers, W, C or B < 1, an unknown mode or act, and B > W (some recording would be empty).  The offsets
 *   themselves are the caller's duty (the host cannot see them): rows outside [0, W) are not read, and a recording that is empty
 *   all the same gets NaN. */
#define PA_POOL_MEAN 0
#define PA_POOL_MAX 1
#define PA_POOL_ACT_NONE 0
#define PA_POOL_ACT_SIGMOID 1
int pa_patch_gather_windows(const float* x, int B, int F, int T_pitch, const int32_t* win_src, const int32_t* win_t0,
                            const int32_t* win_len, int W, const int32_t* row_win, const int32_t* row_f, const int32_t* row_t, int M,
                            int P, int fstride, int tstride, void* cols, int dtype, void* stream);
int pa_window_pool(const float* in, int W, int C, const int32_t* offsets, int B, int mode, int act, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Data-parallel exchange step: gradient all-reduce over RCCL / xGMI, one communicator per process (= per GPU).
 * Replaces Lightning's DDP plugin (ex_audioset.py:488-489 -> torch DDP: NCCL all-reduce of gradient buckets from
 * autograd hooks; mean of the per-rank gradients).  Here the caller owns the buckets: contiguous slices of its flat
 * gradient buffer, reduced IN PLACE (sum; the 1/world factor is folded into the loss gradient), launched as soon as a
 * block's gradients are complete (passt_amd.ddp.GradReducer drives it from the backward's callbacks).
 * RCCL is loaded at run time (dlopen); a process that never calls these functions does not need it.
 * ------------------------------------------------------------------------------------------ */
#define PA_COMM_ID_BYTES 128
/* rank 0: 128 opaque bytes (an ncclUniqueId) to hand to every rank out of band (file, socket, torch store ...) */
int pa_comm_unique_id(void* id_out);
/* every rank, after selecting its device (hipSetDevice / torch.cuda.set_device): blocks until all `world` ranks joined */
int pa_comm_init(const void* id, int rank, int world, void** comm_out);
/* buf[count] (dtype PA_F32 or PA_BF16) <- sum over ranks, in place, asynchronous and ordered on `stream` */
int pa_allreduce_bucket(void* comm, void* buf, int64_t count, int dtype, void* stream);
int pa_comm_destroy(void* comm);
/* What the communicator itself reports (ncclGetVersion / ncclCommCount / ncclCommUserRank / ncclCommCuDevice): the evidence
 * bench.py prints for an N > 1 run.  Any out pointer may be NULL; comm == NULL with only rccl_version asked returns the
 * version of the RCCL the library resolved (e.g. 22703 = 2.27.3). */
int pa_comm_info(void* comm, int* rccl_version, int* nranks, int* rank, int* device);
/* text of the last PA_ECOMM on the calling thread */
const char* pa_comm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* PASST_AMD_H */

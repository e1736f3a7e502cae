// Device-impulse-response augmentation (audioset/dataset.py:103-112: scipy.signal.convolve(waveform, ir, 'full') followed by
// pad_or_truncate): a long FIR convolution of every clip of a batch with one IR of a bank, as overlap-save FFT tiles.
//
// A direct form costs 2 K FLOP per output sample (B = 64, L = 320 000, K = 4096: 168 GFLOP per batch); an FFT tile costs a few
// hundred FLOP per sample and is bound by the 2 B L 4 bytes it moves.
//
// One workgroup = one PAIR of consecutive tiles of one clip: the IR is real, so tile 2p rides as the real part and tile 2p + 1
// as the imaginary part of ONE complex transform (conv(x1 + i x2, h) = conv(x1, h) + i conv(x2, h); no real-FFT split step).
// Geometry (pa_ir_conv_plan): N = 4096 points for banks up to 1024 taps, N = 16 384 above (up to PA_IR_MAX_TAPS = 8192);
// hop = (N - max_taps + 1) rounded down to 64, so every tile starts on a 256-byte boundary of its row.
//
// The transform keeps its N points in REGISTERS, 16 complex per thread (N / 16 threads), and uses the LDS only to regroup them
// between stages, real parts and imaginary parts one after the other: N + N / 16 floats = 17 KiB / 68 KiB per workgroup (two
// workgroups of the large size fit the CU's 160 KiB).  N = Q 16^3 (Q = 1, 4): a slot index is (q, a, b, c), q < Q, a b c < 16.
//   forward  (decimation in frequency): [Q = 4: radix-4 over q, twiddle W_N^(r kq)], radix-16 over a, twiddle W_4096^((16 b + c) k0),
//            radix-16 over b, twiddle W_256^(c k1), radix-16 over c.  The spectrum comes out digit-reversed: slot (kq, k0, k1, k2)
//            holds bin kq + Q (k0 + 16 k1 + 256 k2).
//   inverse  (decimation in time) runs the same steps backwards with conjugate twiddles and takes exactly that order, so nothing
//            is ever reordered; pa_ir_bank_prepare runs the same forward code on the IRs (1 / N folded in), so the pointwise
//            product happens in the registers the forward transform left the spectrum in.
// Twiddles are read from a table of W_N^i (float2, i < N) computed on the host in double precision; it is the head of `spectra`.
#include "pa_common.h"

#include <math.h>

#include <mutex>
#include <vector>

namespace {
using namespace pa;

constexpr int IR_SMALL_TAPS = 1024;      // banks up to this many taps use the 4096-point tile

template <int Q> struct IrGeo {
    static constexpr int N = 4096 * Q, T = 256 * Q, LDS_FLOATS = N + N / 16;
};

// which 16 slots a thread holds.  LQ: (q, top two bits of a) vary; LA / LB / LC: a / b / c varies
enum { LQ = 0, LA = 1, LB = 2, LC = 3 };
template <int LAY> __device__ __forceinline__ int ir_slot(int t, int j) {
    if constexpr (LAY == LQ) return j * 1024 + t;
    else if constexpr (LAY == LA) return (t >> 8) * 4096 + j * 256 + (t & 255);
    else if constexpr (LAY == LB) return (t >> 4) * 256 + j * 16 + (t & 15);
    else return t * 16 + j;
}
// LDS address of a slot: one pad float per 16 (s + (s >> 4)), so that the 16-float runs of LC and the 256-float strides of LB
// fall on distinct banks (64 x 4 B).  Written as (a term of t) + j * constant: the sixteen accesses of a thread share one
// address register and differ in the instruction's immediate offset
template <int LAY> __device__ __forceinline__ int ir_lds_base(int t) {
    if constexpr (LAY == LQ) return t + (t >> 4);
    else if constexpr (LAY == LA) return (t >> 8) * 4352 + (t & 255) + ((t & 255) >> 4);
    else if constexpr (LAY == LB) return (t >> 4) * 272 + (t & 15);
    else return t * 17;
}
template <int LAY> constexpr int ir_lds_step() { return LAY == LQ ? 1088 : LAY == LA ? 272 : LAY == LB ? 17 : 1; }

template <int FROM, int TO> __device__ __forceinline__ void ir_regroup(float (&re)[16], float (&im)[16], float* lds, int t) {
    float* src = lds + ir_lds_base<FROM>(t);
    const float* dst = lds + ir_lds_base<TO>(t);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) src[j * ir_lds_step<FROM>()] = re[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) re[j] = dst[j * ir_lds_step<TO>()];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) src[j * ir_lds_step<FROM>()] = im[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) im[j] = dst[j * ir_lds_step<TO>()];
}

// (r, i) *= -i (forward) / +i (inverse)
template <bool INV> __device__ __forceinline__ void ir_rot(float& r, float& i) {
    const float t = r;
    if constexpr (INV) { r = -i; i = t; } else { r = i; i = -t; }
}
template <bool INV> __device__ __forceinline__ void ir_cmul(float& r, float& i, float wr, float wi) {   // *= w (forward) / conj(w)
    const float a = r, b = i;
    if constexpr (INV) { r = fmaf(a, wr, b * wi); i = fmaf(b, wr, -(a * wi)); }
    else { r = fmaf(a, wr, -(b * wi)); i = fmaf(a, wi, b * wr); }
}
// 4-point DFT of elements i0..i3, results in place (output k at the place of input k)
template <bool INV> __device__ __forceinline__ void ir_radix4(float (&re)[16], float (&im)[16], int i0, int i1, int i2, int i3) {
    const float t0r = re[i0] + re[i2], t0i = im[i0] + im[i2], t1r = re[i0] - re[i2], t1i = im[i0] - im[i2];
    const float t2r = re[i1] + re[i3], t2i = im[i1] + im[i3];
    float t3r = re[i1] - re[i3], t3i = im[i1] - im[i3];
    ir_rot<INV>(t3r, t3i);
    re[i0] = t0r + t2r; im[i0] = t0i + t2i;
    re[i1] = t1r + t3r; im[i1] = t1i + t3i;
    re[i2] = t0r - t2r; im[i2] = t0i - t2i;
    re[i3] = t1r - t3r; im[i3] = t1i - t3i;
}
// 16-point DFT in registers, natural order in and out: n = 4 n1 + n0, k = k0 + 4 k1
template <bool INV> __device__ __forceinline__ void ir_dft16(float (&re)[16], float (&im)[16]) {
    constexpr float C1 = 0.92387953251128675613f, S1 = 0.38268343236508977173f, R2 = 0.70710678118654752440f;
    __builtin_amdgcn_sched_barrier(0);      // keep the table loads of the neighbouring steps out of the butterflies' registers
#pragma unroll
    for (int n0 = 0; n0 < 4; ++n0) ir_radix4<INV>(re, im, n0, 4 + n0, 8 + n0, 12 + n0);      // place 4 k0 + n0
    // W16^(n0 k0), W16 = exp(-2 pi i / 16)
    ir_cmul<INV>(re[5], im[5], C1, -S1);       // 1
    ir_cmul<INV>(re[6], im[6], R2, -R2);       // 2
    ir_cmul<INV>(re[7], im[7], S1, -C1);       // 3
    ir_cmul<INV>(re[9], im[9], R2, -R2);       // 2
    ir_rot<INV>(re[10], im[10]);               // 4
    ir_cmul<INV>(re[11], im[11], -R2, -R2);    // 6
    ir_cmul<INV>(re[13], im[13], S1, -C1);     // 3
    ir_cmul<INV>(re[14], im[14], -R2, -R2);    // 6
    ir_cmul<INV>(re[15], im[15], -C1, S1);     // 9
#pragma unroll
    for (int k0 = 0; k0 < 4; ++k0) ir_radix4<INV>(re, im, 4 * k0, 4 * k0 + 1, 4 * k0 + 2, 4 * k0 + 3);   // place 4 k0 + k1
    // place 4 k0 + k1 holds bin k0 + 4 k1: transpose the 4 x 4 (register renaming)
#pragma unroll
    for (int k0 = 0; k0 < 4; ++k0)
#pragma unroll
        for (int k1 = k0 + 1; k1 < 4; ++k1) {
            float t = re[4 * k0 + k1]; re[4 * k0 + k1] = re[4 * k1 + k0]; re[4 * k1 + k0] = t;
            t = im[4 * k0 + k1]; im[4 * k0 + k1] = im[4 * k1 + k0]; im[4 * k1 + k0] = t;
        }
    __builtin_amdgcn_sched_barrier(0);
}
// element j *= W_N^(base j) (conjugate for the inverse), j = 1..15
template <bool INV> __device__ __forceinline__ void ir_twiddle16(float (&re)[16], float (&im)[16], const float2* __restrict__ tw, int base) {
    // five at a time: all fifteen loads in flight at once cost 45 registers next to the 32 of the data
#pragma unroll
    for (int g = 1; g < 16; g += 5) {
        float2 w[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) w[j] = tw[(unsigned)(base * (g + j))];
#pragma unroll
        for (int j = 0; j < 5; ++j) ir_cmul<INV>(re[g + j], im[g + j], w[j].x, w[j].y);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// the Q = 4 outer stage in layout LQ: element j = (q or kq = j >> 2, m = j & 3), r = 1024 m + t
template <bool INV> __device__ __forceinline__ void ir_twiddle_q(float (&re)[16], float (&im)[16], const float2* __restrict__ tw, int t) {
#pragma unroll
    for (int g = 4; g < 16; g += 4) {
        float2 w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = tw[(unsigned)((j * 1024 + t) * (g >> 2))];
#pragma unroll
        for (int j = 0; j < 4; ++j) ir_cmul<INV>(re[g + j], im[g + j], w[j].x, w[j].y);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// forward: input in layout (Q == 4 ? LQ : LA), natural sample order; output in layout LC, digit-reversed bins
template <int Q> __device__ __forceinline__ void ir_fft_fwd(float (&re)[16], float (&im)[16], float* lds, const float2* __restrict__ tw, int t) {
    if constexpr (Q == 4) {
#pragma unroll
        for (int m = 0; m < 4; ++m) ir_radix4<false>(re, im, m, 4 + m, 8 + m, 12 + m);
        ir_twiddle_q<false>(re, im, tw, t);
        ir_regroup<LQ, LA>(re, im, lds, t);
    }
    ir_dft16<false>(re, im);
    ir_twiddle16<false>(re, im, tw, Q * (t & 255));
    ir_regroup<LA, LB>(re, im, lds, t);
    ir_dft16<false>(re, im);
    ir_twiddle16<false>(re, im, tw, Q * 16 * (t & 15));
    ir_regroup<LB, LC>(re, im, lds, t);
    ir_dft16<false>(re, im);
}
// inverse (unscaled): input in layout LC, digit-reversed bins; output in layout (Q == 4 ? LQ : LA), natural sample order
template <int Q> __device__ __forceinline__ void ir_fft_inv(float (&re)[16], float (&im)[16], float* lds, const float2* __restrict__ tw, int t) {
    ir_dft16<true>(re, im);
    ir_regroup<LC, LB>(re, im, lds, t);
    ir_twiddle16<true>(re, im, tw, Q * 16 * (t & 15));
    ir_dft16<true>(re, im);
    ir_regroup<LB, LA>(re, im, lds, t);
    ir_twiddle16<true>(re, im, tw, Q * (t & 255));
    ir_dft16<true>(re, im);
    if constexpr (Q == 4) {
        ir_regroup<LA, LQ>(re, im, lds, t);
        ir_twiddle_q<true>(re, im, tw, t);
#pragma unroll
        for (int m = 0; m < 4; ++m) ir_radix4<true>(re, im, m, 4 + m, 8 + m, 12 + m);
    }
}

__device__ __forceinline__ int64_t ir_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// spectra = [N float2 twiddles][n_ir][16][T] float2: element j of thread t of the forward transform's output, times 1 / N
template <int Q> __global__ __launch_bounds__(256 * Q) void ir_bank_kernel(const float* __restrict__ irs, int ld_ir,
                                                                           const int32_t* __restrict__ ir_len, float* __restrict__ spectra) {
    constexpr int N = IrGeo<Q>::N, T = IrGeo<Q>::T, IN = Q == 4 ? LQ : LA;
    extern __shared__ float lds[];
    const int t = threadIdx.x, i = blockIdx.x;
    int taps = ir_len ? ir_len[i] : ld_ir;
    if (taps < 1 || taps > ld_ir) taps = 0;                 // such an IR is never applied (pass-through): a zero spectrum
    const float* h = irs + (int64_t)i * ld_ir;
    float re[16], im[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int n = ir_slot<IN>(t, j);
        re[j] = n < taps ? h[n] : 0.f;
        im[j] = 0.f;
    }
    const float2* tw = (const float2*)spectra;
    ir_fft_fwd<Q>(re, im, lds, tw, t);
    float2* H = (float2*)spectra + N + (int64_t)i * N;
    constexpr float inv_n = 1.0f / (float)N;
#pragma unroll
    for (int j = 0; j < 16; ++j) H[j * T + t] = float2{re[j] * inv_n, im[j] * inv_n};
}

template <int Q> __global__ __launch_bounds__(256 * Q) void ir_conv_kernel(
        const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ len, const int32_t* __restrict__ ir_idx,
        const float* __restrict__ spectra, const int32_t* __restrict__ ir_len, int n_ir, int max_taps, int hop,
        float* __restrict__ out, int64_t ldo, int64_t L, int32_t* __restrict__ len_out) {
    constexpr int N = IrGeo<Q>::N, T = IrGeo<Q>::T, IO = Q == 4 ? LQ : LA;
    extern __shared__ float lds[];
    const int t = threadIdx.x, b = blockIdx.y;
    int64_t lb = ldx;
    if (len) lb = len[b] < 0 ? 0 : (len[b] < ldx ? (int64_t)len[b] : ldx);
    // device-side values are clamped: an IR index or tap count outside the bank makes the clip a pass-through
    int ir = ir_idx ? ir_idx[b] : -1, taps = 0;
    if (ir >= 0 && ir < n_ir) {
        taps = ir_len[ir];
        if (taps < 1 || taps > max_taps) taps = 0;
    }
    const bool pass = taps == 0;
    int64_t lo = lb == 0 ? 0 : lb + (pass ? 0 : taps - 1);
    if (lo > L) lo = L;
    if (blockIdx.x == 0 && t == 0 && len_out) len_out[b] = (int32_t)lo;
    const int64_t o0 = (int64_t)blockIdx.x * 2 * hop;       // this workgroup writes out[b][o0 : o0 + 2 hop) (up to L)
    const float* xb = x + (int64_t)b * ldx;
    float* ob = out + (int64_t)b * ldo;
    if (pass || o0 >= lo) {                                 // bit-exact copy / zero fill (uniform over the workgroup)
        for (int i = t; i < 2 * hop; i += T) {
            const int64_t g = o0 + i;
            if (g < L) ob[g] = (pass && g < lo) ? xb[g] : 0.f;
        }
        return;
    }
    // window of tile 2p: samples w0 .. w0 + N of the row, tile 2p + 1 starts hop later.  Row positions are 64-bit and uniform;
    // what a lane adds is a 32-bit slot, tested against the window's part inside [0, lb)
    const int64_t w0 = o0 - (N - hop);
    const float* xw = (const float*)((intptr_t)xb + w0 * 4);
    const int a_lo = (int)ir_clamp(-w0, N), a_hi = (int)ir_clamp(lb - w0, N);
    const int b_lo = (int)ir_clamp(-w0 - hop, N), b_hi = (int)ir_clamp(lb - w0 - hop, N);
    float re[16], im[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int s = ir_slot<IO>(t, j);
        re[j] = (s >= a_lo && s < a_hi) ? xw[s] : 0.f;
        im[j] = (s >= b_lo && s < b_hi) ? xw[s + hop] : 0.f;
    }
    const float2* tw = (const float2*)spectra;
    ir_fft_fwd<Q>(re, im, lds, tw, t);
    const float2* H = tw + N + (int64_t)ir * N;
#pragma unroll
    for (int g = 0; g < 16; g += 8) {
        float2 h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = H[(unsigned)((g + j) * T + t)];
#pragma unroll
        for (int j = 0; j < 8; ++j) ir_cmul<false>(re[g + j], im[g + j], h[j].x, h[j].y);
        __builtin_amdgcn_sched_barrier(0);
    }
    // the inverse uses the forward's table and LDS offsets again: derived afresh from an opaque copy of t they cost a few
    // dozen VALU, kept alive across the forward transform they cost some fifty registers (and spills at 1024 threads)
    int ti = t;
    asm volatile("" : "+v"(ti));
    ir_fft_inv<Q>(re, im, lds, tw, ti);
    // the first N - hop samples of a window carry the circular wrap; of the hop behind them, those below len_out are results,
    // those up to L are the zero fill
    float* ow = ob + o0;
    const int a_val = (int)ir_clamp(lo - o0, hop), a_end = (int)ir_clamp(L - o0, hop);
    const int b_val = (int)ir_clamp(lo - o0 - hop, hop), b_end = (int)ir_clamp(L - o0 - hop, hop);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = ir_slot<IO>(t, j) - (N - hop);
        if (i >= 0) {
            if (i < a_end) ow[i] = i < a_val ? re[j] : 0.f;
            if (i < b_end) ow[i + hop] = i < b_val ? im[j] : 0.f;
        }
    }
}

bool ir_plan(int max_taps, int* fft_n, int* hop) {
    if (max_taps < 1 || max_taps > PA_IR_MAX_TAPS) return false;
    const int n = max_taps <= IR_SMALL_TAPS ? IrGeo<1>::N : IrGeo<4>::N;
    *fft_n = n;
    *hop = (n - max_taps + 1) & ~63;
    return true;
}

// W_N^i = exp(-2 pi i / N), rounded from double; built once per size, lives as long as the library
const float* ir_host_twiddles(int n) {
    static std::mutex mu;
    static std::vector<float> small, big;
    std::lock_guard<std::mutex> g(mu);
    std::vector<float>& v = n == IrGeo<1>::N ? small : big;
    if (v.empty()) {
        v.resize(2 * (size_t)n);
        for (int i = 0; i < n; ++i) {
            const double a = -2.0 * M_PI * (double)i / (double)n;
            v[2 * i] = (float)cos(a);
            v[2 * i + 1] = (float)sin(a);
        }
    }
    return v.data();
}

template <int Q, typename K> bool ir_lds_ok(K kernel, signed char (&state)[64]) {
    constexpr int bytes = IrGeo<Q>::LDS_FLOATS * 4;
    return bytes <= 65536 || lds_attr_on_this_device((const void*)kernel, bytes, state);
}

}  // namespace

extern "C" int pa_ir_conv_plan(int max_taps, int* fft_n, int* hop) {
    int n = 0, h = 0;
    if (!ir_plan(max_taps, &n, &h)) return PA_EINVAL;
    if (fft_n) *fft_n = n;
    if (hop) *hop = h;
    return PA_OK;
}

extern "C" int64_t pa_ir_bank_floats(int n_ir, int max_taps) {
    int n = 0, h = 0;
    if (n_ir <= 0 || !ir_plan(max_taps, &n, &h)) return 0;
    return 2 * (int64_t)n * (1 + (int64_t)n_ir);
}

extern "C" int pa_ir_bank_prepare(const float* irs, int n_ir, int ld_ir, const int32_t* ir_len, float* spectra, void* stream) {
    int n = 0, h = 0;
    if (!irs || !spectra || n_ir <= 0 || !ir_plan(ld_ir, &n, &h) || ((uintptr_t)spectra & 7)) return PA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemcpyAsync(spectra, ir_host_twiddles(n), 2 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return set_hip_error(e);
    static signed char attr[64];
    if (n == IrGeo<1>::N) {
        hipLaunchKernelGGL(ir_bank_kernel<1>, dim3(n_ir), dim3(IrGeo<1>::T), IrGeo<1>::LDS_FLOATS * 4, st, irs, ld_ir, ir_len, spectra);
    } else {
        if (!ir_lds_ok<4>(ir_bank_kernel<4>, attr)) return PA_ELAUNCH;
        hipLaunchKernelGGL(ir_bank_kernel<4>, dim3(n_ir), dim3(IrGeo<4>::T), IrGeo<4>::LDS_FLOATS * 4, st, irs, ld_ir, ir_len, spectra);
    }
    return check_launch();
}

extern "C" int pa_wave_ir_convolve(const float* x, int B, int64_t ldx, const int32_t* len, const int32_t* ir_idx, const float* spectra,
                                   const int32_t* ir_len, int n_ir, int max_taps, float* out, int64_t ldo, int64_t L, int32_t* len_out,
                                   void* stream) {
    int n = 0, hop = 0;
    if (!x || !out || !spectra || B <= 0 || B > 65535 || L <= 0 || L > 0x7fffffff || ldx <= 0 || n_ir <= 0 || ldo < L) return PA_EINVAL;
    if (!ir_plan(max_taps, &n, &hop) || (ir_idx && !ir_len) || ((uintptr_t)spectra & 7)) return PA_EINVAL;
    const dim3 grid((unsigned)cdiv(cdiv(L, hop), 2), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    static signed char attr[64];
    if (n == IrGeo<1>::N) {
        hipLaunchKernelGGL(ir_conv_kernel<1>, grid, dim3(IrGeo<1>::T), IrGeo<1>::LDS_FLOATS * 4, st, x, ldx, len, ir_idx, spectra, ir_len, n_ir,
                           max_taps, hop, out, ldo, L, len_out);
    } else {
        if (!ir_lds_ok<4>(ir_conv_kernel<4>, attr)) return PA_ELAUNCH;
        hipLaunchKernelGGL(ir_conv_kernel<4>, grid, dim3(IrGeo<4>::T), IrGeo<4>::LDS_FLOATS * 4, st, x, ldx, len, ir_idx, spectra, ir_len, n_ir,
                           max_taps, hop, out, ldo, L, len_out);
    }
    return check_launch();
}

// lpips.hip -- the parts of the LPIPS distance (metrics.py:17-24: lpips_tf defaults = AlexNet trunk + linear heads, v0.1) that savp_conv
// does not cover (include/savp_hip.h):
//   savp_lpips_stem          : input affine + conv1 (11x11 stride 4 pad 2, 1|3 -> 64) + bias + ReLU on the fp32 MFMA pipe
//   savp_lpips_maxpool3s2    : NHWC 3x3 stride-2 max-pool (between conv1 / conv2 and conv2 / conv3)
//   savp_lpips_head          : channel normalisation, squared difference, 1x1 `lin`, spatial mean, summed over the five taps
//   savp_lpips_diversity_add : the running sum of eval_diversity over the samples of a chunk
// conv2 .. conv5 are savp_conv FPROP calls.  fp32 throughout; no atomics -- every output element has one writer and every sum a fixed order.
//
// The stem.  As a GEMM conv1 is [pixels] x [K = 11 * 33] x [64]; with three channels a kernel row is 33 CONTIGUOUS floats of the input
// row, so the im2col operand never has to be materialised: a workgroup stages the input rows of a strip of output rows in LDS once (affine
// applied, zeros outside the image) and every A fragment is read straight out of that patch at (4 oy + ky) * RS + 12 ox + k.  K is walked
// as 11 rows of 36 (33 + 3 zero weights; the three extra A values are the next pixels of the staged row, finite by construction), so a
// lane's k pair is 8-byte aligned: one ds_read_b64 per operand feeds two v_mfma_f32_32x32x2_f32.  The weights arrive row by row (9 KB),
// double-buffered through registers, in the pair-interleaved order [kp][co][2] that makes the B read a conflict-free ds_read_b64.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define NT 256
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

#define STEM_K 11
#define STEM_STRIDE 4
#define STEM_PAD 2
#define STEM_CO SAVP_LPIPS_STEM_CO
#define STEM_KROW SAVP_LPIPS_STEM_KROW
#define STEM_WROW (STEM_KROW * STEM_CO)              // floats of one kernel row of the packed weights
#define STEM_MTILE 128                               // output pixels per workgroup: 4 waves x 32
#define STEM_WPT (STEM_WROW / NT)                    // weight floats per thread per kernel row

typedef float floatx16 __attribute__((ext_vector_type(16)));

// strip geometry shared by the launcher and the kernel
__host__ __device__ inline int stem_out(int in) { return (in + 2 * STEM_PAD - STEM_K) / STEM_STRIDE + 1; }
__host__ __device__ inline int stem_rows_per_strip(int Wo) { return Wo >= STEM_MTILE ? 1 : STEM_MTILE / Wo; }
__host__ __device__ inline int stem_row_stride(int Wo) { return (Wo - 1) * STEM_STRIDE * 3 + STEM_KROW; }      // even

__global__ __launch_bounds__(NT) void lpips_stem_kernel(const float* __restrict__ x, long long x_s0, long long x_s1, int N1, int H, int W,
                                                        int C, int Ho, int Wo, const float* __restrict__ wp,
                                                        const float* __restrict__ bias, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Wl = smem;                                // [2][STEM_WROW]
    float* patch = smem + 2 * STEM_WROW;             // [rows_in][RS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, khalf = lane >> 5;
    const int R = stem_rows_per_strip(Wo), RS = stem_row_stride(Wo);
    const int strips = (Ho + R - 1) / R;
    const int n = blockIdx.x / strips, oy0 = (blockIdx.x % strips) * R;
    const int rows_out = min(R, Ho - oy0);
    const int rows_in = (rows_out - 1) * STEM_STRIDE + STEM_K;
    const int npix = rows_out * Wo;                  // valid pixels of this strip (<= STEM_MTILE unless Wo > STEM_MTILE: see launcher)
    const float* px = x + (long long)(n / N1) * x_s0 + (long long)(n % N1) * x_s1;

    float wreg[STEM_WPT];
#pragma unroll
    for (int i = 0; i < STEM_WPT; ++i) wreg[i] = wp[i * NT + tid];
    // the patch: every word of [rows_in][RS] is written (the MFMA loop reads up to 3 floats past a pixel's 33)
    for (int i = tid; i < rows_in * RS; i += NT) {
        const int r = i / RS, q = i - r * RS;
        const int xc = q / 3, c = q - xc * 3;
        const int iy = oy0 * STEM_STRIDE - STEM_PAD + r, ix = xc - STEM_PAD;
        float v = 0.f;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
            const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
            const float t = 2.f * px[((long long)iy * W + ix) * C + (C == 3 ? c : 0)] - 1.f;
            v = (t - shift) / scale;
        }
        patch[i] = v;
    }
#pragma unroll
    for (int i = 0; i < STEM_WPT; ++i) Wl[i * NT + tid] = wreg[i];
    __syncthreads();

    const int m = min(wave * 32 + l31, npix - 1);    // rows past the strip recompute its last pixel and are not stored
    const float* arow = patch + (m / Wo) * STEM_STRIDE * RS + (m % Wo) * STEM_STRIDE * 3 + 2 * khalf;
    floatx16 acc0 = {0}, acc1 = {0};
    for (int ky = 0; ky < STEM_K; ++ky) {
        if (ky + 1 < STEM_K) {
#pragma unroll
            for (int i = 0; i < STEM_WPT; ++i) wreg[i] = wp[(ky + 1) * STEM_WROW + i * NT + tid];
        }
        const float* a = arow + ky * RS;
        const float* b = Wl + (ky & 1) * STEM_WROW + khalf * (2 * STEM_CO) + 2 * l31;
#pragma unroll
        for (int q = 0; q < STEM_KROW / 4; ++q) {
            const float2 av = *reinterpret_cast<const float2*>(a + 4 * q);
            const float2 b0 = *reinterpret_cast<const float2*>(b + q * (4 * STEM_CO));
            const float2 b1 = *reinterpret_cast<const float2*>(b + q * (4 * STEM_CO) + 64);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1.y, acc1, 0, 0, 0);
        }
        if (ky + 1 < STEM_K) {
            float* wn = Wl + ((ky + 1) & 1) * STEM_WROW;
#pragma unroll
            for (int i = 0; i < STEM_WPT; ++i) wn[i * NT + tid] = wreg[i];
        }
        __syncthreads();
    }

    float* py = y + ((long long)n * Ho + oy0) * Wo * STEM_CO;
    const float bias0 = bias[l31], bias1 = bias[32 + l31];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        if (row >= npix) continue;
        py[(long long)row * STEM_CO + l31] = fmaxf(acc0[r] + bias0, 0.f);
        py[(long long)row * STEM_CO + 32 + l31] = fmaxf(acc1[r] + bias1, 0.f);
    }
}

extern "C" int savp_lpips_stem(void* stream, const float* x, int64_t x_s0, int64_t x_s1, int32_t N, int32_t N1, int32_t H, int32_t W,
                               int32_t C, const float* wp, const float* bias, float* y) {
    if (!x || !wp || !bias || !y || N < 1 || N1 < 1 || H < 7 || W < 7 || (C != 1 && C != 3)) return SAVP_EINVAL;
    const int Ho = stem_out(H), Wo = stem_out(W);
    if (Wo > STEM_MTILE) return SAVP_EINVAL;        // a strip is at least one whole output row
    const int R = stem_rows_per_strip(Wo), RS = stem_row_stride(Wo);
    const int strips = (Ho + R - 1) / R;
    const size_t lds = ((size_t)2 * STEM_WROW + (size_t)((R - 1) * STEM_STRIDE + STEM_K) * RS) * sizeof(float);
    if (lds > 64 * 1024 || (int64_t)N * strips > 0x7fffffff) return SAVP_EINVAL;
    hipLaunchKernelGGL(lpips_stem_kernel, dim3((unsigned)(N * strips)), dim3(NT), lds, (hipStream_t)stream, x, (long long)x_s0,
                       (long long)x_s1, N1, H, W, C, Ho, Wo, wp, bias, y);
    return LAUNCH_OK();
}

// one thread per (n, oy, ox, 4 channels)
__global__ __launch_bounds__(NT) void lpips_maxpool_kernel(const float4* __restrict__ x, int H, int W, int C4, int Ho, int Wo, long long total,
                                                           float4* __restrict__ y) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4);
    long long r = i / C4;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const long long n = r / Ho;
    const float4* p = x + ((n * H + 2 * oy) * W + 2 * ox) * C4 + c;
    float4 v = p[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 u = p[((long long)dy * W + dx) * C4];
            v.x = fmaxf(v.x, u.x); v.y = fmaxf(v.y, u.y); v.z = fmaxf(v.z, u.z); v.w = fmaxf(v.w, u.w);
        }
    y[i] = v;
}

extern "C" int savp_lpips_maxpool3s2(void* stream, const float* x, int32_t N, int32_t H, int32_t W, int32_t C, float* y) {
    if (!x || !y || N < 1 || H < 3 || W < 3 || C < 4 || (C & 3) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return SAVP_EINVAL;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    const long long total = (long long)N * Ho * Wo * (C / 4);
    const long long blocks = (total + NT - 1) / NT;
    if (blocks > 0x7fffffff) return SAVP_EINVAL;
    hipLaunchKernelGGL(lpips_maxpool_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, (const float4*)x, H, W, C / 4, Ho, Wo,
                       total, (float4*)y);
    return LAUNCH_OK();
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// head
// ---------------------------------------------------------------------------------------------------------------------------------------
#define HEAD_MAXC 384
#define HEAD_CPL (HEAD_MAXC / 64)                   // channels per lane

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(NT) void lpips_head_kernel(SavpLpipsHeadArgs a) {
    __shared__ float sh[NT / 64];
    const int f = blockIdx.x / a.N, n = blockIdx.x % a.N;
    if (a.ctl) {                                     // uniform per workgroup
        const int s = a.s0 + n / a.B;
        if (s >= a.ctl[0]) return;
        if (a.nd > 0 && !(a.ctl[1] + s > 0 && a.ctl[1] + s <= a.nd)) return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float total = 0.f;                               // identical on every thread
    for (int l = 0; l < SAVP_LPIPS_TAPS; ++l) {
        const int hw = a.hw[l], C = a.c[l];
        const float* pa = a.a[l] + ((long long)f * a.a_n1 + n) * hw * C;
        const float* pb = a.b[l] + ((long long)f * a.b_n1 + n % a.b_mod) * hw * C;
        const float* lin = a.lin[l];
        float acc = 0.f;                             // this wave's pixels, in order
        for (int p = wave; p < hw; p += NT / 64) {
            float va[HEAD_CPL], vb[HEAD_CPL];
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int j = 0; j < HEAD_CPL; ++j) {
                const int c = j * 64 + lane;
                va[j] = c < C ? pa[(long long)p * C + c] : 0.f;
                vb[j] = c < C ? pb[(long long)p * C + c] : 0.f;
                sa += va[j] * va[j];
                sb += vb[j] * vb[j];
            }
            const float ia = 1.f / (sqrtf(wave_sum(sa)) + 1e-10f), ib = 1.f / (sqrtf(wave_sum(sb)) + 1e-10f);
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < HEAD_CPL; ++j) {
                const int c = j * 64 + lane;
                float e;
                {   // the two products are rounded before the subtraction: contracted into an fma, equal taps would leave the rounding
                    // residual of one product instead of exactly 0
#pragma clang fp contract(off)
                    const float na = va[j] * ia, nb = vb[j] * ib;
                    e = na - nb;
                }
                d += (c < C ? lin[c] : 0.f) * e * e;
            }
            acc += wave_sum(d);
        }
        __syncthreads();
        if (lane == 0) sh[wave] = acc;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) t += sh[w];
        total += t / (float)hw;
    }
    if (threadIdx.x == 0) a.out[(long long)f * a.out_n1 + n] = a.sign * total;
}

extern "C" int savp_lpips_head(void* stream, const SavpLpipsHeadArgs* a) {
    if (!a || !a->out || a->F < 1 || a->N < 1 || a->a_n1 < 1 || a->b_n1 < 1 || a->b_mod < 1 || a->out_n1 < 1) return SAVP_EINVAL;
    for (int l = 0; l < SAVP_LPIPS_TAPS; ++l)
        if (!a->a[l] || !a->b[l] || !a->lin[l] || a->hw[l] < 1 || a->c[l] < 1 || a->c[l] > HEAD_MAXC) return SAVP_EINVAL;
    if (a->ctl && a->B < 1) return SAVP_EINVAL;
    if ((int64_t)a->F * a->N > 0x7fffffff) return SAVP_EINVAL;
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)(a->F * a->N)), dim3(NT), 0, (hipStream_t)stream, *a);
    return LAUNCH_OK();
}

// one thread per (f, b)
__global__ __launch_bounds__(NT) void lpips_diversity_add_kernel(const float* dv, int FB, int S, int B, const int* ctl, int nd, float* div) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= FB) return;
    const int f = i / B, b = i % B, nv = ctl[0], base = ctl[1];
    float v = div[i];
    for (int s = 0; s < nv; ++s)
        if (base + s > 0 && base + s <= nd) v += dv[((long long)f * S + s) * B + b];
    div[i] = v;
}

extern "C" int savp_lpips_diversity_add(void* stream, const float* dv, int32_t F, int32_t S, int32_t B, const int32_t* ctl, int32_t nd,
                                        float* div) {
    if (!dv || !ctl || !div || F < 1 || S < 1 || B < 1 || nd < 0 || (int64_t)F * B > 0x7fffffff) return SAVP_EINVAL;
    hipLaunchKernelGGL(lpips_diversity_add_kernel, dim3((unsigned)((F * B + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, dv, F * B, S,
                       B, ctl, nd, div);
    return LAUNCH_OK();
}

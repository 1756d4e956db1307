// metrics.hip -- evaluation metrics and the best-of-N sampling fold of the reference:
//   frame mse / psnr   : video_prediction/metrics.py:5-10 (tf.image.psnr with max_val 1)
//   frame ssim         : metrics.py:13-14 (tf.image.ssim: 11x11 Gaussian window sigma 1.5, k1 0.01, k2 0.03, 'VALID')
//   eval_accumulate    : base_model.py:176-190 -- running min / sum / max of a [T, B] metric, chosen per batch element by the
//                        mean over time (sort_criterion :173-174)
//   select_batch       : base_model.py:170-171,191-196 -- where_axis1 on time-major tensors / running sum of the samples
// All tensors are time-major [T, B, ...] with explicit (time, batch) strides so that one batch half of the generator's
// [T, 2B, ...] buffer can be used in place.  HBM-bound, tiny next to the generator unroll; one launch each.  SSIM reads every pixel 121
// times out of LDS and is the largest of them: the fold's SSIM launch is 2.8 % of the kernel time of a parallel evaluation chunk of the
// 128x128 workload (1.36 ms of 48.2 ms at S = 4, B = 8, 28 future frames; profiles/ssim_large.md).
// Frame size: SSIM, and with it savp_eval_fold_samples, takes any H >= 11 and 11 <= W <= 744: planes of up to 8192 pixels sit in LDS whole,
// larger ones are walked in strips of whole rows (ssim_strip_rows); wider rows would need column tiling and are refused.  The other
// entries take any frame.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"
#include "zero_fill.h"

#define NT 256
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float block_sum1(float v, float* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    float s = wsum(v);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
    return t;
}

// Per-frame device code shared by the single-sample kernels below and the multi-sample fold (savp_eval_fold_samples): one workgroup of
// NT threads, the same loop order and reduction tree, hence bit-identical values.  Macros rather than inline functions: the two
// single-sample kernels keep exactly the instruction stream they had before the fold existed.
//   FRAME_SQ_ERR_SUM: const float s = sum over the frame of (pa - pb)^2 (on every thread)
#define FRAME_SQ_ERR_SUM(s, pa, pb, inner, sh)                                                                        \
    float acc_##s = 0.f;                                                                                              \
    for (int i = threadIdx.x; i < inner; i += NT) { const float d = pa[i] - pb[i]; acc_##s += d * d; }               \
    const float s = block_sum1(acc_##s, sh)

// one workgroup per frame (t, b): mse = mean((a-b)^2) over the frame; psnr = -10 log10(mse)
__global__ __launch_bounds__(NT) void frame_mse_kernel(const float* a, long long a_st, long long a_sb, const float* b, long long b_st,
                                                       long long b_sb, int B, int inner, float* mse, float* psnr) {
    __shared__ float sh[4];
    const int t = blockIdx.x / B, bb = blockIdx.x % B;
    const float* pa = a + t * a_st + bb * a_sb;
    const float* pb = b + t * b_st + bb * b_sb;
    FRAME_SQ_ERR_SUM(s, pa, pb, inner, sh);
    if (threadIdx.x == 0) {
        const float m = s / (float)inner;
        if (mse) mse[blockIdx.x] = m;
        if (psnr) psnr[blockIdx.x] = -10.f * log10f(m);
    }
}

#define SSIM_K 11
//   SSIM_PLANE_SUM: both planes of one channel (pa / pb point at channel c of the frame, pixel stride C) into LDS `plane` [2][H*W];
//   const float s = sum of lum * cs over the Ho x Wo window positions (on every thread); also declares Ho, Wo.  Needs `plane`, `g`
//   [SSIM_K] and `sh` [4] in shared memory.
#define SSIM_PLANE_SUM(RES, pa, pb, H, W, C)                                                                                                \
    float* xa = plane;                                                                                                                     \
    float* xb = plane + H * W;                                                                                                             \
    for (int i = threadIdx.x; i < H * W; i += NT) { xa[i] = pa[(long long)i * C]; xb[i] = pb[(long long)i * C]; }                          \
    if (threadIdx.x == 0) {                            /* _fspecial_gauss: the 2-D softmax factorises into normalised 1-D windows */    \
        float s = 0.f, w[SSIM_K];                                                                                                          \
        for (int i = 0; i < SSIM_K; ++i) { const float d = (float)i - 0.5f * (SSIM_K - 1); w[i] = expf(-d * d / (2.f * 1.5f * 1.5f)); s += w[i]; }\
        for (int i = 0; i < SSIM_K; ++i) g[i] = w[i] / s;                                                                                  \
    }                                                                                                                                      \
    __syncthreads();                                                                                                                       \
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;                                                                                    \
    const int Ho = H - SSIM_K + 1, Wo = W - SSIM_K + 1;                                                                                    \
    float acc = 0.f;                                                                                                                       \
    for (int o = threadIdx.x; o < Ho * Wo; o += NT) {                                                                                      \
        const int oy = o / Wo, ox = o % Wo;                                                                                                \
        float m0 = 0.f, m1 = 0.f, sxy = 0.f, sqq = 0.f;                                                                                    \
        for (int u = 0; u < SSIM_K; ++u) {                                                                                                 \
            float r0 = 0.f, r1 = 0.f, rxy = 0.f, rqq = 0.f;                                                                                \
            const float* ra = xa + (oy + u) * W + ox;                                                                                      \
            const float* rb = xb + (oy + u) * W + ox;                                                                                      \
_Pragma("unroll")                                                                                                                          \
            for (int v = 0; v < SSIM_K; ++v) {                                                                                             \
                const float x = ra[v], y = rb[v], w = g[v];                                                                                \
                r0 += w * x; r1 += w * y; rxy += w * x * y; rqq += w * (x * x + y * y);                                                    \
            }                                                                                                                              \
            m0 += g[u] * r0; m1 += g[u] * r1; sxy += g[u] * rxy; sqq += g[u] * rqq;                                                        \
        }                                                                                                                                  \
        const float num0 = 2.f * m0 * m1, den0 = m0 * m0 + m1 * m1;                                                                        \
        const float lum = (num0 + c1) / (den0 + c1);                                                                                       \
        const float cs = (2.f * sxy - num0 + c2) / (sqq - den0 + c2);                                                                      \
        acc += lum * cs;                                                                                                                   \
    }                                                                                                                                      \
    const float RES = block_sum1(acc, sh)

// Planes that do not fit SSIM_LDS_BYTES whole (more than 8192 pixels) are walked in strips of R window rows, ascending: R + SSIM_K - 1 input
// rows of both planes are staged per strip and every thread carries its sum of lum * cs across the strips into one block_sum1.  The same
// direct 11x11 window as SSIM_PLANE_SUM; neighbouring strips re-read the SSIM_K - 1 rows they share.
#define SSIM_LDS_BYTES (64 * 1024)
// strip geometry shared by the launchers and the kernels: the largest R with [2][R + SSIM_K - 1][W] floats inside SSIM_LDS_BYTES
// (54 at W = 128, 15 at W = 320); < 1 when not even one window row fits (W > 744)
__host__ __device__ inline int ssim_strip_rows(int W) { return SSIM_LDS_BYTES / (2 * W * (int)sizeof(float)) - (SSIM_K - 1); }
static inline size_t ssim_strip_lds(int R, int W) { return (size_t)2 * (R + SSIM_K - 1) * W * sizeof(float); }

//   returns the sum of lum * cs over the Ho x Wo window positions (on every thread); pa / pb as for SSIM_PLANE_SUM, `plane` is
//   [2][R + SSIM_K - 1][W]
__device__ __forceinline__ float ssim_strip_sum(const float* pa, const float* pb, int H, int W, int C, float* plane, float* g, float* sh) {
    const int R = ssim_strip_rows(W);
    const int Ho = H - SSIM_K + 1, Wo = W - SSIM_K + 1;
    float* xa = plane;
    float* xb = plane + (R + SSIM_K - 1) * W;
    if (threadIdx.x == 0) {                            // the normalised 1-D window of SSIM_PLANE_SUM
        float s = 0.f, w[SSIM_K];
        for (int i = 0; i < SSIM_K; ++i) { const float d = (float)i - 0.5f * (SSIM_K - 1); w[i] = expf(-d * d / (2.f * 1.5f * 1.5f)); s += w[i]; }
        for (int i = 0; i < SSIM_K; ++i) g[i] = w[i] / s;
    }
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    float acc = 0.f;
    for (int oy0 = 0; oy0 < Ho; oy0 += R) {
        const int rows_out = min(R, Ho - oy0);         // the last strip may be short
        const int n_in = (rows_out + SSIM_K - 1) * W;  // input rows oy0 .. oy0 + rows_out + 9 <= H - 1
        const long long base = (long long)oy0 * W;
        __syncthreads();                               // the previous strip's windows are done with the planes
        for (int i = threadIdx.x; i < n_in; i += NT) { xa[i] = pa[(base + i) * C]; xb[i] = pb[(base + i) * C]; }
        __syncthreads();
        for (int o = threadIdx.x; o < rows_out * Wo; o += NT) {
            const int oy = o / Wo, ox = o % Wo;
            float m0 = 0.f, m1 = 0.f, sxy = 0.f, sqq = 0.f;
            for (int u = 0; u < SSIM_K; ++u) {
                float r0 = 0.f, r1 = 0.f, rxy = 0.f, rqq = 0.f;
                const float* ra = xa + (oy + u) * W + ox;
                const float* rb = xb + (oy + u) * W + ox;
#pragma unroll
                for (int v = 0; v < SSIM_K; ++v) {
                    const float x = ra[v], y = rb[v], w = g[v];
                    r0 += w * x; r1 += w * y; rxy += w * x * y; rqq += w * (x * x + y * y);
                }
                m0 += g[u] * r0; m1 += g[u] * r1; sxy += g[u] * rxy; sqq += g[u] * rqq;
            }
            const float num0 = 2.f * m0 * m1, den0 = m0 * m0 + m1 * m1;
            const float lum = (num0 + c1) / (den0 + c1);
            const float cs = (2.f * sxy - num0 + c2) / (sqq - den0 + c2);
            acc += lum * cs;
        }
    }
    return block_sum1(acc, sh);
}

// one workgroup per (frame, channel): both planes in LDS, every thread evaluates a strip of window positions
__global__ __launch_bounds__(NT) void frame_ssim_kernel(const float* a, long long a_st, long long a_sb, const float* b, long long b_st,
                                                        long long b_sb, int B, int H, int W, int C, float* out) {
    extern __shared__ float plane[];                   // [2][H*W]
    __shared__ float sh[4];
    __shared__ float g[SSIM_K];
    const int f = blockIdx.x / C, c = blockIdx.x % C;
    const int t = f / B, bb = f % B;
    const float* pa = a + t * a_st + bb * a_sb + c;
    const float* pb = b + t * b_st + bb * b_sb + c;
    SSIM_PLANE_SUM(s, pa, pb, H, W, C);
    if (threadIdx.x == 0) unsafeAtomicAdd(out + f, s / ((float)(Ho * Wo) * (float)C));
}

// frame_ssim_kernel for planes of more than 8192 pixels: the same grid and the same add into out, the plane in strips
__global__ __launch_bounds__(NT) void frame_ssim_strip_kernel(const float* a, long long a_st, long long a_sb, const float* b, long long b_st,
                                                              long long b_sb, int B, int H, int W, int C, float* out) {
    extern __shared__ float plane[];                   // [2][R + SSIM_K - 1][W]
    __shared__ float sh[4];
    __shared__ float g[SSIM_K];
    const int f = blockIdx.x / C, c = blockIdx.x % C;
    const int t = f / B, bb = f % B;
    const float s = ssim_strip_sum(a + t * a_st + bb * a_sb + c, b + t * b_st + bb * b_sb + c, H, W, C, plane, g, sh);
    if (threadIdx.x == 0) unsafeAtomicAdd(out + f, s / ((float)((H - SSIM_K + 1) * (W - SSIM_K + 1)) * (float)C));
}

// single workgroup: per batch element b compare mean_t metric with mean_t vmin / vmax, update min / sum / max
__global__ __launch_bounds__(NT) void eval_accumulate_kernel(const float* metric, float* vmin, float* vsum, float* vmax, int* cmin, int* cmax,
                                                            int T, int B) {
    for (int b = threadIdx.x; b < B; b += NT) {
        float sm = 0.f, smin = 0.f, smax = 0.f;
        for (int t = 0; t < T; ++t) { sm += metric[t * B + b]; smin += vmin[t * B + b]; smax += vmax[t * B + b]; }
        const bool lo = sm / (float)T < smin / (float)T, hi = sm / (float)T > smax / (float)T;
        for (int t = 0; t < T; ++t) {
            const float m = metric[t * B + b];
            if (lo) vmin[t * B + b] = m;
            if (hi) vmax[t * B + b] = m;
            vsum[t * B + b] += m;
        }
        cmin[b] = lo ? 1 : 0; cmax[b] = hi ? 1 : 0;
    }
}

// out[t, b, :] = cond[b] ? x[t, b, :] : out[t, b, :]   (mode 0)   |   out[t, b, :] += x[t, b, :]   (mode 1)
__global__ __launch_bounds__(NT) void select_batch_kernel(const int* cond, const float* x, long long x_st, long long x_sb, float* out,
                                                         long long o_st, long long o_sb, int B, int inner, int mode) {
    const int t = blockIdx.y, bb = blockIdx.z;
    if (mode == 0 && !cond[bb]) return;
    const float* px = x + t * x_st + bb * x_sb;
    float* po = out + t * o_st + bb * o_sb;
    for (int i = blockIdx.x * NT + threadIdx.x; i < inner; i += gridDim.x * NT) po[i] = mode ? po[i] + px[i] : px[i];
}

extern "C" int savp_frame_mse_psnr(void* stream, const float* a, int64_t a_st, int64_t a_sb, const float* b, int64_t b_st, int64_t b_sb,
                                   int32_t T, int32_t B, int32_t inner, float* mse, float* psnr) {
    if (!a || !b || T < 1 || B < 1 || inner < 1 || (!mse && !psnr)) return SAVP_EINVAL;
    hipLaunchKernelGGL(frame_mse_kernel, dim3((unsigned)(T * B)), dim3(NT), 0, (hipStream_t)stream, a, (long long)a_st, (long long)a_sb, b,
                       (long long)b_st, (long long)b_sb, B, inner, mse, psnr);
    return LAUNCH_OK();
}

extern "C" int savp_frame_ssim(void* stream, const float* a, int64_t a_st, int64_t a_sb, const float* b, int64_t b_st, int64_t b_sb,
                               int32_t T, int32_t B, int32_t H, int32_t W, int32_t C, float* out) {
    if (!a || !b || !out || T < 1 || B < 1 || H < SSIM_K || W < SSIM_K || C < 1) return SAVP_EINVAL;
    const size_t lds = (size_t)2 * H * W * sizeof(float);
    const bool strips = lds > SSIM_LDS_BYTES;          // more than 8192 pixels: strips of whole rows
    const int R = ssim_strip_rows(W);
    if (strips && (R < 1 || (int64_t)H * W * C > 0x7fffffff)) return SAVP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    savp_zero_async(out, (size_t)T * B * sizeof(float), st);
    if (strips)
        hipLaunchKernelGGL(frame_ssim_strip_kernel, dim3((unsigned)(T * B * C)), dim3(NT), ssim_strip_lds(R, W), st, a, (long long)a_st,
                           (long long)a_sb, b, (long long)b_st, (long long)b_sb, B, H, W, C, out);
    else
        hipLaunchKernelGGL(frame_ssim_kernel, dim3((unsigned)(T * B * C)), dim3(NT), lds, st, a, (long long)a_st, (long long)a_sb, b,
                           (long long)b_st, (long long)b_sb, B, H, W, C, out);
    return LAUNCH_OK();
}

extern "C" int savp_eval_accumulate(void* stream, const float* metric, float* vmin, float* vsum, float* vmax, int32_t* cond_min,
                                    int32_t* cond_max, int32_t T, int32_t B) {
    if (!metric || !vmin || !vsum || !vmax || !cond_min || !cond_max || T < 1 || B < 1) return SAVP_EINVAL;
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, metric, vmin, vsum, vmax, cond_min, cond_max, T, B);
    return LAUNCH_OK();
}

extern "C" int savp_select_batch(void* stream, const int32_t* cond, const float* x, int64_t x_st, int64_t x_sb, float* out, int64_t o_st,
                                 int64_t o_sb, int32_t T, int32_t B, int32_t inner, int32_t mode) {
    if (!x || !out || T < 1 || B < 1 || inner < 1 || (mode == 0 && !cond)) return SAVP_EINVAL;
    unsigned gx = (unsigned)((inner + NT * 4 - 1) / (NT * 4));
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(select_batch_kernel, dim3(gx, (unsigned)T, (unsigned)B), dim3(NT), 0, (hipStream_t)stream, cond, x, (long long)x_st,
                       (long long)x_sb, out, (long long)o_st, (long long)o_sb, B, inner, mode);
    return LAUNCH_OK();
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// savp_eval_fold_samples: the per-frame metrics of S prior samples at once and the reference's sequential fold over them
// (base_model.py:176-201 run for s = 0 .. n_valid-1).  Prediction rows are sample-major, n = s * B + b.  Four launches, none with
// atomics: every output element has exactly one writer, and every sum is taken in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------------------------
struct EvalFoldStates { SavpEvalFoldState m[SAVP_EVAL_NMETRICS]; };

// one workgroup per (f, n): mse / psnr of future frame f of prediction row n against target (f, n % B)
__global__ __launch_bounds__(NT) void fold_mse_kernel(const float* tgt, long long t_st, long long t_sb, const float* pred, long long p_st,
                                                      long long p_sb, int SB, int B, int inner, const int* n_valid, float* psnr, float* mse) {
    __shared__ float sh[4];
    const int f = blockIdx.x / SB, n = blockIdx.x % SB;
    if (n / B >= *n_valid) return;                     // padded sample of the last chunk: never read
    const float* pa = tgt + f * t_st + (n % B) * t_sb;
    const float* pb = pred + f * p_st + n * p_sb;
    FRAME_SQ_ERR_SUM(s, pa, pb, inner, sh);
    if (threadIdx.x == 0) {
        const float m = s / (float)inner;
        mse[blockIdx.x] = m;
        psnr[blockIdx.x] = -10.f * log10f(m);
    }
}

// one workgroup per (f, n, c): channel c's share of the frame's ssim into its own slot (summed over c in order by fold_select_kernel)
__global__ __launch_bounds__(NT) void fold_ssim_kernel(const float* tgt, long long t_st, long long t_sb, const float* pred, long long p_st,
                                                       long long p_sb, int SB, int B, int H, int W, int C, const int* n_valid, float* part) {
    extern __shared__ float plane[];                   // [2][H*W]
    __shared__ float sh[4];
    __shared__ float g[SSIM_K];
    const int fn = blockIdx.x / C, c = blockIdx.x % C;
    const int f = fn / SB, n = fn % SB;
    if (n / B >= *n_valid) return;
    const float* pa = tgt + f * t_st + (n % B) * t_sb + c;
    const float* pb = pred + f * p_st + n * p_sb + c;
    SSIM_PLANE_SUM(s, pa, pb, H, W, C);
    if (threadIdx.x == 0) part[blockIdx.x] = s / ((float)(Ho * Wo) * (float)C);
}

// fold_ssim_kernel for planes of more than 8192 pixels: frame_ssim_strip_kernel's device code, the share into its own slot
__global__ __launch_bounds__(NT) void fold_ssim_strip_kernel(const float* tgt, long long t_st, long long t_sb, const float* pred,
                                                             long long p_st, long long p_sb, int SB, int B, int H, int W, int C,
                                                             const int* n_valid, float* part) {
    extern __shared__ float plane[];                   // [2][R + SSIM_K - 1][W]
    __shared__ float sh[4];
    __shared__ float g[SSIM_K];
    const int fn = blockIdx.x / C, c = blockIdx.x % C;
    const int f = fn / SB, n = fn % SB;
    if (n / B >= *n_valid) return;
    const float s = ssim_strip_sum(tgt + f * t_st + (n % B) * t_sb + c, pred + f * p_st + n * p_sb + c, H, W, C, plane, g, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s / ((float)((H - SSIM_K + 1) * (W - SSIM_K + 1)) * (float)C);
}

// single workgroup.  Phase 1: ssim[f, n] = sum over c of the channel shares, c ascending from 0 (frame_ssim_kernel adds them to a zeroed
// float).  Phase 2: one thread per (metric, b) runs eval_accumulate_kernel's update for s = 0 .. n_valid-1 in order and records the last
// sample that replaced the running min / max (-1: none) in sel[metric][0 | 1][b].
__global__ __launch_bounds__(NT) void fold_select_kernel(float* met, const float* part, int F, int SB, int B, int C, const int* n_valid,
                                                         EvalFoldStates st, int* sel) {
    const int nv = *n_valid;
    float* ssim = met + (size_t)SAVP_EVAL_SSIM * F * SB;
    for (int i = threadIdx.x; i < F * SB; i += NT) {
        if ((i % SB) / B >= nv) continue;
        float v = 0.f;
        for (int c = 0; c < C; ++c) v += part[(size_t)i * C + c];
        ssim[i] = v;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < SAVP_EVAL_NMETRICS * B; j += NT) {
        const int k = j / B, b = j % B;
        const float* metric = met + (size_t)k * F * SB;
        float* vmin = st.m[k].vmin;
        float* vsum = st.m[k].vsum;
        float* vmax = st.m[k].vmax;
        int smin_i = -1, smax_i = -1;
        for (int s = 0; s < nv; ++s) {
            const int n = s * B + b;
            float sm = 0.f, smin = 0.f, smax = 0.f;
            for (int t = 0; t < F; ++t) { sm += metric[t * SB + n]; smin += vmin[t * B + b]; smax += vmax[t * B + b]; }
            const bool lo = sm / (float)F < smin / (float)F, hi = sm / (float)F > smax / (float)F;
            for (int t = 0; t < F; ++t) {
                const float m = metric[t * SB + n];
                if (lo) vmin[t * B + b] = m;
                if (hi) vmax[t * B + b] = m;
                vsum[t * B + b] += m;
            }
            if (lo) smin_i = s;
            if (hi) smax_i = s;
        }
        sel[(k * 2 + 0) * B + b] = smin_i;
        sel[(k * 2 + 1) * B + b] = smax_i;
    }
}

// grid (x: slices of the frame, y: t, z: b): for each metric, gsum[t, b, i] += pred[t, s B + b, i] for s ascending, and the winning
// samples' whole sequences into gmin / gmax.  States are [T1, B, inner] contiguous.
__global__ __launch_bounds__(NT) void fold_gather_kernel(const float* pred, long long p_st, long long p_sb, int B, int inner,
                                                         const int* n_valid, EvalFoldStates st, const int* sel) {
    const int t = blockIdx.y, b = blockIdx.z;
    const int nv = *n_valid;
    const size_t o = ((size_t)t * B + b) * inner;
    const float* px = pred + t * p_st + b * p_sb;
    int smin[SAVP_EVAL_NMETRICS], smax[SAVP_EVAL_NMETRICS];
#pragma unroll
    for (int k = 0; k < SAVP_EVAL_NMETRICS; ++k) { smin[k] = sel[(k * 2 + 0) * B + b]; smax[k] = sel[(k * 2 + 1) * B + b]; }
    for (int i = blockIdx.x * NT + threadIdx.x; i < inner; i += gridDim.x * NT) {
        float acc[SAVP_EVAL_NMETRICS];
#pragma unroll
        for (int k = 0; k < SAVP_EVAL_NMETRICS; ++k) acc[k] = st.m[k].gsum[o + i];
        for (int s = 0; s < nv; ++s) {
            const float x = px[(long long)s * B * p_sb + i];
#pragma unroll
            for (int k = 0; k < SAVP_EVAL_NMETRICS; ++k) acc[k] = acc[k] + x;
        }
#pragma unroll
        for (int k = 0; k < SAVP_EVAL_NMETRICS; ++k) {
            st.m[k].gsum[o + i] = acc[k];
            if (smin[k] >= 0) st.m[k].gmin[o + i] = px[(long long)smin[k] * B * p_sb + i];
            if (smax[k] >= 0) st.m[k].gmax[o + i] = px[(long long)smax[k] * B * p_sb + i];
        }
    }
}

extern "C" int64_t savp_eval_fold_ws_floats(int32_t F, int32_t S, int32_t B, int32_t C) {
    if (F < 1 || S < 1 || B < 1 || C < 1) return 0;
    const int64_t fsb = (int64_t)F * S * B;
    return SAVP_EVAL_NMETRICS * fsb + fsb * C + 2 * SAVP_EVAL_NMETRICS * (int64_t)B;
}

extern "C" int savp_eval_fold_samples(void* stream, const float* target, int64_t t_st, int64_t t_sb, const float* pred, int64_t p_st,
                                      int64_t p_sb, int32_t F, int32_t T1, int32_t S, int32_t B, int32_t H, int32_t W, int32_t C,
                                      const int32_t* n_valid, const SavpEvalFoldState* states, float* ws, int64_t ws_floats) {
    if (!target || !pred || !n_valid || !states || !ws || F < 1 || T1 < F || S < 1 || B < 1 || H < SSIM_K || W < SSIM_K || C < 1)
        return SAVP_EINVAL;
    if (ws_floats < savp_eval_fold_ws_floats(F, S, B, C)) return SAVP_EINVAL;
    const int64_t SB = (int64_t)S * B, inner = (int64_t)H * W * C;
    if (SB * F * C > 0x7fffffff || inner > 0x7fffffff) return SAVP_EINVAL;
    const size_t lds = (size_t)2 * H * W * sizeof(float);
    const bool strips = lds > SSIM_LDS_BYTES;          // more than 8192 pixels: strips of whole rows
    const int R = ssim_strip_rows(W);
    if (strips && R < 1) return SAVP_EINVAL;
    EvalFoldStates st;
    for (int k = 0; k < SAVP_EVAL_NMETRICS; ++k) {
        const SavpEvalFoldState& m = states[k];
        if (!m.vmin || !m.vsum || !m.vmax || !m.gmin || !m.gsum || !m.gmax) return SAVP_EINVAL;
        st.m[k] = m;
    }
    hipStream_t sm = (hipStream_t)stream;
    float* met = ws;                                                    // [metric][F][S*B]
    float* part = ws + SAVP_EVAL_NMETRICS * F * SB;                     // [F][S*B][C]
    int* sel = (int*)(part + F * SB * C);                               // [metric][min | max][B]
    const float* fut = pred + (int64_t)(T1 - F) * p_st;                 // future frames of the prediction
    hipLaunchKernelGGL(fold_mse_kernel, dim3((unsigned)(F * SB)), dim3(NT), 0, sm, target, (long long)t_st, (long long)t_sb, fut,
                       (long long)p_st, (long long)p_sb, (int)SB, B, (int)inner, n_valid, met + SAVP_EVAL_PSNR * F * SB,
                       met + SAVP_EVAL_MSE * F * SB);
    if (strips)
        hipLaunchKernelGGL(fold_ssim_strip_kernel, dim3((unsigned)(F * SB * C)), dim3(NT), ssim_strip_lds(R, W), sm, target, (long long)t_st,
                           (long long)t_sb, fut, (long long)p_st, (long long)p_sb, (int)SB, B, H, W, C, n_valid, part);
    else
        hipLaunchKernelGGL(fold_ssim_kernel, dim3((unsigned)(F * SB * C)), dim3(NT), lds, sm, target, (long long)t_st, (long long)t_sb, fut,
                           (long long)p_st, (long long)p_sb, (int)SB, B, H, W, C, n_valid, part);
    hipLaunchKernelGGL(fold_select_kernel, dim3(1), dim3(NT), 0, sm, met, (const float*)part, F, (int)SB, B, C, n_valid, st, sel);
    unsigned gx = (unsigned)((inner + NT * 4 - 1) / (NT * 4));
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(fold_gather_kernel, dim3(gx, (unsigned)T1, (unsigned)B), dim3(NT), 0, sm, pred, (long long)p_st, (long long)p_sb, B,
                       (int)inner, n_valid, st, (const int*)sel);
    return LAUNCH_OK();
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// savp_eval_fold_metric: fold_select_kernel's phase 2 and fold_gather_kernel for ONE metric the caller computed per frame (LPIPS).
// ---------------------------------------------------------------------------------------------------------------------------------------
// single workgroup, one thread per b: eval_accumulate_kernel's update for s = 0 .. n_valid-1 in order; sel[0 | 1][b] = the last sample that
// replaced the running min / max (-1: none)
__global__ __launch_bounds__(NT) void fold_metric_select_kernel(const float* metric, int F, int SB, int B, const int* n_valid,
                                                                SavpEvalFoldState st, int* sel) {
    const int nv = *n_valid;
    for (int b = threadIdx.x; b < B; b += NT) {
        int smin_i = -1, smax_i = -1;
        for (int s = 0; s < nv; ++s) {
            const int n = s * B + b;
            float sm = 0.f, smin = 0.f, smax = 0.f;
            for (int t = 0; t < F; ++t) { sm += metric[t * SB + n]; smin += st.vmin[t * B + b]; smax += st.vmax[t * B + b]; }
            const bool lo = sm / (float)F < smin / (float)F, hi = sm / (float)F > smax / (float)F;
            for (int t = 0; t < F; ++t) {
                const float m = metric[t * SB + n];
                if (lo) st.vmin[t * B + b] = m;
                if (hi) st.vmax[t * B + b] = m;
                st.vsum[t * B + b] += m;
            }
            if (lo) smin_i = s;
            if (hi) smax_i = s;
        }
        sel[b] = smin_i;
        sel[B + b] = smax_i;
    }
}

// grid (x: slices of the frame, y: t, z: b), as fold_gather_kernel
__global__ __launch_bounds__(NT) void fold_metric_gather_kernel(const float* pred, long long p_st, long long p_sb, int B, int inner,
                                                                const int* n_valid, SavpEvalFoldState st, const int* sel) {
    const int t = blockIdx.y, b = blockIdx.z;
    const int nv = *n_valid;
    const size_t o = ((size_t)t * B + b) * inner;
    const float* px = pred + t * p_st + b * p_sb;
    const int smin = sel[b], smax = sel[B + b];
    for (int i = blockIdx.x * NT + threadIdx.x; i < inner; i += gridDim.x * NT) {
        float acc = st.gsum[o + i];
        for (int s = 0; s < nv; ++s) acc = acc + px[(long long)s * B * p_sb + i];
        st.gsum[o + i] = acc;
        if (smin >= 0) st.gmin[o + i] = px[(long long)smin * B * p_sb + i];
        if (smax >= 0) st.gmax[o + i] = px[(long long)smax * B * p_sb + i];
    }
}

extern "C" int savp_eval_fold_metric(void* stream, const float* metric, const float* pred, int64_t p_st, int64_t p_sb, int32_t F, int32_t T1,
                                     int32_t S, int32_t B, int32_t inner, const int32_t* n_valid, const SavpEvalFoldState* state,
                                     int32_t* sel) {
    if (!metric || !pred || !n_valid || !state || !sel || F < 1 || T1 < F || S < 1 || B < 1 || inner < 1) return SAVP_EINVAL;
    const SavpEvalFoldState st = *state;
    if (!st.vmin || !st.vsum || !st.vmax || !st.gmin || !st.gsum || !st.gmax) return SAVP_EINVAL;
    if ((int64_t)F * S * B > 0x7fffffff) return SAVP_EINVAL;
    hipStream_t sm = (hipStream_t)stream;
    hipLaunchKernelGGL(fold_metric_select_kernel, dim3(1), dim3(NT), 0, sm, metric, F, S * B, B, n_valid, st, sel);
    unsigned gx = (unsigned)((inner + NT * 4 - 1) / (NT * 4));
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(fold_metric_gather_kernel, dim3(gx, (unsigned)T1, (unsigned)B), dim3(NT), 0, sm, pred, (long long)p_st,
                       (long long)p_sb, B, inner, n_valid, st, (const int*)sel);
    return LAUNCH_OK();
}

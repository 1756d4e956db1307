// input_resize.hip -- the dataset hyper-parameters crop_size / scale_size of the reference's input pipeline
// (base_dataset.py:159-184 decode_and_preprocess_image) on the device, fused with what u8_frames_kernel (util_ops.hip) does:
//
//     uint8 [B, T, Hs, Ws, C]  --centre crop or zero pad to crop x crop--  --resize to S x S--  * (1/255)  ->  float32 [T, B, S, S, C]
//
//  * crop or pad: tf.image.resize_image_with_crop_or_pad.  Per axis, a longer source starts at (dim - crop) / 2 (the odd pixel is dropped at
//    the far end); a shorter one gets (crop - dim) / 2 zeros in front and the rest behind.  The zeros are part of the image that is resized.
//  * crop <  S: tf.image.resize_images(BILINEAR) of TF1 (align_corners=False, no half-pixel offset): output index o reads the source
//    position o * crop / S; top = floor, bottom = min(top + 1, crop - 1), weights (1 - frac, frac).
//  * crop >  S: ResizeMethod.AREA (resize_area, align_corners=False): output cell o covers [o * crop / S, (o + 1) * crop / S); every source
//    pixel contributes with the length of its overlap with that interval, the sum is divided by (crop / S)^2.
//  * crop == S: the cropped window unchanged.
//
// Arithmetic.  Both methods are separable, and with positions taken from the integers (o * crop / S and o * crop % S, not from a rounded
// float scale) every weight is an integer count of 1/S per axis.  The kernel therefore accumulates sum = SUM wy * wx * pixel in uint32 --
// exact, at most 255 * 4096^2 < 2^32 -- and rounds at the end only: (float)sum / den^2 * (float)(1/255), den = S (bilinear) or crop (area).
// A pixel whose weights fall onto one source value (a copy, the even outputs of a 2x enlargement, a constant image) comes out as that
// value * (float)(1/255) exactly, bit-equal to u8_frames_kernel.  Hence the limit crop, S <= 4096.  crop == S runs the bilinear
// instantiation (all the weight on the first tap).
//
// One thread per 16-byte piece of an output frame (4 consecutive floats along W * C, which may straddle pixels and rows), float4 stores
// coalesced over the wave; a frame whose size is not a multiple of 4 floats takes the one-float-per-thread instantiation.  The uint8 taps
// are gathered straight from global memory (a frame is a few KiB .. 48 KiB: L1 / L2 hits), one byte load per tap and channel; that load
// count, not the fp32 store stream, is what the kernel's time follows (profiles/input_resize.md).  No load is guarded: a tap in the zero
// padding reads a clamped address and has its weight cleared.  Every output element is written, the padding zeros included.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define NT 256
#define RESIZE_MAX 4096          // crop, S: keeps the integer weighted sum (at most 255 * 4096^2) inside 32 bits
#define SRC_MAX 16384            // Hs, Ws
#define CH_MAX 64                // C: a source row is below 2^24 elements
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

// n / d and n % d for 0 <= n < 2^30, 1 <= d < 2^24, quotient < 2^20, with inv = 1.0f / d from the host: the float estimate is within one
// of the quotient ((float)n and inv carry 2^-24 relative error each, the quotient is small), the integer remainder corrects it.  Replaces
// the ~40-instruction 32-bit division sequence (worth a third of the bilinear kernel's time, profiles/input_resize.md).
__device__ __forceinline__ void divmod(int n, int d, float inv, int& q, int& r) {
    q = (int)((float)n * inv);
    r = n - (int)__umul24(q, d);
    if (r < 0) { --q; r += d; }
    else if (r >= d) { ++q; r -= d; }
}

struct ResizeGeom {
    int Hs, Ws, C, crop, S, oy, ox;          // oy / ox: source row / column of the crop window's origin (negative: zero padding in front)
    float inv_S, inv_C, inv_row, inv_den;    // 1 / S, 1 / C, 1 / (S * C), 1 / den^2 with den = S (crop <= S) or crop (area)
};

// Index `i` of the crop-long axis (clamped to crop - 1 like TF's bottom / right index) as an element offset into the source frame, `stride`
// elements per step; a position in the zero padding keeps an in-bounds offset and loses its weight instead, so no load is ever guarded.
__device__ __forceinline__ unsigned tap(int i, int crop, int origin, int dim, int stride, unsigned& w) {
    const int a = min(i, crop - 1) + origin;
    if ((unsigned)a >= (unsigned)dim) w = 0;
    return __umul24(min(max(a, 0), dim - 1), stride);
}

// crop <= S: the two taps of one axis of the legacy bilinear resize for output index o (crop == S: all the weight on the first one).
struct Taps2 { unsigned o0, o1, w0, w1; };
__device__ __forceinline__ Taps2 taps2(int o, const ResizeGeom& g, int origin, int dim, int stride) {
    int i0, r;
    divmod(__umul24(o, g.crop), g.S, g.inv_S, i0, r);               // r / S = the lerp fraction
    Taps2 t;
    t.w0 = g.S - r; t.w1 = r;
    t.o0 = tap(i0, g.crop, origin, dim, stride, t.w0);
    t.o1 = tap(i0 + 1, g.crop, origin, dim, stride, t.w1);
    return t;
}

// crop > S: the source indices i0 .. i0 + n - 1 that the cell [lo, lo + crop) of output index o overlaps (units of 1/S of a source pixel)
struct Span { int i0, n, lo; };
__device__ __forceinline__ Span span(int o, const ResizeGeom& g) {
    Span s;
    int rem, last;
    s.lo = __umul24(o, g.crop);
    divmod(s.lo, g.S, g.inv_S, s.i0, rem);
    divmod(s.lo + g.crop + g.S - 1, g.S, g.inv_S, last, rem);
    s.n = last - s.i0;
    return s;
}
__device__ __forceinline__ unsigned overlap(int i, const Span& s, const ResizeGeom& g) {
    return (unsigned)(min((int)__umul24(i + 1, g.S), s.lo + g.crop) - max((int)__umul24(i, g.S), s.lo));
}

template <bool AREA, bool VEC>
__global__ __launch_bounds__(NT) void u8_frames_resize_kernel(const uint8_t* __restrict__ in, float* __restrict__ out, int B, int T, ResizeGeom g) {
    constexpr int PER = VEC ? 4 : 1;
    const int t = blockIdx.y, b = blockIdx.z;
    const uint8_t* src = in + ((long long)b * T + t) * ((long long)g.Hs * g.Ws * g.C);
    const int F = g.S * g.S * g.C, row = g.S * g.C, src_row = g.Ws * g.C;
    float* dst = out + ((long long)t * B + b) * (long long)F;
    const float scale = (float)(1.0 / 255.0);
    const float den = AREA ? (float)(g.crop * g.crop) : (float)(g.S * g.S);
    for (int i = blockIdx.x * NT + threadIdx.x; i < F / PER; i += gridDim.x * NT) {
        int y, x, c, rem;
        divmod(i * PER, row, g.inv_row, y, rem);
        divmod(rem, g.C, g.inv_C, x, c);
        Taps2 ty = {}, tx = {};
        Span sy = {}, sx = {};
        bool newy = true, newx = true;
        float v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            unsigned sum = 0;                                            // exact: every factor below is under 2^24, every sum under 2^32
            if (!AREA) {
                if (newy) ty = taps2(y, g, g.oy, g.Hs, src_row);
                if (newx) tx = taps2(x, g, g.ox, g.Ws, g.C);
                const unsigned l = tx.o0 + c, r = tx.o1 + c;              // 32-bit offsets from the block-uniform frame pointer
                const unsigned top = __umul24(tx.w0, src[ty.o0 + l]) + __umul24(tx.w1, src[ty.o0 + r]);
                const unsigned bot = __umul24(tx.w0, src[ty.o1 + l]) + __umul24(tx.w1, src[ty.o1 + r]);
                sum = __umul24(ty.w0, top) + __umul24(ty.w1, bot);
            } else {
                if (newy) sy = span(y, g);
                if (newx) sx = span(x, g);
                for (int ky = 0; ky < sy.n; ++ky) {
                    unsigned wy = overlap(sy.i0 + ky, sy, g);
                    const unsigned line0 = tap(sy.i0 + ky, g.crop, g.oy, g.Hs, src_row, wy) + c;
                    unsigned line = 0;
                    for (int kx = 0; kx < sx.n; ++kx) {
                        unsigned wx = overlap(sx.i0 + kx, sx, g);
                        const unsigned o = tap(sx.i0 + kx, g.crop, g.ox, g.Ws, g.C, wx);
                        line += __umul24(wx, src[line0 + o]);
                    }
                    sum += __umul24(wy, line);
                }
            }
            // (float)sum / den by one Newton step on the host's reciprocal: the fma leaves the exact residual, so a sum that is a multiple
            // of den (one source value carrying all the weight: a copy, the even outputs of a 2x enlargement) gives that value exactly
            const float fs = (float)sum;
            const float q = fs * g.inv_den;
            v[k] = fmaf(fmaf(-q, den, fs), g.inv_den, q) * scale;
            newy = newx = false;
            if (++c == g.C) {
                c = 0; newx = true;
                if (++x == g.S) { x = 0; ++y; newy = true; }
            }
        }
        if (VEC) reinterpret_cast<float4*>(dst)[i] = make_float4(v[0], v[1 % PER], v[2 % PER], v[3 % PER]);
        else dst[i] = v[0];
    }
}

template <bool AREA>
static void launch_resize(hipStream_t st, bool vec, dim3 grid, const uint8_t* in, float* out, int B, int T, const ResizeGeom& g) {
    if (vec) hipLaunchKernelGGL((u8_frames_resize_kernel<AREA, true>), grid, dim3(NT), 0, st, in, out, B, T, g);
    else hipLaunchKernelGGL((u8_frames_resize_kernel<AREA, false>), grid, dim3(NT), 0, st, in, out, B, T, g);
}

extern "C" int savp_u8_frames_resize_f32(void* stream, const uint8_t* in, float* out, int32_t B, int32_t T, int32_t Hs, int32_t Ws, int32_t C,
                                         int32_t crop, int32_t S) {
    if (!in || !out || B < 1 || T < 1 || Hs < 1 || Ws < 1 || C < 1 || crop < 1 || S < 1) return SAVP_EINVAL;
    if (crop > RESIZE_MAX || S > RESIZE_MAX || B > 65535 || T > 65535) return SAVP_EINVAL;
    if (Hs > SRC_MAX || Ws > SRC_MAX || C > CH_MAX) return SAVP_EINVAL;              // offsets and 24-bit multiplies: see divmod / tap
    if ((long long)Hs * Ws * C > 0x3fffffffLL || (long long)S * S * C > 0x3fffffffLL) return SAVP_EINVAL;
    if ((((uintptr_t)out) & 3) != 0) return SAVP_EINVAL;
    const long long F = (long long)S * S * C;
    const bool vec = (F % 4) == 0 && (((uintptr_t)out) & 15) == 0;
    ResizeGeom g;
    g.Hs = Hs; g.Ws = Ws; g.C = C; g.crop = crop; g.S = S;
    // source offset of the crop window's origin: positive = crop, negative = zero padding in front (resize_image_with_crop_or_pad)
    g.oy = Hs > crop ? (Hs - crop) / 2 : -((crop - Hs) / 2);
    g.ox = Ws > crop ? (Ws - crop) / 2 : -((crop - Ws) / 2);
    const float den = crop < S ? (float)S : (float)crop;
    g.inv_S = 1.0f / (float)S; g.inv_C = 1.0f / (float)C; g.inv_row = 1.0f / (float)(S * C); g.inv_den = 1.0f / (den * den);
    const long long items = vec ? F / 4 : F;
    unsigned gx = (unsigned)((items + NT - 1) / NT);
    if (gx > 1024) gx = 1024;
    const dim3 grid(gx, (unsigned)T, (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (crop <= S) launch_resize<false>(st, vec, grid, in, out, B, T, g);
    else launch_resize<true>(st, vec, grid, in, out, B, T, g);
    return LAUNCH_OK();
}

// jpeg_decode.hip -- the device half of JPEG decoding: what tf.image.decode_jpeg (base_dataset.py:161-162, ucf101_dataset.py:48,52) does after
// the Huffman bitstream, for the coefficients that savp_jpeg_entropy_decode (libsavp_io.so, include/savp_io.h) hands over:
//
//     int16 coef [N, total_blocks, 64] x uint16 qtab [N, C, 64]  --dequantise, IDCT-->  uint8 planes (workspace)
//                                                                 --crop, fancy upsampling, YCbCr -> RGB, window-->  uint8 out [N, out_h, out_w, C]
//
// The arithmetic is the integer one of libjpeg / libjpeg-turbo with its defaults (jidctint.c "islow", jdsample.c fancy upsampling,
// jdcolor.c), so the result EQUALS theirs sample for sample:
//   * IDCT: CONST_BITS 13, PASS1_BITS 2; columns first, descaled by 11, then rows, descaled by 18, + 128, clamped to 0..255.
//   * planes are cropped to ceil(W * h / hmax) x ceil(H * v / vmax) before upsampling; a neighbour outside replicates the edge sample.
//   * h2v1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2.
//     h2v2: cs[i] = 3 cur[i] + nb[i] (nb = row r-1 for output row 2r, r+1 for 2r+1); out[2i] = (3 cs[i] + cs[i-1] + 8) >> 4,
//     out[2i+1] = (3 cs[i] + cs[i+1] + 7) >> 4.  With the edge replicated these are libjpeg's special first / last columns as well.
//     libjpeg takes the fancy upsamplers only when the chroma plane is more than 2 samples wide; a narrower one is replicated (box).
//   * YCbCr -> RGB in 16.16 fixed point, rounding constant 32768 (on the Cb term of G).
//
// Two launches.  savp_jpeg_idct_kernel: 8 threads per 8x8 block, 32 blocks per workgroup.  Thread r loads row r of the block with one
// 16-byte load (a wave reads 1 KiB contiguous), dequantises, and the block is transposed through LDS twice (row stride 9 words): column
// pass, row pass, one 8-byte store per thread into the component plane.  savp_jpeg_colour_kernel: one thread per 4 output pixels of a row;
// 12 bytes leave as three dword stores when the row length allows it.  The planes make one round trip through the caller's workspace
// (1.5 B / pixel written and read again at 4:2:0, on top of 3 B of coefficients in and 3 B out).
//
// Multiplies.  For streams an encoder can produce (|coefficient| <= 2^11 .. 2^12 after dequantisation) every multiplicand of both passes is
// below 2^23 in magnitude, so the 24-bit multiply (full rate on CDNA, v_mul_lo_u32 is quarter rate) returns the same low 32 bits as a 32-bit
// one; the black / white and primary-colour fixtures at quality 100 drive every clamp and pin this.  A stream whose coefficients are far
// outside that range decodes to clamped samples that need not be libjpeg's (whose own arithmetic is 64-bit there).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define NT 256
#define BLOCKS_PER_WG 32
#define LDS_ROW 9                 // words per block row in LDS: the transposed reads of the 8 blocks of a wave spread over the banks
#define JPEG_DIM_MAX 65535
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

struct JpegGeom {
    int width, height, C, mode;                   // mode 0: one component or 4:4:4, 1: h2v1, 2: h2v2
    int blocks_w[3], block_offset[3], total_blocks;
    int cw, ch;                                   // cropped chroma plane
    int out_h, out_w, quads;                      // quads = ceil(out_w / 4)
    float inv_quads;
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jidctint.c jpeg_idct_islow, one dimension, without the final descale
__device__ __forceinline__ void idct_1d(const int (&in)[8], int (&out)[8]) {
    int z1 = __mul24(in[2] + in[6], 4433);
    const int tmp2 = z1 - __mul24(in[6], 15137);
    const int tmp3 = z1 + __mul24(in[2], 6270);
    const int tmp0 = (in[0] + in[4]) << 13;
    const int tmp1 = (in[0] - in[4]) << 13;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    int t0 = in[7], t1 = in[5], t2 = in[3], t3 = in[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = __mul24(z3 + z4, 9633);
    t0 = __mul24(t0, 2446); t1 = __mul24(t1, 16819); t2 = __mul24(t2, 25172); t3 = __mul24(t3, 12299);
    z1 = __mul24(z1, -7373); z2 = __mul24(z2, -20995);
    z3 = __mul24(z3, -16069) + z5; z4 = __mul24(z4, -3196) + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    out[0] = tmp10 + t3; out[7] = tmp10 - t3;
    out[1] = tmp11 + t2; out[6] = tmp11 - t2;
    out[2] = tmp12 + t1; out[5] = tmp12 - t1;
    out[3] = tmp13 + t0; out[4] = tmp13 - t0;
}

__global__ __launch_bounds__(NT) void savp_jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qtab,
                                                            uint8_t* __restrict__ planes, int N, JpegGeom g) {
    __shared__ int lds[BLOCKS_PER_WG][8 * LDS_ROW];
    const int blk = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int bi = blockIdx.x * BLOCKS_PER_WG + blk;
    const bool valid = bi < g.total_blocks;
    int c = 0;
    if (g.C == 3) c = bi >= g.block_offset[2] ? 2 : (bi >= g.block_offset[1] ? 1 : 0);
    const int local = bi - g.block_offset[c], bw = g.blocks_w[c];
    const int by = local / bw, bx = local - by * bw;
    int* mine = lds[blk];
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        if (valid) {
            const int4 raw = *reinterpret_cast<const int4*>(coef + ((long long)n * g.total_blocks + bi) * 64 + r * 8);
            const uint4 q = *reinterpret_cast<const uint4*>(qtab + ((long long)n * g.C + c) * 64 + r * 8);
            const int cw[4] = {raw.x, raw.y, raw.z, raw.w};
            const unsigned qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                     // two int16 / uint16 per word, little endian
                mine[r * LDS_ROW + 2 * j] = __mul24((int)(short)(cw[j] & 0xffff), (int)(qw[j] & 0xffff));
                mine[r * LDS_ROW + 2 * j + 1] = __mul24(cw[j] >> 16, (int)(qw[j] >> 16));
            }
        }
        __syncthreads();
        if (valid) {                                                          // pass 1: column r
            int in[8], out[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) in[k] = mine[k * LDS_ROW + r];
            idct_1d(in, out);
#pragma unroll
            for (int k = 0; k < 8; ++k) mine[k * LDS_ROW + r] = descale(out[k], 11);
        }
        __syncthreads();
        if (valid) {                                                          // pass 2: row r
            int in[8], out[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) in[k] = mine[r * LDS_ROW + k];
            idct_1d(in, out);
            unsigned w[2] = {0, 0};
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k >> 2] |= (unsigned)min(max(descale(out[k], 18) + 128, 0), 255) << (8 * (k & 3));
            uint8_t* dst = planes + (long long)n * g.total_blocks * 64 + (long long)g.block_offset[c] * 64 + (long long)(by * 8 + r) * (bw * 8) + bx * 8;
            *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
        }
        __syncthreads();
    }
}

// one upsampled chroma sample at full-resolution position (y, x); p: the component's plane, stride its padded row length
template <int MODE>
__device__ __forceinline__ int chroma(const uint8_t* __restrict__ p, int stride, int cw, int ch, bool fancy, int y, int x) {
    if (MODE == 0) return p[y * stride + x];
    const int i = x >> 1, odd = x & 1;
    const int nb = odd ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (MODE == 1) {
        const uint8_t* row = p + y * stride;
        const int s = row[i];
        return fancy ? (3 * s + row[nb] + 1 + odd) >> 2 : s;
    }
    const int r = y >> 1;
    const uint8_t* cur = p + r * stride;
    if (!fancy) return cur[i];
    const uint8_t* other = p + ((y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0)) * stride;
    const int cs = 3 * cur[i] + other[i], csn = 3 * cur[nb] + other[nb];
    return (3 * cs + csn + 8 - odd) >> 4;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

template <int MODE, bool COLOUR, bool VEC>
__global__ __launch_bounds__(NT) void savp_jpeg_colour_kernel(const uint8_t* __restrict__ planes, const int32_t* __restrict__ window,
                                                              uint8_t* __restrict__ out, int N, JpegGeom g) {
    const int items = g.out_h * g.quads;
    const bool fancy = g.cw > 2;
    const int s0 = g.blocks_w[0] * 8, s1 = COLOUR ? g.blocks_w[1] * 8 : 0;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const uint8_t* py = planes + (long long)n * g.total_blocks * 64;
        const uint8_t* pcb = py + (long long)g.block_offset[COLOUR ? 1 : 0] * 64;
        const uint8_t* pcr = py + (long long)g.block_offset[COLOUR ? 2 : 0] * 64;
        int y0 = 0, x0 = 0;
        if (window) {                                                         // the values live on the device: clamped, never trusted
            y0 = min(max(window[2 * n], 0), g.height - g.out_h);
            x0 = min(max(window[2 * n + 1], 0), g.width - g.out_w);
        }
        uint8_t* dst = out + (long long)n * g.out_h * g.out_w * g.C;
        for (int i = blockIdx.x * NT + threadIdx.x; i < items; i += gridDim.x * NT) {
            int oy = (int)((float)i * g.inv_quads);                           // i / quads: float estimate, corrected by the integer remainder
            int rem = i - oy * g.quads;
            if (rem < 0) { --oy; rem += g.quads; } else if (rem >= g.quads) { ++oy; rem -= g.quads; }
            const int ox = rem * 4, y = y0 + oy;
            unsigned px[4][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                px[k][0] = px[k][1] = px[k][2] = 0;
                if (!VEC && ox + k >= g.out_w) continue;
                const int x = x0 + ox + k;
                const int Y = py[y * s0 + x];
                if (!COLOUR) { px[k][0] = (unsigned)Y; continue; }
                const int cb = chroma<MODE>(pcb, s1, g.cw, g.ch, fancy, y, x) - 128;
                const int cr = chroma<MODE>(pcr, s1, g.cw, g.ch, fancy, y, x) - 128;
                px[k][0] = clamp255(Y + ((91881 * cr + 32768) >> 16));                       // FIX(1.402)
                px[k][1] = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));         // FIX(0.34414), FIX(0.71414)
                px[k][2] = clamp255(Y + ((116130 * cb + 32768) >> 16));                      // FIX(1.772)
            }
            uint8_t* o = dst + ((long long)oy * g.out_w + ox) * g.C;
            if (VEC && COLOUR) {
                unsigned* o32 = reinterpret_cast<unsigned*>(o);
                o32[0] = px[0][0] | px[0][1] << 8 | px[0][2] << 16 | px[1][0] << 24;
                o32[1] = px[1][1] | px[1][2] << 8 | px[2][0] << 16 | px[2][1] << 24;
                o32[2] = px[2][2] | px[3][0] << 8 | px[3][1] << 16 | px[3][2] << 24;
            } else if (VEC) {
                *reinterpret_cast<unsigned*>(o) = px[0][0] | px[1][0] << 8 | px[2][0] << 16 | px[3][0] << 24;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (ox + k < g.out_w)
                        for (int c = 0; c < (COLOUR ? 3 : 1); ++c) o[k * (COLOUR ? 3 : 1) + c] = (uint8_t)px[k][c];
            }
        }
    }
}

// The argument checks mirror what the host decoder accepts (csrc_host/jpeg_decode.cpp); returns the geometry the kernels use.
static int check_args(const SavpJpegArgs* a, JpegGeom& g) {
    if (!a || a->N < 1 || a->width < 1 || a->height < 1 || a->width > JPEG_DIM_MAX || a->height > JPEG_DIM_MAX) return SAVP_EINVAL;
    if (a->components != 1 && a->components != 3) return SAVP_EINVAL;
    const int C = a->components;
    int mode = 0;
    if (C == 1) {
        if (a->h[0] != 1 || a->v[0] != 1) return SAVP_EINVAL;
    } else {
        if (a->h[1] != 1 || a->v[1] != 1 || a->h[2] != 1 || a->v[2] != 1) return SAVP_EINVAL;
        if (a->h[0] == 1 && a->v[0] == 1) mode = 0;
        else if (a->h[0] == 2 && a->v[0] == 1) mode = 1;
        else if (a->h[0] == 2 && a->v[0] == 2) mode = 2;
        else return SAVP_EINVAL;
    }
    const int hmax = a->h[0], vmax = a->v[0];
    const int mx = (a->width + 8 * hmax - 1) / (8 * hmax), my = (a->height + 8 * vmax - 1) / (8 * vmax);
    long long off = 0;
    for (int c = 0; c < C; ++c) {
        if (a->blocks_w[c] != mx * a->h[c] || a->blocks_h[c] != my * a->v[c] || a->block_offset[c] != off) return SAVP_EINVAL;
        off += (long long)a->blocks_w[c] * a->blocks_h[c];
    }
    if (off != a->total_blocks || off > (1 << 24)) return SAVP_EINVAL;
    if (a->window) {
        if (a->out_h < 1 || a->out_w < 1 || a->out_h > a->height || a->out_w > a->width) return SAVP_EINVAL;
    } else if (a->out_h != a->height || a->out_w != a->width) return SAVP_EINVAL;
    g.width = a->width; g.height = a->height; g.C = C; g.mode = mode;
    for (int c = 0; c < 3; ++c) { g.blocks_w[c] = c < C ? a->blocks_w[c] : 0; g.block_offset[c] = c < C ? a->block_offset[c] : 0; }
    g.total_blocks = a->total_blocks;
    g.cw = (a->width + hmax - 1) / hmax; g.ch = (a->height + vmax - 1) / vmax;
    g.out_h = a->out_h; g.out_w = a->out_w; g.quads = (a->out_w + 3) / 4;
    g.inv_quads = 1.0f / (float)g.quads;
    if ((long long)g.out_h * g.quads > 0x3fffffffLL) return SAVP_EINVAL;
    return SAVP_OK;
}

extern "C" int64_t savp_jpeg_workspace_bytes(const SavpJpegArgs* a) {
    JpegGeom g;
    if (check_args(a, g) != SAVP_OK) return -1;
    return (int64_t)a->N * a->total_blocks * 64;                              // the component planes, one byte per sample
}

template <int MODE, bool COLOUR>
static void launch_colour(hipStream_t st, bool vec, dim3 grid, const uint8_t* planes, const int32_t* window, uint8_t* out, int N, const JpegGeom& g) {
    if (vec) hipLaunchKernelGGL((savp_jpeg_colour_kernel<MODE, COLOUR, true>), grid, dim3(NT), 0, st, planes, window, out, N, g);
    else hipLaunchKernelGGL((savp_jpeg_colour_kernel<MODE, COLOUR, false>), grid, dim3(NT), 0, st, planes, window, out, N, g);
}

extern "C" int savp_jpeg_decode_u8(void* stream, const SavpJpegArgs* a) {
    JpegGeom g;
    const int rc = check_args(a, g);
    if (rc != SAVP_OK) return rc;
    if (!a->coef || !a->qtab || !a->out || !a->ws) return SAVP_EINVAL;
    if ((((uintptr_t)a->coef) & 15) || (((uintptr_t)a->qtab) & 15) || (((uintptr_t)a->ws) & 7) || (a->window && (((uintptr_t)a->window) & 3))) return SAVP_EINVAL;
    if (a->ws_bytes < (int64_t)a->N * a->total_blocks * 64) return SAVP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const unsigned gy = (unsigned)(a->N < 65535 ? a->N : 65535);
    uint8_t* planes = (uint8_t*)a->ws;
    hipLaunchKernelGGL(savp_jpeg_idct_kernel, dim3((unsigned)((g.total_blocks + BLOCKS_PER_WG - 1) / BLOCKS_PER_WG), gy), dim3(NT), 0, st,
                       a->coef, a->qtab, planes, a->N, g);
    if (hipGetLastError() != hipSuccess) return SAVP_ELAUNCH;
    const bool vec = (a->out_w % 4) == 0 && (((uintptr_t)a->out) & 3) == 0;
    const long long items = (long long)g.out_h * g.quads;
    unsigned gx = (unsigned)((items + NT - 1) / NT);
    if (gx > 4096) gx = 4096;
    const dim3 grid(gx, gy);
    if (g.C == 1) launch_colour<0, false>(st, vec, grid, planes, a->window, a->out, a->N, g);
    else if (g.mode == 0) launch_colour<0, true>(st, vec, grid, planes, a->window, a->out, a->N, g);
    else if (g.mode == 1) launch_colour<1, true>(st, vec, grid, planes, a->window, a->out, a->N, g);
    else launch_colour<2, true>(st, vec, grid, planes, a->window, a->out, a->N, g);
    return LAUNCH_OK();
}

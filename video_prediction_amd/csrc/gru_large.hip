// gru_large.hip -- the instance-norm gate blocks of Conv2DGRUCell (gru.hip) for planes of ANY size: savp_convgru_large_*.
// gru.hip holds a whole plane in registers (one workgroup = one sample x 4 channels, H*W <= 1024).  Here every block is two launches over
// chunks of pixels, in the manner of inorm_stats_kernel / inorm_apply_kernel (norm_lstm.hip):
//   pass 1 (sums)  : a workgroup covers `chunk` pixels x a slab of <= 256 of the F channels of one sample; a thread owns 4 channels and walks
//                    the chunk's pixel rows, so a wave reads whole channel-last rows with 16-byte accesses.  The workgroup's sums are folded
//                    over its pixel rows in float64 and STORED to the caller's workspace ws[n][chunk][4][F] (float64): no atomics, and the
//                    workspace needs no clearing.
//   pass 2 (apply) : the same grid; every workgroup folds the sample's chunk partials in chunk order (float64) and writes its pixels.
// The forward sums are taken around the sample's first pixel (a shifted variance, finished in float64); the backward sums are sum dz and
// sum dz*xhat, which are also dbeta and dgamma.  Activations are recomputed in both passes; no normalised tensor is stored.  Every result
// is a function of the operands alone (fixed summation order), except that several samples add to dgamma / dbeta with float64 atomics of
// fp32-rounded per-sample totals, like every other norm of the step.
// The statistics are always computed here: there is no stats_ready shortcut from the producing convolution's epilogue.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define NT 256
#define GL_SLAB 256                   // channels of F per workgroup
#define GL_K 4                        // float64 partials per channel of F in the workspace
#define GL_MAX_CHUNKS 64              // the apply pass folds this many partials per value at the most
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_(float x) {
    float e = __expf(-2.f * fabsf(x));
    return copysignf((1.f - e) / (1.f + e), x);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void unpack(const float4 v, float (&o)[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ float4 pack(const float (&o)[4]) { return make_float4(o[0], o[1], o[2], o[3]); }

struct GruLP {
    int N, HW, F, chunk, nchunks;
    float eps;
    const float* pre;                                    // gates stage: [N,HW,2F]; output stage: [N,HW,F]
    const float* h; long long h_sn, h_sp;
    const float *gamma, *beta;
    float *mean, *rstd;                                  // [N,2F] / [N,F]
    float* u;                                            // [N,HW,F]
    float* rh; long long rh_sn, rh_sp;
    int nout; float* out[4]; long long o_sn[4], o_sp[4];
    int ndy; const float* dy[4]; long long dy_sn[4], dy_sp[4];
    float* dpre;
    float* du;
    float* dh; long long dh_sn, dh_sp;
    const float* drh; long long drh_sn, drh_sp;
    double *dgamma, *dbeta;
    double* ws;                                          // [N][nchunks][GL_K][F]
};

// thread geometry of every kernel: c4 = this thread's 4-channel group inside the slab, prow = its pixel row, `on` = it has work
#define GL_GEOM()                                                                                                     \
    const int F = p.F, FS = F < GL_SLAB ? F : GL_SLAB, F4s = FS >> 2;                                                 \
    const int c4 = threadIdx.x % F4s, prow = threadIdx.x / F4s, rows = NT / F4s;                                      \
    const int n = blockIdx.y, slab0 = blockIdx.z * GL_SLAB, c0 = slab0 + c4 * 4;                                      \
    const bool on = prow < rows && c0 < F;                                                                            \
    const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk)

// The apply passes walk their pixel rows two at a time and issue every load of a trip before its first store (the destinations may alias
// the sources as far as the compiler knows, so a one-pixel loop exposes a memory round trip per pixel).  A trip's second row repeats the
// first when it lies past the chunk (`two` false): loaded again, never stored.
#define GL_TRIP()                                                                                                     \
    const bool two = px0 + rows < p1;                                                                                 \
    const int pxs[2] = {px0, two ? px0 + rows : px0}

// pass 1 epilogue: v[k*4+e] = this thread's sum k of channel c0+e -> ws[n][chunk][k][c], folded over the pixel rows in float64, row order
template <int K>
__device__ __forceinline__ void gl_store_partials(const GruLP& p, const float (&v)[K * 4], float* sh, int FS, int c4, int prow, int rows,
                                                  int n, int slab0) {
    if (prow < rows) {
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) sh[(prow * K + k) * FS + c4 * 4 + e] = v[k * 4 + e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * FS; i += NT) {
        double t = 0.0;
        for (int r = 0; r < rows; ++r) t += (double)sh[r * K * FS + i];
        const int k = i / FS, cc = slab0 + i % FS;
        if (cc < p.F) p.ws[(((long long)n * p.nchunks + blockIdx.x) * GL_K + k) * p.F + cc] = t;
    }
}

// pass 2 prologue: tot[k*FS + c] = the sample's sum k of channel slab0+c over all chunks, chunk order
template <int K>
__device__ __forceinline__ void gl_fold(const GruLP& p, double* tot, int FS, int n, int slab0) {
    for (int i = threadIdx.x; i < K * FS; i += NT) {
        const int k = i / FS, cc = slab0 + i % FS;
        double t = 0.0;
        if (cc < p.F) {
            const double* w = p.ws + ((long long)n * p.nchunks * GL_K + k) * p.F + cc;
#pragma unroll 4
            for (int ch = 0; ch < p.nchunks; ++ch) t += w[(long long)ch * GL_K * p.F];
        }
        tot[i] = t;
    }
    __syncthreads();
}

// mean and rstd of one channel from its shifted sums (around `shift`), finished in float64
__device__ __forceinline__ void gl_moments(double s, double q, float shift, int HW, float eps, float& mean, float& rstd) {
    const double inv = 1.0 / (double)HW, ms = s * inv;
    double var = q * inv - ms * ms;
    if (var < 0.0) var = 0.0;
    mean = (float)((double)shift + ms);
    rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// ---- gates stage forward ---------------------------------------------------------------------------------------------------------
// sums of pre - pre[pixel 0]: k = 0 sum r, 1 sum of squares r, 2 sum u, 3 sum of squares u
__global__ __launch_bounds__(NT) void grul_gates_fwd_sums(GruLP p) {
    __shared__ float sh[NT * 16];
    GL_GEOM();
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
        float kr[4], ku[4];
        unpack(ld4(gp), kr); unpack(ld4(gp + F), ku);
        for (int px = p0 + prow; px < p1; px += rows) {
            float a[4], b[4];
            unpack(ld4(gp + (long long)px * 2 * F), a); unpack(ld4(gp + (long long)px * 2 * F + F), b);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dr = a[e] - kr[e], du = b[e] - ku[e];
                v[e] += dr; v[4 + e] += dr * dr; v[8 + e] += du; v[12 + e] += du * du;
            }
        }
    }
    gl_store_partials<4>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void grul_gates_fwd_apply(GruLP p) {
    __shared__ double tot[4 * GL_SLAB];
    GL_GEOM();
    gl_fold<4>(p, tot, FS, n, slab0);
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
    float kr[4], ku[4], mu[8], rs[8], ga[8], be[8];
    unpack(ld4(gp), kr); unpack(ld4(gp + F), ku);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = c4 * 4 + e;
        gl_moments(tot[c], tot[FS + c], kr[e], p.HW, p.eps, mu[e], rs[e]);
        gl_moments(tot[2 * FS + c], tot[3 * FS + c], ku[e], p.HW, p.eps, mu[4 + e], rs[4 + e]);
        ga[e] = p.gamma[c0 + e]; ga[4 + e] = p.gamma[F + c0 + e];
        be[e] = p.beta[c0 + e]; be[4 + e] = p.beta[F + c0 + e];
    }
    if (blockIdx.x == 0 && prow == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            p.mean[(long long)n * 2 * F + c0 + e] = mu[e]; p.mean[(long long)n * 2 * F + F + c0 + e] = mu[4 + e];
            p.rstd[(long long)n * 2 * F + c0 + e] = rs[e]; p.rstd[(long long)n * 2 * F + F + c0 + e] = rs[4 + e];
        }
    }
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        GL_TRIP();
        float a[2][4], b[2][4], hv[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unpack(ld4(gp + (long long)pxs[j] * 2 * F), a[j]); unpack(ld4(gp + (long long)pxs[j] * 2 * F + F), b[j]);
            unpack(ld4(p.h + (long long)n * p.h_sn + (long long)pxs[j] * p.h_sp + c0), hv[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float r[4], u[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r[e] = sigm((a[j][e] - mu[e]) * rs[e] * ga[e] + be[e]) * hv[j][e];
                u[e] = sigm((b[j][e] - mu[4 + e]) * rs[4 + e] * ga[4 + e] + be[4 + e]);
            }
            st4(p.rh + (long long)n * p.rh_sn + (long long)pxs[j] * p.rh_sp + c0, pack(r));
            st4(p.u + ((long long)n * p.HW + pxs[j]) * F + c0, pack(u));
        }
    }
}

// ---- output stage forward --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void grul_out_fwd_sums(GruLP p) {
    __shared__ float sh[NT * 8];
    GL_GEOM();
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * F + c0;
        float k[4];
        unpack(ld4(gp), k);
        for (int px = p0 + prow; px < p1; px += rows) {
            float a[4];
            unpack(ld4(gp + (long long)px * F), a);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = a[e] - k[e]; v[e] += d; v[4 + e] += d * d; }
        }
    }
    gl_store_partials<2>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void grul_out_fwd_apply(GruLP p) {
    __shared__ double tot[2 * GL_SLAB];
    GL_GEOM();
    gl_fold<2>(p, tot, FS, n, slab0);
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * F + c0;
    float k[4], mu[4], rs[4], ga[4], be[4];
    unpack(ld4(gp), k); unpack(ld4(p.gamma + c0), ga); unpack(ld4(p.beta + c0), be);
#pragma unroll
    for (int e = 0; e < 4; ++e) gl_moments(tot[c4 * 4 + e], tot[FS + c4 * 4 + e], k[e], p.HW, p.eps, mu[e], rs[e]);
    if (blockIdx.x == 0 && prow == 0) {
        st4(p.mean + (long long)n * F + c0, pack(mu));
        st4(p.rstd + (long long)n * F + c0, pack(rs));
    }
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        GL_TRIP();
        float a[2][4], hv[2][4], uv[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unpack(ld4(gp + (long long)pxs[j] * F), a[j]);
            unpack(ld4(p.h + (long long)n * p.h_sn + (long long)pxs[j] * p.h_sp + c0), hv[j]);
            unpack(ld4(p.u + ((long long)n * p.HW + pxs[j]) * F + c0), uv[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float cnd = tanh_((a[j][e] - mu[e]) * rs[e] * ga[e] + be[e]);
                o[e] = uv[j][e] * hv[j][e] + (1.f - uv[j][e]) * cnd;
            }
            const float4 o4 = pack(o);
            for (int q = 0; q < p.nout; ++q) st4(p.out[q] + (long long)n * p.o_sn[q] + (long long)pxs[j] * p.o_sp[q] + c0, o4);
        }
    }
}

// ---- output stage backward -------------------------------------------------------------------------------------------------------
// dz and xhat of one pixel's 4 channels (dz = dL/d(normalised candidate pre-activation)); dv = dh', uv = u, cnd = the candidate
struct OutBwdPx { float x[4], dz[4], dv[4], uv[4], cnd[4]; };
__device__ __forceinline__ void grul_out_bwd_px(const GruLP& p, int n, int px, int c0, const float* gp, const float (&mu)[4], const float (&rs)[4],
                                                const float (&ga)[4], const float (&be)[4], OutBwdPx& o) {
    // the two passes must round dz identically (pass 2 subtracts pass 1's sum of it; at HW = 1 the difference is exactly 0 times rstd =
    // 1000): no multiply of this function may be fused into an addition of its caller
#pragma clang fp contract(off)
    float a[4];
    unpack(ld4(gp + (long long)px * p.F), a);
    unpack(ld4(p.u + ((long long)n * p.HW + px) * p.F + c0), o.uv);
    float4 d4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < p.ndy; ++q) {
        const float4 t = ld4(p.dy[q] + (long long)n * p.dy_sn[q] + (long long)px * p.dy_sp[q] + c0);
        d4.x += t.x; d4.y += t.y; d4.z += t.z; d4.w += t.w;
    }
    unpack(d4, o.dv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o.x[e] = (a[e] - mu[e]) * rs[e];
        o.cnd[e] = tanh_(o.x[e] * ga[e] + be[e]);
        o.dz[e] = o.dv[e] * (1.f - o.uv[e]) * (1.f - o.cnd[e] * o.cnd[e]);
    }
}

// pass 1: k = 0 sum dz, 1 sum dz*xhat; writes du and dh = u*dh' (overwrites) on the way
__global__ __launch_bounds__(NT) void grul_out_bwd_sums(GruLP p) {
    __shared__ float sh[NT * 8];
    GL_GEOM();
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * F + c0;
        float mu[4], rs[4], ga[4], be[4];
        unpack(ld4(p.mean + (long long)n * F + c0), mu); unpack(ld4(p.rstd + (long long)n * F + c0), rs);
        unpack(ld4(p.gamma + c0), ga); unpack(ld4(p.beta + c0), be);
        for (int px = p0 + prow; px < p1; px += rows) {
            OutBwdPx o;
            grul_out_bwd_px(p, n, px, c0, gp, mu, rs, ga, be, o);
            float hv[4], duv[4], dhv[4];
            unpack(ld4(p.h + (long long)n * p.h_sn + (long long)px * p.h_sp + c0), hv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                duv[e] = o.dv[e] * (hv[e] - o.cnd[e]);
                dhv[e] = o.dv[e] * o.uv[e];
                v[e] += o.dz[e]; v[4 + e] += o.dz[e] * o.x[e];
            }
            st4(p.du + ((long long)n * p.HW + px) * F + c0, pack(duv));
            st4(p.dh + (long long)n * p.dh_sn + (long long)px * p.dh_sp + c0, pack(dhv));
        }
    }
    gl_store_partials<2>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void grul_out_bwd_apply(GruLP p) {
    __shared__ double tot[2 * GL_SLAB];
    GL_GEOM();
    gl_fold<2>(p, tot, FS, n, slab0);
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * F + c0;
    float mu[4], rs[4], ga[4], be[4], sb[4], sg[4];
    unpack(ld4(p.mean + (long long)n * F + c0), mu); unpack(ld4(p.rstd + (long long)n * F + c0), rs);
    unpack(ld4(p.gamma + c0), ga); unpack(ld4(p.beta + c0), be);
#pragma unroll
    for (int e = 0; e < 4; ++e) { sb[e] = (float)tot[c4 * 4 + e]; sg[e] = (float)tot[FS + c4 * 4 + e]; }
    if (blockIdx.x == 0 && prow == 0) {
        // fp32-rounded per-sample totals: their float64 sum over the samples does not depend on the arrival order
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsafeAtomicAdd(p.dbeta + c0 + e, (double)sb[e]);
            unsafeAtomicAdd(p.dgamma + c0 + e, (double)sg[e]);
        }
    }
    const float inv = 1.f / (float)p.HW;
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        GL_TRIP();
        OutBwdPx o[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) grul_out_bwd_px(p, n, pxs[j], c0, gp, mu, rs, ga, be, o[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = ga[e] * rs[e] * (o[j].dz[e] - sb[e] * inv - o[j].x[e] * sg[e] * inv);
            st4(p.dpre + ((long long)n * p.HW + pxs[j]) * F + c0, pack(d));
        }
    }
}

// ---- gates stage backward --------------------------------------------------------------------------------------------------------
// xhat, dz of one pixel's 4 r-channels ([0..3]) and 4 u-channels ([4..7]); rr = the reset gate, drhv = the gradient of the r*h slot
struct GatesBwdPx { float x[8], dz[8], rr[4], drhv[4]; };
__device__ __forceinline__ void grul_gates_bwd_px(const GruLP& p, int n, int px, int c0, const float* gp, const float (&mu)[8],
                                                  const float (&rs)[8], const float (&ga)[8], const float (&be)[8], GatesBwdPx& o) {
#pragma clang fp contract(off)             // see grul_out_bwd_px
    float a[4], b[4], hv[4], duv[4];
    unpack(ld4(gp + (long long)px * 2 * p.F), a); unpack(ld4(gp + (long long)px * 2 * p.F + p.F), b);
    unpack(ld4(p.h + (long long)n * p.h_sn + (long long)px * p.h_sp + c0), hv);
    unpack(ld4(p.drh + (long long)n * p.drh_sn + (long long)px * p.drh_sp + c0), o.drhv);
    unpack(ld4(p.du + ((long long)n * p.HW + px) * p.F + c0), duv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o.x[e] = (a[e] - mu[e]) * rs[e];
        o.x[4 + e] = (b[e] - mu[4 + e]) * rs[4 + e];
        o.rr[e] = sigm(o.x[e] * ga[e] + be[e]);
        const float uu = sigm(o.x[4 + e] * ga[4 + e] + be[4 + e]);
        o.dz[e] = o.drhv[e] * hv[e] * o.rr[e] * (1.f - o.rr[e]);
        o.dz[4 + e] = duv[e] * uu * (1.f - uu);
    }
}

#define GL_GATES_BWD_PARAMS()                                                                                         \
    float mu[8], rs[8], ga[8], be[8];                                                                                 \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                   \
        const long long o_ = (long long)n * 2 * F + c0 + e;                                                           \
        mu[e] = p.mean[o_]; mu[4 + e] = p.mean[o_ + F]; rs[e] = p.rstd[o_]; rs[4 + e] = p.rstd[o_ + F];               \
        ga[e] = p.gamma[c0 + e]; ga[4 + e] = p.gamma[F + c0 + e]; be[e] = p.beta[c0 + e]; be[4 + e] = p.beta[F + c0 + e]; \
    }

// pass 1: k = 0 sum dz_r, 1 sum dz_r*xhat_r, 2 sum dz_u, 3 sum dz_u*xhat_u; reads only
__global__ __launch_bounds__(NT) void grul_gates_bwd_sums(GruLP p) {
    __shared__ float sh[NT * 16];
    GL_GEOM();
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
        GL_GATES_BWD_PARAMS();
        for (int px = p0 + prow; px < p1; px += rows) {
            GatesBwdPx o;
            grul_gates_bwd_px(p, n, px, c0, gp, mu, rs, ga, be, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] += o.dz[e]; v[4 + e] += o.dz[e] * o.x[e];
                v[8 + e] += o.dz[4 + e]; v[12 + e] += o.dz[4 + e] * o.x[4 + e];
            }
        }
    }
    gl_store_partials<4>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void grul_gates_bwd_apply(GruLP p) {
    __shared__ double tot[4 * GL_SLAB];
    GL_GEOM();
    gl_fold<4>(p, tot, FS, n, slab0);
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
    GL_GATES_BWD_PARAMS();
    float sb[8], sg[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = c4 * 4 + e;
        sb[e] = (float)tot[c]; sg[e] = (float)tot[FS + c]; sb[4 + e] = (float)tot[2 * FS + c]; sg[4 + e] = (float)tot[3 * FS + c];
    }
    if (blockIdx.x == 0 && prow == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsafeAtomicAdd(p.dbeta + c0 + e, (double)sb[e]); unsafeAtomicAdd(p.dbeta + F + c0 + e, (double)sb[4 + e]);
            unsafeAtomicAdd(p.dgamma + c0 + e, (double)sg[e]); unsafeAtomicAdd(p.dgamma + F + c0 + e, (double)sg[4 + e]);
        }
    }
    const float inv = 1.f / (float)p.HW;
    float* dp = p.dpre + (long long)n * p.HW * 2 * F + c0;
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        GL_TRIP();
        GatesBwdPx o[2];
        float acc[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            grul_gates_bwd_px(p, n, pxs[j], c0, gp, mu, rs, ga, be, o[j]);
            unpack(ld4(p.dh + (long long)n * p.dh_sn + (long long)pxs[j] * p.dh_sp + c0), acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float d[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] += o[j].drhv[e] * o[j].rr[e];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = ga[i] * rs[i] * (o[j].dz[i] - sb[i] * inv - o[j].x[i] * sg[i] * inv);
            st4(p.dh + (long long)n * p.dh_sn + (long long)pxs[j] * p.dh_sp + c0, pack(acc[j]));
            st4(dp + (long long)pxs[j] * 2 * F, make_float4(d[0], d[1], d[2], d[3]));
            st4(dp + (long long)pxs[j] * 2 * F + F, make_float4(d[4], d[5], d[6], d[7]));
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool al16(const void* q) { return (((uintptr_t)q) & 15) == 0; }
bool vec_ok(const void* q) { return q && al16(q); }
bool view_ok(const void* q, long long sn, long long sp) { return q && al16(q) && sn % 4 == 0 && sp % 4 == 0; }

int fill(GruLP& p, const SavpGruLargeArgs* L) {
    if (!L) return SAVP_EINVAL;
    const SavpGruArgs* a = &L->g;
    if (a->F < 4 || a->F % 4 || a->N < 1 || a->N > 65535 || a->HW < 1) return SAVP_EINVAL;
    if (a->nout < 0 || a->nout > 4 || a->ndy < 0 || a->ndy > 4) return SAVP_EINVAL;
    if (!vec_ok(a->pre) || !view_ok(a->h.p, a->h.sn, a->h.sp)) return SAVP_EINVAL;
    if (!vec_ok(a->gamma) || !vec_ok(a->beta) || !vec_ok(a->mean) || !vec_ok(a->rstd)) return SAVP_EINVAL;
    if (!L->ws || (((uintptr_t)L->ws) & 7) || L->ws_bytes < savp_convgru_large_ws_bytes(a->N, a->HW, a->F)) return SAVP_EINVAL;
    p.N = a->N; p.HW = a->HW; p.F = a->F; p.eps = a->eps;
    p.chunk = savp_convgru_large_chunk(a->N, a->HW);
    p.nchunks = (a->HW + p.chunk - 1) / p.chunk;
    p.pre = a->pre;
    p.h = (const float*)a->h.p; p.h_sn = a->h.sn; p.h_sp = a->h.sp;
    p.gamma = a->gamma; p.beta = a->beta; p.mean = a->mean; p.rstd = a->rstd;
    p.u = a->u;
    p.rh = (float*)a->rh.p; p.rh_sn = a->rh.sn; p.rh_sp = a->rh.sp;
    p.nout = a->nout;
    for (int i = 0; i < a->nout; ++i) {
        if (!view_ok(a->out[i].p, a->out[i].sn, a->out[i].sp)) return SAVP_EINVAL;
        p.out[i] = (float*)a->out[i].p; p.o_sn[i] = a->out[i].sn; p.o_sp[i] = a->out[i].sp;
    }
    p.ndy = a->ndy;
    for (int i = 0; i < a->ndy; ++i) {
        if (!view_ok(a->dy[i].p, a->dy[i].sn, a->dy[i].sp)) return SAVP_EINVAL;
        p.dy[i] = (const float*)a->dy[i].p; p.dy_sn[i] = a->dy[i].sn; p.dy_sp[i] = a->dy[i].sp;
    }
    p.dpre = a->dpre; p.du = a->du;
    p.dh = (float*)a->dh.p; p.dh_sn = a->dh.sn; p.dh_sp = a->dh.sp;
    p.drh = (const float*)a->drh.p; p.drh_sn = a->drh.sn; p.drh_sp = a->drh.sp;
    p.dgamma = a->dgamma; p.dbeta = a->dbeta;
    p.ws = (double*)L->ws;
    return SAVP_OK;
}

}  // namespace

// pixels per workgroup: about 512 workgroups per launch, between 32 and 256 pixels, and at most GL_MAX_CHUNKS chunks per plane
extern "C" int32_t savp_convgru_large_chunk(int32_t N, int32_t HW) {
    if (N < 1 || HW < 1) return 0;
    long long c = ((long long)N * HW + 511) / 512;
    if (c < 32) c = 32;
    if (c > 256) c = 256;
    if ((HW + c - 1) / c > GL_MAX_CHUNKS) c = ((long long)HW + GL_MAX_CHUNKS - 1) / GL_MAX_CHUNKS;
    return (int32_t)c;
}

extern "C" int64_t savp_convgru_large_ws_bytes(int32_t N, int32_t HW, int32_t F) {
    const int chunk = savp_convgru_large_chunk(N, HW);
    if (!chunk || F < 1) return 0;
    return (int64_t)N * ((HW + chunk - 1) / chunk) * GL_K * F * (int64_t)sizeof(double);
}

#define GRUL_ENTRY(name, sums, apply, cond)                                                                        \
    extern "C" int name(void* stream, const SavpGruLargeArgs* a) {                                                 \
        GruLP p;                                                                                                    \
        int rc = fill(p, a);                                                                                        \
        if (rc) return rc;                                                                                          \
        if (!(cond)) return SAVP_EINVAL;                                                                            \
        const dim3 grid(p.nchunks, p.N, (p.F + GL_SLAB - 1) / GL_SLAB);                                             \
        hipLaunchKernelGGL(sums, grid, dim3(NT), 0, (hipStream_t)stream, p);                                        \
        hipLaunchKernelGGL(apply, grid, dim3(NT), 0, (hipStream_t)stream, p);                                       \
        return LAUNCH_OK();                                                                                         \
    }
GRUL_ENTRY(savp_convgru_large_gates_fwd, grul_gates_fwd_sums, grul_gates_fwd_apply, vec_ok(p.u) && view_ok(p.rh, p.rh_sn, p.rh_sp))
GRUL_ENTRY(savp_convgru_large_out_fwd, grul_out_fwd_sums, grul_out_fwd_apply, vec_ok(p.u) && p.nout >= 1)
GRUL_ENTRY(savp_convgru_large_out_bwd, grul_out_bwd_sums, grul_out_bwd_apply,
           vec_ok(p.u) && vec_ok(p.du) && vec_ok(p.dpre) && view_ok(p.dh, p.dh_sn, p.dh_sp) && p.ndy >= 1 && p.dgamma && p.dbeta)
GRUL_ENTRY(savp_convgru_large_gates_bwd, grul_gates_bwd_sums, grul_gates_bwd_apply,
           vec_ok(p.du) && vec_ok(p.dpre) && view_ok(p.dh, p.dh_sn, p.dh_sp) && view_ok(p.drh, p.drh_sn, p.drh_sp) && p.dgamma &&
               p.dbeta)

// ln_gru.hip -- the gate blocks of Conv2DGRUCell with LAYER norms inside the cell (rnn_ops.py:234-267 with separate_norms = True, which
// conv_rnn_norm_layer = 'layer' switches on): savp_convgru_ln_*.  r = sigmoid(LN(pre_r)), u = sigmoid(LN(pre_u)), c = tanh(LN(cand)),
// LN = tf.contrib.layers.layer_norm: statistics per sample over (H, W, F) of THAT tensor, biased variance, gamma / beta of shape [F].
// So the 2F gate channels are G = 2 groups (reset | update) and the candidate is G = 1; mean and rstd are [N][G].
// The structure is that of gru_large.hip, for a plane of any size: every block is two launches over chunks of pixels,
//   pass 1 (sums)  : a workgroup covers `chunk` pixels x a slab of <= 256 of the F channels of one sample; a thread owns 4 channels and walks
//                    the chunk's pixel rows (whole channel-last rows per wave, 16-byte accesses).  Per-channel sums, folded over the pixel
//                    rows in float64, are STORED to the caller's workspace ws[n][chunk][4][F] (float64): no atomics, nothing to clear.
//   pass 2 (apply) : the same grid; every workgroup folds the partials of ALL F channels of its sample in chunk order (float64, into LDS),
//                    then one wave per group folds the channels of the group (lane-strided, then a butterfly: a fixed order), and the
//                    workgroup writes its pixels.
// Forward: the per-channel sums are taken around the channel's value at the sample's first pixel; a channel's mean and M2 come from them in
// float64, and the group's from its channels' by the parallel-variance identity (M2_g = sum M2_c + HW * sum (mean_c - mean_g)^2), as
// group_norm.hip combines its partials.  Backward: per channel sum dz and sum dz*xhat (dz = the gradient at the activation's input); they
// are dbeta and dgamma, and their gamma-weighted sums over the group give dx = rstd * (gamma*dz - mean_g(gamma*dz) - xhat * mean_g(gamma*dz*xhat)).
// Activations are recomputed in both passes; no normalised tensor is stored.  Every result is a function of the operands alone, except
// that several samples add to dgamma / dbeta with float64 atomics of fp32-rounded per-sample totals, like every other norm of the step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define NT 256
#define LG_SLAB 256                   // channels of F per workgroup
#define LG_K 4                        // float64 partials per channel of F in the workspace
#define LG_MAX_F 1024                 // the apply pass holds LG_K * F float64 totals in LDS (32 KB at the most)
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

struct LnGruP {
    int N, HW, F, chunk, nchunks;
    float eps;
    const float* pre;                                    // gates stage: [N,HW,2F]; output stage: [N,HW,F]
    const float* h; long long h_sn, h_sp;
    const float *gamma, *beta;                           // [2F] (reset | update) / [F]
    float *mean, *rstd;                                  // [N,2] / [N,1]
    float* u;                                            // [N,HW,F]
    float* rh; long long rh_sn, rh_sp;
    int nout; float* out[4]; long long o_sn[4], o_sp[4];
    int ndy; const float* dy[4]; long long dy_sn[4], dy_sp[4];
    float* dpre;
    float* du;
    float* dh; long long dh_sn, dh_sp;
    const float* drh; long long drh_sn, drh_sp;
    double *dgamma, *dbeta;
    double* ws;                                          // [N][nchunks][LG_K][F]
};

// thread geometry of every kernel: c4 = this thread's 4-channel group inside the slab, prow = its pixel row, `on` = it has work
#define LG_GEOM()                                                                                                     \
    const int F = p.F, FS = F < LG_SLAB ? F : LG_SLAB, F4s = FS >> 2;                                                 \
    const int c4 = threadIdx.x % F4s, prow = threadIdx.x / F4s, rows = NT / F4s;                                      \
    const int n = blockIdx.y, slab0 = blockIdx.z * LG_SLAB, c0 = slab0 + c4 * 4;                                      \
    const bool on = prow < rows && c0 < F;                                                                            \
    const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk)

// The apply passes walk their pixel rows two at a time and issue every load of a trip before its first store (see gru_large.hip).  A
// trip's second row repeats the first when it lies past the chunk (`two` false): loaded again, never stored.
#define LG_TRIP()                                                                                                     \
    const bool two = px0 + rows < p1;                                                                                 \
    const int pxs[2] = {px0, two ? px0 + rows : px0}

// pass 1 epilogue: v[k*4+e] = this thread's sum k of channel c0+e -> ws[n][chunk][k][c], folded over the pixel rows in float64, row order
template <int K>
__device__ __forceinline__ void lg_store_partials(const LnGruP& p, const float (&v)[K * 4], float* sh, int FS, int c4, int prow, int rows,
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
        if (cc < p.F) p.ws[(((long long)n * p.nchunks + blockIdx.x) * LG_K + k) * p.F + cc] = t;
    }
}

// pass 2 prologue: tot[k*F + c] = the sample's sum k of channel c over all chunks, chunk order, for ALL F channels (the group's
// statistics need every slab's)
template <int K>
__device__ __forceinline__ void lg_fold(const LnGruP& p, double* tot, int n) {
    const long long step = (long long)LG_K * p.F;
    for (int i = threadIdx.x; i < K * p.F; i += NT) {
        const double* w = p.ws + (long long)n * p.nchunks * step + i;          // [k][c] of a chunk is contiguous: k*F + c = i
        double t = 0.0;
#pragma unroll 4
        for (int ch = 0; ch < p.nchunks; ++ch) t += w[ch * step];
        tot[i] = t;
    }
    __syncthreads();
}

// sum over the 64 lanes of a wave, the same bits in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave: mean and rstd of a group of F channels from the channels' shifted sums s[c] = sum (x - shift[c]), q[c] = sum (x - shift[c])^2
// over the HW pixels.  gs[0] = mean, gs[1] = rstd (LDS); `stat` true: also stored to *mean / *rstd.
__device__ __forceinline__ void lg_group_moments(const double* s, const double* q, const float* shift, int F, int HW, float eps, float* gs,
                                                 bool stat, float* mean, float* rstd) {
    const int lane = threadIdx.x & 63;
    const double inv = 1.0 / (double)HW;
    double a = 0.0;
    for (int c = lane; c < F; c += 64) a += (double)shift[c] + s[c] * inv;
    const double mg = wave_sum(a) / (double)F;
    double m2 = 0.0;
    for (int c = lane; c < F; c += 64) {
        const double mc = (double)shift[c] + s[c] * inv, d = mc - mg;
        double m2c = q[c] - s[c] * s[c] * inv;
        if (m2c < 0.0) m2c = 0.0;
        m2 += m2c + (double)HW * d * d;
    }
    const double var = wave_sum(m2) / ((double)HW * (double)F);
    if (lane == 0) {
        const float mu = (float)mg, rs = (float)(1.0 / sqrt(var + (double)eps));
        gs[0] = mu; gs[1] = rs;
        if (stat) { *mean = mu; *rstd = rs; }
    }
}

// One wave: gs[0] = mean_g(gamma*dz), gs[1] = mean_g(gamma*dz*xhat) of a group from the channels' sums sb[c] = sum dz, sg[c] = sum dz*xhat
__device__ __forceinline__ void lg_group_bwd(const double* sb, const double* sg, const float* gamma, int F, int HW, float* gs) {
    const int lane = threadIdx.x & 63;
    double a = 0.0, b = 0.0;
    for (int c = lane; c < F; c += 64) { a += (double)gamma[c] * sb[c]; b += (double)gamma[c] * sg[c]; }
    a = wave_sum(a); b = wave_sum(b);
    if (lane == 0) {
        const double inv = 1.0 / ((double)HW * (double)F);
        gs[0] = (float)(a * inv); gs[1] = (float)(b * inv);
    }
}

// ---- gates stage forward ---------------------------------------------------------------------------------------------------------
// sums of pre - pre[pixel 0]: k = 0 sum r, 1 sum of squares r, 2 sum u, 3 sum of squares u
__global__ __launch_bounds__(NT) void lng_gates_fwd_sums(LnGruP p) {
    __shared__ float sh[NT * 16];
    LG_GEOM();
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
    lg_store_partials<4>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void lng_gates_fwd_apply(LnGruP p) {
    extern __shared__ double tot[];                      // [4][F]
    __shared__ float gs[4];                              // mean, rstd of r; mean, rstd of u
    LG_GEOM();
    lg_fold<4>(p, tot, n);
    const int g = threadIdx.x >> 6;
    if (g < 2)
        lg_group_moments(tot + 2 * g * F, tot + (2 * g + 1) * F, p.pre + (long long)n * p.HW * 2 * F + g * F, F, p.HW, p.eps, gs + 2 * g,
                         blockIdx.x == 0 && blockIdx.z == 0, p.mean + (long long)n * 2 + g, p.rstd + (long long)n * 2 + g);
    __syncthreads();
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
    const float mur = gs[0], rsr = gs[1], muu = gs[2], rsu = gs[3];
    float gr[4], gu[4], br[4], bu[4];
    unpack(ld4(p.gamma + c0), gr); unpack(ld4(p.gamma + F + c0), gu);
    unpack(ld4(p.beta + c0), br); unpack(ld4(p.beta + F + c0), bu);
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        LG_TRIP();
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
                r[e] = sigm((a[j][e] - mur) * rsr * gr[e] + br[e]) * hv[j][e];
                u[e] = sigm((b[j][e] - muu) * rsu * gu[e] + bu[e]);
            }
            st4(p.rh + (long long)n * p.rh_sn + (long long)pxs[j] * p.rh_sp + c0, pack(r));
            st4(p.u + ((long long)n * p.HW + pxs[j]) * F + c0, pack(u));
        }
    }
}

// ---- output stage forward --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void lng_out_fwd_sums(LnGruP p) {
    __shared__ float sh[NT * 8];
    LG_GEOM();
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
    lg_store_partials<2>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void lng_out_fwd_apply(LnGruP p) {
    extern __shared__ double tot[];                      // [2][F]
    __shared__ float gs[2];
    LG_GEOM();
    lg_fold<2>(p, tot, n);
    if (threadIdx.x < 64)
        lg_group_moments(tot, tot + F, p.pre + (long long)n * p.HW * F, F, p.HW, p.eps, gs, blockIdx.x == 0 && blockIdx.z == 0, p.mean + n,
                         p.rstd + n);
    __syncthreads();
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * F + c0;
    const float mu = gs[0], rs = gs[1];
    float ga[4], be[4];
    unpack(ld4(p.gamma + c0), ga); unpack(ld4(p.beta + c0), be);
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        LG_TRIP();
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
                const float cnd = tanh_((a[j][e] - mu) * rs * ga[e] + be[e]);
                o[e] = uv[j][e] * hv[j][e] + (1.f - uv[j][e]) * cnd;
            }
            const float4 o4 = pack(o);
            for (int q = 0; q < p.nout; ++q) st4(p.out[q] + (long long)n * p.o_sn[q] + (long long)pxs[j] * p.o_sp[q] + c0, o4);
        }
    }
}

// ---- output stage backward -------------------------------------------------------------------------------------------------------
// dz and xhat of one pixel's 4 channels (dz = dL/d(gamma * xhat + beta) of the candidate); dv = dh', uv = u, cnd = the candidate
struct OutBwdPx { float x[4], dz[4], dv[4], uv[4], cnd[4]; };
__device__ __forceinline__ void lng_out_bwd_px(const LnGruP& p, int n, int px, int c0, const float* gp, float mu, float rs, const float (&ga)[4],
                                               const float (&be)[4], OutBwdPx& o) {
    // the two passes must round dz and xhat identically (pass 2 subtracts means of pass 1's sums): no multiply of this function may be
    // fused into an addition of its caller
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
        o.x[e] = (a[e] - mu) * rs;
        o.cnd[e] = tanh_(o.x[e] * ga[e] + be[e]);
        o.dz[e] = o.dv[e] * (1.f - o.uv[e]) * (1.f - o.cnd[e] * o.cnd[e]);
    }
}

// pass 1: k = 0 sum dz, 1 sum dz*xhat; writes du and dh = u*dh' (overwrites) on the way
__global__ __launch_bounds__(NT) void lng_out_bwd_sums(LnGruP p) {
    __shared__ float sh[NT * 8];
    LG_GEOM();
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * F + c0;
        const float mu = p.mean[n], rs = p.rstd[n];
        float ga[4], be[4];
        unpack(ld4(p.gamma + c0), ga); unpack(ld4(p.beta + c0), be);
        for (int px = p0 + prow; px < p1; px += rows) {
            OutBwdPx o;
            lng_out_bwd_px(p, n, px, c0, gp, mu, rs, ga, be, o);
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
    lg_store_partials<2>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void lng_out_bwd_apply(LnGruP p) {
    extern __shared__ double tot[];                      // [2][F]
    __shared__ float gs[2];
    LG_GEOM();
    lg_fold<2>(p, tot, n);
    if (threadIdx.x < 64) lg_group_bwd(tot, tot + F, p.gamma, F, p.HW, gs);
    __syncthreads();
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * F + c0;
    const float mu = p.mean[n], rs = p.rstd[n], ma = gs[0], mb = gs[1];
    float ga[4], be[4];
    unpack(ld4(p.gamma + c0), ga); unpack(ld4(p.beta + c0), be);
    if (blockIdx.x == 0 && prow == 0) {
        // fp32-rounded per-sample totals: their float64 sum over the samples does not depend on the arrival order
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsafeAtomicAdd(p.dbeta + c0 + e, (double)(float)tot[c0 + e]);
            unsafeAtomicAdd(p.dgamma + c0 + e, (double)(float)tot[F + c0 + e]);
        }
    }
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        LG_TRIP();
        OutBwdPx o[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) lng_out_bwd_px(p, n, pxs[j], c0, gp, mu, rs, ga, be, o[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = rs * (ga[e] * o[j].dz[e] - ma - o[j].x[e] * mb);
            st4(p.dpre + ((long long)n * p.HW + pxs[j]) * F + c0, pack(d));
        }
    }
}

// ---- gates stage backward --------------------------------------------------------------------------------------------------------
// xhat, dz of one pixel's 4 r-channels ([0..3]) and 4 u-channels ([4..7]); rr = the reset gate, drhv = the gradient of the r*h slot
struct GatesBwdPx { float x[8], dz[8], rr[4], drhv[4]; };
__device__ __forceinline__ void lng_gates_bwd_px(const LnGruP& p, int n, int px, int c0, const float* gp, const float (&st)[4],
                                                 const float (&ga)[8], const float (&be)[8], GatesBwdPx& o) {
#pragma clang fp contract(off)             // see lng_out_bwd_px
    float a[4], b[4], hv[4], duv[4];
    unpack(ld4(gp + (long long)px * 2 * p.F), a); unpack(ld4(gp + (long long)px * 2 * p.F + p.F), b);
    unpack(ld4(p.h + (long long)n * p.h_sn + (long long)px * p.h_sp + c0), hv);
    unpack(ld4(p.drh + (long long)n * p.drh_sn + (long long)px * p.drh_sp + c0), o.drhv);
    unpack(ld4(p.du + ((long long)n * p.HW + px) * p.F + c0), duv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        o.x[e] = (a[e] - st[0]) * st[1];
        o.x[4 + e] = (b[e] - st[2]) * st[3];
        o.rr[e] = sigm(o.x[e] * ga[e] + be[e]);
        const float uu = sigm(o.x[4 + e] * ga[4 + e] + be[4 + e]);
        o.dz[e] = o.drhv[e] * hv[e] * o.rr[e] * (1.f - o.rr[e]);
        o.dz[4 + e] = duv[e] * uu * (1.f - uu);
    }
}

// st = (mean r, rstd r, mean u, rstd u) of sample n; ga / be = this thread's 4 + 4 channels of gamma / beta
#define LG_GATES_BWD_PARAMS()                                                                                         \
    const float st[4] = {p.mean[2 * n], p.rstd[2 * n], p.mean[2 * n + 1], p.rstd[2 * n + 1]};                         \
    float ga[8], be[8];                                                                                               \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                                   \
        ga[e] = p.gamma[c0 + e]; ga[4 + e] = p.gamma[F + c0 + e]; be[e] = p.beta[c0 + e]; be[4 + e] = p.beta[F + c0 + e]; \
    }

// pass 1: k = 0 sum dz_r, 1 sum dz_r*xhat_r, 2 sum dz_u, 3 sum dz_u*xhat_u; reads only
__global__ __launch_bounds__(NT) void lng_gates_bwd_sums(LnGruP p) {
    __shared__ float sh[NT * 16];
    LG_GEOM();
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
        LG_GATES_BWD_PARAMS();
        for (int px = p0 + prow; px < p1; px += rows) {
            GatesBwdPx o;
            lng_gates_bwd_px(p, n, px, c0, gp, st, ga, be, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] += o.dz[e]; v[4 + e] += o.dz[e] * o.x[e];
                v[8 + e] += o.dz[4 + e]; v[12 + e] += o.dz[4 + e] * o.x[4 + e];
            }
        }
    }
    lg_store_partials<4>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

__global__ __launch_bounds__(NT) void lng_gates_bwd_apply(LnGruP p) {
    extern __shared__ double tot[];                      // [4][F]
    __shared__ float gs[4];                              // mean(gamma dz), mean(gamma dz xhat) of r; of u
    LG_GEOM();
    lg_fold<4>(p, tot, n);
    const int g = threadIdx.x >> 6;
    if (g < 2) lg_group_bwd(tot + 2 * g * F, tot + (2 * g + 1) * F, p.gamma + g * F, F, p.HW, gs + 2 * g);
    __syncthreads();
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
    LG_GATES_BWD_PARAMS();
    const float ma[2] = {gs[0], gs[2]}, mb[2] = {gs[1], gs[3]};
    if (blockIdx.x == 0 && prow == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            unsafeAtomicAdd(p.dbeta + c0 + e, (double)(float)tot[c0 + e]);
            unsafeAtomicAdd(p.dgamma + c0 + e, (double)(float)tot[F + c0 + e]);
            unsafeAtomicAdd(p.dbeta + F + c0 + e, (double)(float)tot[2 * F + c0 + e]);
            unsafeAtomicAdd(p.dgamma + F + c0 + e, (double)(float)tot[3 * F + c0 + e]);
        }
    }
    float* dp = p.dpre + (long long)n * p.HW * 2 * F + c0;
    for (int px0 = p0 + prow; px0 < p1; px0 += 2 * rows) {
        LG_TRIP();
        GatesBwdPx o[2];
        float acc[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            lng_gates_bwd_px(p, n, pxs[j], c0, gp, st, ga, be, o[j]);
            unpack(ld4(p.dh + (long long)n * p.dh_sn + (long long)pxs[j] * p.dh_sp + c0), acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float d[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] += o[j].drhv[e] * o[j].rr[e];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = st[2 * (i >> 2) + 1] * (ga[i] * o[j].dz[i] - ma[i >> 2] - o[j].x[i] * mb[i >> 2]);
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
bool f32_ok(const void* q) { return q && (((uintptr_t)q) & 3) == 0; }          // mean / rstd: [N][G], read and written one float at a time

int fill(LnGruP& p, const SavpGruLargeArgs* L) {
    if (!L) return SAVP_EINVAL;
    const SavpGruArgs* a = &L->g;
    if (a->F < 4 || a->F % 4 || a->F > LG_MAX_F || a->N < 1 || a->N > 65535 || a->HW < 1) return SAVP_EINVAL;
    if (a->nout < 0 || a->nout > 4 || a->ndy < 0 || a->ndy > 4) return SAVP_EINVAL;
    if (!vec_ok(a->pre) || !view_ok(a->h.p, a->h.sn, a->h.sp)) return SAVP_EINVAL;
    if (!vec_ok(a->gamma) || !vec_ok(a->beta) || !f32_ok(a->mean) || !f32_ok(a->rstd)) return SAVP_EINVAL;
    if (!L->ws || (((uintptr_t)L->ws) & 7) || L->ws_bytes < savp_convgru_ln_ws_bytes(a->N, a->HW, a->F)) return SAVP_EINVAL;
    p.N = a->N; p.HW = a->HW; p.F = a->F; p.eps = a->eps;
    p.chunk = savp_convgru_ln_chunk(a->N, a->HW);
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

// pixels per workgroup: about 512 workgroups per launch, between 32 and 256 pixels, and at most 64 chunks per plane (the rule of
// gru_large.hip, restated so that this file stands alone)
extern "C" int32_t savp_convgru_ln_chunk(int32_t N, int32_t HW) {
    if (N < 1 || HW < 1) return 0;
    long long c = ((long long)N * HW + 511) / 512;
    if (c < 32) c = 32;
    if (c > 256) c = 256;
    if ((HW + c - 1) / c > 64) c = ((long long)HW + 63) / 64;
    return (int32_t)c;
}

extern "C" int64_t savp_convgru_ln_ws_bytes(int32_t N, int32_t HW, int32_t F) {
    const int chunk = savp_convgru_ln_chunk(N, HW);
    if (!chunk || F < 1) return 0;
    return (int64_t)N * ((HW + chunk - 1) / chunk) * LG_K * F * (int64_t)sizeof(double);
}

// K = the float64 totals per channel the apply pass holds in LDS
#define LNG_ENTRY(name, sums, apply, K, cond)                                                                      \
    extern "C" int name(void* stream, const SavpGruLargeArgs* a) {                                                 \
        LnGruP p;                                                                                                   \
        int rc = fill(p, a);                                                                                        \
        if (rc) return rc;                                                                                          \
        if (!(cond)) return SAVP_EINVAL;                                                                            \
        const dim3 grid(p.nchunks, p.N, (p.F + LG_SLAB - 1) / LG_SLAB);                                             \
        hipLaunchKernelGGL(sums, grid, dim3(NT), 0, (hipStream_t)stream, p);                                        \
        hipLaunchKernelGGL(apply, grid, dim3(NT), (K) * p.F * sizeof(double), (hipStream_t)stream, p);              \
        return LAUNCH_OK();                                                                                         \
    }
LNG_ENTRY(savp_convgru_ln_gates_fwd, lng_gates_fwd_sums, lng_gates_fwd_apply, 4, vec_ok(p.u) && view_ok(p.rh, p.rh_sn, p.rh_sp))
LNG_ENTRY(savp_convgru_ln_out_fwd, lng_out_fwd_sums, lng_out_fwd_apply, 2, vec_ok(p.u) && p.nout >= 1)
LNG_ENTRY(savp_convgru_ln_out_bwd, lng_out_bwd_sums, lng_out_bwd_apply, 2,
          vec_ok(p.u) && vec_ok(p.du) && vec_ok(p.dpre) && view_ok(p.dh, p.dh_sn, p.dh_sp) && p.ndy >= 1 && p.dgamma && p.dbeta)
LNG_ENTRY(savp_convgru_ln_gates_bwd, lng_gates_bwd_sums, lng_gates_bwd_apply, 4,
          vec_ok(p.du) && vec_ok(p.dpre) && view_ok(p.dh, p.dh_sn, p.dh_sp) && view_ok(p.drh, p.drh_sn, p.drh_sp) && p.dgamma &&
              p.dbeta)

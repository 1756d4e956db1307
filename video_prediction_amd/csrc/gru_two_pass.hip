// gru_two_pass.hip -- the gate blocks of Conv2DGRUCell (rnn_ops.py:234-267) for planes of ANY size, with the cell's norms inside:
//   savp_convgru_large_* : the INSTANCE norms of gru.hip (separate_norms = False), mean and rstd per (sample, channel);
//   savp_convgru_ln_*    : LAYER norms (separate_norms = True, which conv_rnn_norm_layer = 'layer' switches on): r = sigmoid(LN(pre_r)),
//                          u = sigmoid(LN(pre_u)), c = tanh(LN(cand)), LN = tf.contrib.layers.layer_norm: statistics per sample over
//                          (H, W, F) of THAT tensor, biased variance, gamma / beta of shape [F].  So the 2F gate channels are G = 2 groups
//                          (reset | update) and the candidate is G = 1; mean and rstd are [N][G].
// gru.hip holds a whole plane in registers (one workgroup = one sample x 4 channels, H*W <= 1024).  Here every block is two launches over
// chunks of pixels, in the manner of inorm_stats_kernel / inorm_apply_kernel (norm_lstm.hip):
//   pass 1 (sums)  : a workgroup covers `chunk` pixels x a slab of <= 256 of the F channels of one sample; a thread owns 4 channels and walks
//                    the chunk's pixel rows, so a wave reads whole channel-last rows with 16-byte accesses.  The workgroup's per-channel
//                    sums are folded over its pixel rows in float64 and STORED to the caller's workspace ws[n][chunk][4][F] (float64): no
//                    atomics, and the workspace needs no clearing.  The two families share these kernels (gru2p_*_sums).
//   pass 2 (apply) : the same grid.  Instance norm: every workgroup folds the chunk partials of its slab in chunk order (float64) and writes
//                    its pixels.  Layer norm: every workgroup folds the partials of ALL F channels of its sample (into dynamic LDS), then
//                    one wave per group folds the channels of the group (lane-strided, then a butterfly: a fixed order).
// Forward: the per-channel sums are taken around the channel's value at the sample's first pixel (a shifted variance, finished in float64);
// the layer norm combines its channels' means and M2 by the parallel-variance identity (M2_g = sum M2_c + HW * sum (mean_c - mean_g)^2), as
// group_norm.hip combines its partials.  Backward: per channel sum dz and sum dz*xhat (dz = the gradient at the activation's input), which
// are also dbeta and dgamma; under the layer norm their gamma-weighted sums over the group give
// dx = rstd * (gamma*dz - mean_g(gamma*dz) - xhat * mean_g(gamma*dz*xhat)).
// Activations are recomputed in both passes; no normalised tensor is stored.  Every result is a function of the operands alone (fixed
// summation order), except that several samples add to dgamma / dbeta with float64 atomics of fp32-rounded per-sample totals, like every
// other norm of the step.  The statistics are always computed here: there is no stats_ready shortcut from the producing convolution.
#include "gru_blocks.h"

#define G2_SLAB 256                   // channels of F per workgroup
#define G2_K 4                        // float64 partials per channel of F in the workspace
#define G2_MAX_CHUNKS 64              // the apply pass folds this many partials per value at the most

namespace {

// thread geometry of every kernel: c4 = this thread's 4-channel group inside the slab, prow = its pixel row, `on` = it has work
#define G2_GEOM()                                                                                                     \
    const int F = p.F, FS = F < G2_SLAB ? F : G2_SLAB, F4s = FS >> 2;                                                 \
    const int c4 = threadIdx.x % F4s, prow = threadIdx.x / F4s, rows = NT / F4s;                                      \
    const int n = blockIdx.y, slab0 = blockIdx.z * G2_SLAB, c0 = slab0 + c4 * 4;                                      \
    const bool on = prow < rows && c0 < F;                                                                            \
    const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk)

// The apply passes walk their pixel rows two at a time and issue every load of a trip before its first store (the destinations may alias
// the sources as far as the compiler knows, so a one-pixel loop exposes a memory round trip per pixel).  A trip's second row repeats the
// first when it lies past the chunk (`two` false): loaded again, never stored.
#define G2_TRIP()                                                                                                     \
    const bool two = px0 + rows < p1;                                                                                 \
    const int pxs[2] = {px0, two ? px0 + rows : px0}

// pass 1 epilogue: v[k*4+e] = this thread's sum k of channel c0+e -> ws[n][chunk][k][c], folded over the pixel rows in float64, row order
template <int K>
__device__ __forceinline__ void store_partials(const GruP& p, const float (&v)[K * 4], float* sh, int FS, int c4, int prow, int rows,
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
        if (cc < p.F) p.ws[(((long long)n * p.nchunks + blockIdx.x) * G2_K + k) * p.F + cc] = t;
    }
}

// ---- forward sums (both families) ------------------------------------------------------------------------------------------------
// gates stage: sums of pre - pre[pixel 0]: k = 0 sum r, 1 sum of squares r, 2 sum u, 3 sum of squares u
__global__ __launch_bounds__(NT) void gru2p_gates_fwd_sums(GruP p) {
    __shared__ float sh[NT * 16];
    G2_GEOM();
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
    store_partials<4>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

// output stage: k = 0 sum, 1 sum of squares of pre - pre[pixel 0]
__global__ __launch_bounds__(NT) void gru2p_out_fwd_sums(GruP p) {
    __shared__ float sh[NT * 8];
    G2_GEOM();
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
    store_partials<2>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

// ---- backward: one pixel, and the sums (both families) ---------------------------------------------------------------------------
// The saved statistics of a thread's channels.  LAYER false: mean / rstd are [N][F] (output stage) or [N][2F] (gates stage), one value
// per channel; true: [N][1] or [N][2], one value per group, repeated here for each of the thread's channels.
template <bool LAYER>
__device__ __forceinline__ void out_stats(const GruP& p, int n, int c0, float (&mu)[4], float (&rs)[4]) {
    if (LAYER) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { mu[e] = p.mean[n]; rs[e] = p.rstd[n]; }
    } else {
        unpack(ld4(p.mean + (long long)n * p.F + c0), mu); unpack(ld4(p.rstd + (long long)n * p.F + c0), rs);
    }
}
// [0..3] = the thread's reset channels, [4..7] = its update channels, of the statistics and of gamma / beta
template <bool LAYER>
__device__ __forceinline__ void gates_params(const GruP& p, int n, int c0, float (&mu)[8], float (&rs)[8], float (&ga)[8], float (&be)[8]) {
    const int F = p.F;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long long o = (long long)n * 2 * F + c0 + e;
        mu[e] = LAYER ? p.mean[2 * n] : p.mean[o]; mu[4 + e] = LAYER ? p.mean[2 * n + 1] : p.mean[o + F];
        rs[e] = LAYER ? p.rstd[2 * n] : p.rstd[o]; rs[4 + e] = LAYER ? p.rstd[2 * n + 1] : p.rstd[o + F];
        ga[e] = p.gamma[c0 + e]; ga[4 + e] = p.gamma[F + c0 + e]; be[e] = p.beta[c0 + e]; be[4 + e] = p.beta[F + c0 + e];
    }
}

// dz and xhat of one pixel's 4 channels (dz = dL/d(gamma * xhat + beta) of the candidate); dv = dh', uv = u, cnd = the candidate
struct OutBwdPx { float x[4], dz[4], dv[4], uv[4], cnd[4]; };
__device__ __forceinline__ void out_bwd_px(const GruP& p, int n, int px, int c0, const float* gp, const float (&mu)[4], const float (&rs)[4],
                                           const float (&ga)[4], const float (&be)[4], OutBwdPx& o) {
    // the two passes must round dz and xhat identically (pass 2 subtracts pass 1's sums of them; under the instance norm at HW = 1 the
    // difference is exactly 0 times rstd = 1000): no multiply of this function may be fused into an addition of its caller
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

// xhat, dz of one pixel's 4 r-channels ([0..3]) and 4 u-channels ([4..7]); rr = the reset gate, drhv = the gradient of the r*h slot
struct GatesBwdPx { float x[8], dz[8], rr[4], drhv[4]; };
__device__ __forceinline__ void gates_bwd_px(const GruP& p, int n, int px, int c0, const float* gp, const float (&mu)[8],
                                             const float (&rs)[8], const float (&ga)[8], const float (&be)[8], GatesBwdPx& o) {
#pragma clang fp contract(off)             // see out_bwd_px
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

// output stage, pass 1: k = 0 sum dz, 1 sum dz*xhat; writes du and dh = u*dh' (overwrites) on the way
template <bool LAYER>
__global__ __launch_bounds__(NT) void gru2p_out_bwd_sums(GruP p) {
    __shared__ float sh[NT * 8];
    G2_GEOM();
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * F + c0;
        float mu[4], rs[4], ga[4], be[4];
        out_stats<LAYER>(p, n, c0, mu, rs);
        unpack(ld4(p.gamma + c0), ga); unpack(ld4(p.beta + c0), be);
        for (int px = p0 + prow; px < p1; px += rows) {
            OutBwdPx o;
            out_bwd_px(p, n, px, c0, gp, mu, rs, ga, be, o);
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
    store_partials<2>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

// gates stage, pass 1: k = 0 sum dz_r, 1 sum dz_r*xhat_r, 2 sum dz_u, 3 sum dz_u*xhat_u; reads only
template <bool LAYER>
__global__ __launch_bounds__(NT) void gru2p_gates_bwd_sums(GruP p) {
    __shared__ float sh[NT * 16];
    G2_GEOM();
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0.f;
    if (on) {
        const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
        float mu[8], rs[8], ga[8], be[8];
        gates_params<LAYER>(p, n, c0, mu, rs, ga, be);
        for (int px = p0 + prow; px < p1; px += rows) {
            GatesBwdPx o;
            gates_bwd_px(p, n, px, c0, gp, mu, rs, ga, be, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] += o.dz[e]; v[4 + e] += o.dz[e] * o.x[e];
                v[8 + e] += o.dz[4 + e]; v[12 + e] += o.dz[4 + e] * o.x[4 + e];
            }
        }
    }
    store_partials<4>(p, v, sh, FS, c4, prow, rows, n, slab0);
}

// ==== instance norm: the apply passes =============================================================================================
// pass 2 prologue: tot[k*FS + c] = the sample's sum k of channel slab0+c over all chunks, chunk order
template <int K>
__device__ __forceinline__ void gl_fold(const GruP& p, double* tot, int FS, int n, int slab0) {
    for (int i = threadIdx.x; i < K * FS; i += NT) {
        const int k = i / FS, cc = slab0 + i % FS;
        double t = 0.0;
        if (cc < p.F) {
            const double* w = p.ws + ((long long)n * p.nchunks * G2_K + k) * p.F + cc;
#pragma unroll 4
            for (int ch = 0; ch < p.nchunks; ++ch) t += w[(long long)ch * G2_K * p.F];
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

__global__ __launch_bounds__(NT) void grul_gates_fwd_apply(GruP p) {
    __shared__ double tot[4 * G2_SLAB];
    G2_GEOM();
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
        G2_TRIP();
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

__global__ __launch_bounds__(NT) void grul_out_fwd_apply(GruP p) {
    __shared__ double tot[2 * G2_SLAB];
    G2_GEOM();
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
        G2_TRIP();
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

__global__ __launch_bounds__(NT) void grul_out_bwd_apply(GruP p) {
    __shared__ double tot[2 * G2_SLAB];
    G2_GEOM();
    gl_fold<2>(p, tot, FS, n, slab0);
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * F + c0;
    float mu[4], rs[4], ga[4], be[4], sb[4], sg[4];
    out_stats<false>(p, n, c0, mu, rs);
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
        G2_TRIP();
        OutBwdPx o[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) out_bwd_px(p, n, pxs[j], c0, gp, mu, rs, ga, be, o[j]);
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

__global__ __launch_bounds__(NT) void grul_gates_bwd_apply(GruP p) {
    __shared__ double tot[4 * G2_SLAB];
    G2_GEOM();
    gl_fold<4>(p, tot, FS, n, slab0);
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
    float mu[8], rs[8], ga[8], be[8], sb[8], sg[8];
    gates_params<false>(p, n, c0, mu, rs, ga, be);
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
        G2_TRIP();
        GatesBwdPx o[2];
        float acc[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            gates_bwd_px(p, n, pxs[j], c0, gp, mu, rs, ga, be, o[j]);
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

// ==== layer norm: the apply passes ================================================================================================
// pass 2 prologue: tot[k*F + c] = the sample's sum k of channel c over all chunks, chunk order, for ALL F channels (the group's
// statistics need every slab's)
template <int K>
__device__ __forceinline__ void lg_fold(const GruP& p, double* tot, int n) {
    const long long step = (long long)G2_K * p.F;
    for (int i = threadIdx.x; i < K * p.F; i += NT) {
        const double* w = p.ws + (long long)n * p.nchunks * step + i;          // [k][c] of a chunk is contiguous: k*F + c = i
        double t = 0.0;
#pragma unroll 4
        for (int ch = 0; ch < p.nchunks; ++ch) t += w[ch * step];
        tot[i] = t;
    }
    __syncthreads();
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

__global__ __launch_bounds__(NT) void lng_gates_fwd_apply(GruP p) {
    extern __shared__ double tot[];                      // [4][F]
    __shared__ float gs[4];                              // mean, rstd of r; mean, rstd of u
    G2_GEOM();
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
        G2_TRIP();
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

__global__ __launch_bounds__(NT) void lng_out_fwd_apply(GruP p) {
    extern __shared__ double tot[];                      // [2][F]
    __shared__ float gs[2];
    G2_GEOM();
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
        G2_TRIP();
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

__global__ __launch_bounds__(NT) void lng_out_bwd_apply(GruP p) {
    extern __shared__ double tot[];                      // [2][F]
    __shared__ float gs[2];
    G2_GEOM();
    lg_fold<2>(p, tot, n);
    if (threadIdx.x < 64) lg_group_bwd(tot, tot + F, p.gamma, F, p.HW, gs);
    __syncthreads();
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * F + c0;
    const float ma = gs[0], mb = gs[1];
    float mu[4], rs[4], ga[4], be[4];
    out_stats<true>(p, n, c0, mu, rs);
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
        G2_TRIP();
        OutBwdPx o[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) out_bwd_px(p, n, pxs[j], c0, gp, mu, rs, ga, be, o[j]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = rs[e] * (ga[e] * o[j].dz[e] - ma - o[j].x[e] * mb);
            st4(p.dpre + ((long long)n * p.HW + pxs[j]) * F + c0, pack(d));
        }
    }
}

__global__ __launch_bounds__(NT) void lng_gates_bwd_apply(GruP p) {
    extern __shared__ double tot[];                      // [4][F]
    __shared__ float gs[4];                              // mean(gamma dz), mean(gamma dz xhat) of r; of u
    G2_GEOM();
    lg_fold<4>(p, tot, n);
    const int g = threadIdx.x >> 6;
    if (g < 2) lg_group_bwd(tot + 2 * g * F, tot + (2 * g + 1) * F, p.gamma + g * F, F, p.HW, gs + 2 * g);
    __syncthreads();
    if (!on) return;
    const float* gp = p.pre + (long long)n * p.HW * 2 * F + c0;
    float mu[8], rs[8], ga[8], be[8];
    gates_params<true>(p, n, c0, mu, rs, ga, be);
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
        G2_TRIP();
        GatesBwdPx o[2];
        float acc[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            gates_bwd_px(p, n, pxs[j], c0, gp, mu, rs, ga, be, o[j]);
            unpack(ld4(p.dh + (long long)n * p.dh_sn + (long long)pxs[j] * p.dh_sp + c0), acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j && !two) break;
            float d[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] += o[j].drhv[e] * o[j].rr[e];
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = rs[i] * (ga[i] * o[j].dz[i] - ma[i >> 2] - o[j].x[i] * mb[i >> 2]);
            st4(p.dh + (long long)n * p.dh_sn + (long long)pxs[j] * p.dh_sp + c0, pack(acc[j]));
            st4(dp + (long long)pxs[j] * 2 * F, make_float4(d[0], d[1], d[2], d[3]));
            st4(dp + (long long)pxs[j] * 2 * F + F, make_float4(d[4], d[5], d[6], d[7]));
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int fill(GruP& p, const SavpGruLargeArgs* L, GruChecks checks) {
    if (!L) return SAVP_EINVAL;
    const int rc = fill_gru(p, &L->g, checks);
    if (rc) return rc;
    if (!L->ws || (((uintptr_t)L->ws) & 7) || L->ws_bytes < savp_convgru_large_ws_bytes(p.N, p.HW, p.F)) return SAVP_EINVAL;
    p.chunk = savp_convgru_large_chunk(p.N, p.HW);
    p.nchunks = (p.HW + p.chunk - 1) / p.chunk;
    p.ws = (double*)L->ws;
    return SAVP_OK;
}

}  // namespace

// pixels per workgroup: about 512 workgroups per launch, between 32 and 256 pixels, and at most G2_MAX_CHUNKS chunks per plane
extern "C" int32_t savp_convgru_large_chunk(int32_t N, int32_t HW) {
    if (N < 1 || HW < 1) return 0;
    long long c = ((long long)N * HW + 511) / 512;
    if (c < 32) c = 32;
    if (c > 256) c = 256;
    if ((HW + c - 1) / c > G2_MAX_CHUNKS) c = ((long long)HW + G2_MAX_CHUNKS - 1) / G2_MAX_CHUNKS;
    return (int32_t)c;
}

extern "C" int64_t savp_convgru_large_ws_bytes(int32_t N, int32_t HW, int32_t F) {
    const int chunk = savp_convgru_large_chunk(N, HW);
    if (!chunk || F < 1) return 0;
    return (int64_t)N * ((HW + chunk - 1) / chunk) * G2_K * F * (int64_t)sizeof(double);
}

// the layer-norm blocks take the same chunks and the same workspace
extern "C" int32_t savp_convgru_ln_chunk(int32_t N, int32_t HW) { return savp_convgru_large_chunk(N, HW); }
extern "C" int64_t savp_convgru_ln_ws_bytes(int32_t N, int32_t HW, int32_t F) { return savp_convgru_large_ws_bytes(N, HW, F); }

// apply_lds: the dynamic LDS of the apply pass in bytes (the layer norm's K * F float64 totals)
#define GRU2P_ENTRY(name, checks, sums, apply, apply_lds, cond)                                                    \
    extern "C" int name(void* stream, const SavpGruLargeArgs* a) {                                                 \
        GruP p;                                                                                                    \
        int rc = fill(p, a, checks);                                                                                \
        if (rc) return rc;                                                                                          \
        if (!(cond)) return SAVP_EINVAL;                                                                            \
        const dim3 grid(p.nchunks, p.N, (p.F + G2_SLAB - 1) / G2_SLAB);                                             \
        hipLaunchKernelGGL(sums, grid, dim3(NT), 0, (hipStream_t)stream, p);                                        \
        hipLaunchKernelGGL(apply, grid, dim3(NT), apply_lds, (hipStream_t)stream, p);                               \
        return LAUNCH_OK();                                                                                         \
    }
// the operands of each block, beside what fill() checks
#define GATES_FWD_OK (vec_ok(p.u) && view_ok(p.rh, p.rh_sn, p.rh_sp))
#define OUT_FWD_OK (vec_ok(p.u) && p.nout >= 1)
#define OUT_BWD_OK (vec_ok(p.u) && vec_ok(p.du) && vec_ok(p.dpre) && view_ok(p.dh, p.dh_sn, p.dh_sp) && p.ndy >= 1 && p.dgamma && p.dbeta)
#define GATES_BWD_OK                                                                                               \
    (vec_ok(p.du) && vec_ok(p.dpre) && view_ok(p.dh, p.dh_sn, p.dh_sp) && view_ok(p.drh, p.drh_sn, p.drh_sp) && p.dgamma && p.dbeta)
GRU2P_ENTRY(savp_convgru_large_gates_fwd, GRU_LARGE, gru2p_gates_fwd_sums, grul_gates_fwd_apply, 0, GATES_FWD_OK)
GRU2P_ENTRY(savp_convgru_large_out_fwd, GRU_LARGE, gru2p_out_fwd_sums, grul_out_fwd_apply, 0, OUT_FWD_OK)
GRU2P_ENTRY(savp_convgru_large_out_bwd, GRU_LARGE, gru2p_out_bwd_sums<false>, grul_out_bwd_apply, 0, OUT_BWD_OK)
GRU2P_ENTRY(savp_convgru_large_gates_bwd, GRU_LARGE, gru2p_gates_bwd_sums<false>, grul_gates_bwd_apply, 0, GATES_BWD_OK)
GRU2P_ENTRY(savp_convgru_ln_gates_fwd, GRU_LN, gru2p_gates_fwd_sums, lng_gates_fwd_apply, 4 * p.F * sizeof(double), GATES_FWD_OK)
GRU2P_ENTRY(savp_convgru_ln_out_fwd, GRU_LN, gru2p_out_fwd_sums, lng_out_fwd_apply, 2 * p.F * sizeof(double), OUT_FWD_OK)
GRU2P_ENTRY(savp_convgru_ln_out_bwd, GRU_LN, gru2p_out_bwd_sums<true>, lng_out_bwd_apply, 2 * p.F * sizeof(double), OUT_BWD_OK)
GRU2P_ENTRY(savp_convgru_ln_gates_bwd, GRU_LN, gru2p_gates_bwd_sums<true>, lng_gates_bwd_apply, 4 * p.F * sizeof(double), GATES_BWD_OK)

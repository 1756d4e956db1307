// group_norm.hip -- normalisation + activation with statistics shared by groups of consecutive channels, forward and backward.
//
// G = 1 is tf.contrib.layers.layer_norm (mean / biased variance per sample over H, W and C; gamma / beta per channel), the reference's
// norm_layer = 'layer' (ops.py:1062-1074; savp_model.py:463-464,499-500,564-565,627-628; networks.py:26-27); G = C is the instance norm of
// norm_lstm.hip.  The instance-norm entries are untouched; these are separate entries with their own kernels.
//
// The statistics are per-(sample, channel) shifted sums in float64 -- either written by the producing convolution's epilogue
// (SavpConvArgs.stats, taken around that convolution's bias) or by a coalesced pass here (taken around the sample's first pixel) -- and a
// fold kernel combines them per (sample, group) with the parallel-variance identity
//     mean_g = mean over c of mean_c,   M2_g = sum_c (M2_c + HW * (mean_c - mean_g)^2),   var_g = M2_g / (HW * C/G)
// in float64 and a fixed order, so the result does not depend on the order in which workgroups arrived.  The backward pass folds the
// per-(sample, channel) sums sum(dz) and sum(dz * xhat) the same way, weighted by gamma.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"
#include "zero_fill.h"

#define GN_NT 256

namespace {

__device__ __forceinline__ float4 gn_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void gn_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// four consecutive elements at element index idx of a tensor that holds fp32 or (is16) bf16 (round to nearest even)
__device__ __forceinline__ void gn_st4x(float* base, long long idx, float4 v, int is16) {
    if (is16) {
        typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
        const bf16x4_t o = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
        *reinterpret_cast<bf16x4_t*>(reinterpret_cast<unsigned short*>(base) + idx) = o;
    } else {
        gn_st4(base + idx, v);
    }
}
__device__ __forceinline__ float gn_act(float v, int act, float alpha) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return fmaxf(v, alpha * v);
    if (act == 3) return v > 0.f ? v : expm1f(v);             // tf.nn.elu
    return v;
}
__device__ __forceinline__ float gn_act_grad(float z, int act, float alpha) {      // from the pre-activation: y > 0 <=> z > 0
    if (act == 1) return z > 0.f ? 1.f : 0.f;
    if (act == 2) return z > 0.f ? 1.f : alpha;
    if (act == 3) return z > 0.f ? 1.f : expf(z);             // ELU: no mask, the factor exp(z) where z <= 0
    return 1.f;
}

// float64 sum over the block in a fixed order (tree in shared memory); result valid in every thread
__device__ __forceinline__ double gn_block_sum(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = GN_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

struct GnP {
    int N, HW, C, G, Cg;            // Cg = C / G channels per group
    int chunk;                      // pixels per workgroup of the streaming passes
    int cq;                         // channel quads per workgroup (C/4 if <= 256, else 256); blockIdx.z = quad block
    const float* x; long long x_sn, x_sp;
    const float* gamma; const float* beta;
    float eps; int act; float alpha;
    int nout; float* out[4]; long long o_sn[4], o_sp[4];
    int o_c0[4], o_c1[4], o16[4];
    float* mean; float* rstd;       // [N, G]
    int ndy; const float* dy[4]; long long dy_sn[4], dy_sp[4];
    int dy_c0[4], dy_c1[4];
    float* dx; long long dx_sn, dx_sp; int dx_beta, dx16;
    double* dgamma; double* dbeta; double* dsum;
    double* ws;                     // [N][C][2] per-(sample, channel) sums
    double* wsg;                    // [N][G][2] per-(sample, group) backward sums
    int unshifted; const float* shift;
};

// mean / rstd of the groups of channels c .. c + 3 (a quad spans several groups when C/G < 4, e.g. G = C)
__device__ __forceinline__ void gn_quad_stats(const GnP& p, int n, int c, float4& m, float4& r) {
    const float* mp = p.mean + (long long)n * p.G;
    const float* rp = p.rstd + (long long)n * p.G;
    m = make_float4(mp[c / p.Cg], mp[(c + 1) / p.Cg], mp[(c + 2) / p.Cg], mp[(c + 3) / p.Cg]);
    r = make_float4(rp[c / p.Cg], rp[(c + 1) / p.Cg], rp[(c + 2) / p.Cg], rp[(c + 3) / p.Cg]);
}

// thread -> (channel quad, pixel row) of a streaming pass; false for the threads past the last row
__device__ __forceinline__ bool gn_lane(const GnP& p, int& c4, int& prow, int& rows) {
    rows = GN_NT / p.cq;
    c4 = blockIdx.z * p.cq + (int)threadIdx.x % p.cq;
    prow = (int)threadIdx.x / p.cq;
    return prow < rows;
}

// per-(sample, channel) sums of (x - x[pixel 0]) and its square -> ws (float64 atomics of fp32 workgroup partials: exact)
__global__ __launch_bounds__(GN_NT) void gn_stats_kernel(GnP p) {
    extern __shared__ float sh[];                 // [rows][2][4 * cq]
    int c4, prow, rows;
    const bool on = gn_lane(p, c4, prow, rows);
    const int n = blockIdx.y, W = 4 * p.cq;
    const float* x = p.x + (long long)n * p.x_sn + c4 * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
    if (on) {
        const float4 k = gn_ld4(x);
        const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk);
        for (int px = p0 + prow; px < p1; px += rows) {
            float4 v = gn_ld4(x + (long long)px * p.x_sp);
            v.x -= k.x; v.y -= k.y; v.z -= k.z; v.w -= k.w;
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            q.x += v.x * v.x; q.y += v.y * v.y; q.z += v.z * v.z; q.w += v.w * v.w;
        }
        float* d = sh + prow * 2 * W + ((int)threadIdx.x % p.cq) * 4;
        d[0] = s.x; d[1] = s.y; d[2] = s.z; d[3] = s.w;
        d[W] = q.x; d[W + 1] = q.y; d[W + 2] = q.z; d[W + 3] = q.w;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * W; i += GN_NT) {
        float t = 0.f;
        for (int r = 0; r < rows; ++r) t += sh[r * 2 * W + i];
        const int c = blockIdx.z * W + i % W, which = i / W;
        unsafeAtomicAdd(p.ws + ((long long)n * p.C + c) * 2 + which, (double)t);
    }
}

// per-(sample, group) mean / rstd from the per-channel sums (parallel-variance identity, float64, fixed order).  grid (G, N)
__global__ __launch_bounds__(GN_NT) void gn_fold_kernel(GnP p) {
    __shared__ double sh[GN_NT];
    const int g = blockIdx.x, n = blockIdx.y, c0 = g * p.Cg;
    const double hw = (double)p.HW;
    const float* x0 = p.x + (long long)n * p.x_sn;               // pixel 0 of the sample: the shift of a pass of our own
    auto mean_c = [&](int c, double& S, double& Q) -> double {
        const double* w = p.ws + ((long long)n * p.C + c) * 2;
        S = w[0]; Q = w[1];
        const double k = p.unshifted ? (p.shift ? (double)p.shift[c] : 0.0) : (double)x0[c];
        return k + S / hw;
    };
    double a = 0.0;
    for (int c = c0 + threadIdx.x; c < c0 + p.Cg; c += GN_NT) { double S, Q; a += mean_c(c, S, Q); }
    const double mg = gn_block_sum(a, sh) / (double)p.Cg;
    double m2 = 0.0;
    for (int c = c0 + threadIdx.x; c < c0 + p.Cg; c += GN_NT) {
        double S, Q;
        const double mc = mean_c(c, S, Q);
        m2 += fmax(Q - S * S / hw, 0.0) + hw * (mc - mg) * (mc - mg);
    }
    const double var = gn_block_sum(m2, sh) / (hw * (double)p.Cg);
    if (threadIdx.x == 0) {
        p.mean[(long long)n * p.G + g] = (float)mg;
        p.rstd[(long long)n * p.G + g] = (float)(1.0 / sqrt(var + (double)p.eps));
    }
}

__global__ __launch_bounds__(GN_NT) void gn_apply_kernel(GnP p) {
    int c4, prow, rows;
    if (!gn_lane(p, c4, prow, rows)) return;
    const int n = blockIdx.y, c = c4 * 4;
    float4 m, r;
    gn_quad_stats(p, n, c, m, r);
    const float4 gm = gn_ld4(p.gamma + c), bt = gn_ld4(p.beta + c);
    const float* x = p.x + (long long)n * p.x_sn + c;
    const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk);
    for (int px = p0 + prow; px < p1; px += rows) {
        const float4 v = gn_ld4(x + (long long)px * p.x_sp);
        float4 o;
        o.x = gn_act((v.x - m.x) * r.x * gm.x + bt.x, p.act, p.alpha);
        o.y = gn_act((v.y - m.y) * r.y * gm.y + bt.y, p.act, p.alpha);
        o.z = gn_act((v.z - m.z) * r.z * gm.z + bt.z, p.act, p.alpha);
        o.w = gn_act((v.w - m.w) * r.w * gm.w + bt.w, p.act, p.alpha);
        for (int k = 0; k < p.nout; ++k)
            if (c >= p.o_c0[k] && c < p.o_c1[k])
                gn_st4x(p.out[k], (long long)n * p.o_sn[k] + (long long)px * p.o_sp[k] + (c - p.o_c0[k]), o, p.o16[k]);
    }
}

// dz (= dL/d(gamma * xhat + beta), the activation's derivative applied) and xhat of one pixel of this thread's four channels
__device__ __forceinline__ float4 gn_dz(const GnP& p, int n, int px, int c, const float* x, float4 m, float4 r, float4 gm, float4 bt, float4& xh) {
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < p.ndy; ++k) {
        if (c < p.dy_c0[k] || c >= p.dy_c1[k]) continue;
        const float4 t = gn_ld4(p.dy[k] + (long long)n * p.dy_sn[k] + (long long)px * p.dy_sp[k] + (c - p.dy_c0[k]));
        d.x += t.x; d.y += t.y; d.z += t.z; d.w += t.w;
    }
    const float4 v = gn_ld4(x + (long long)px * p.x_sp);
    xh.x = (v.x - m.x) * r.x; xh.y = (v.y - m.y) * r.y; xh.z = (v.z - m.z) * r.z; xh.w = (v.w - m.w) * r.w;
    d.x *= gn_act_grad(xh.x * gm.x + bt.x, p.act, p.alpha); d.y *= gn_act_grad(xh.y * gm.y + bt.y, p.act, p.alpha);
    d.z *= gn_act_grad(xh.z * gm.z + bt.z, p.act, p.alpha); d.w *= gn_act_grad(xh.w * gm.w + bt.w, p.act, p.alpha);
    return d;
}

// per-(sample, channel) sum(dz), sum(dz * xhat) -> ws
__global__ __launch_bounds__(GN_NT) void gn_bwd_stats_kernel(GnP p) {
    extern __shared__ float sh[];
    int c4, prow, rows;
    const bool on = gn_lane(p, c4, prow, rows);
    const int n = blockIdx.y, W = 4 * p.cq, c = c4 * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
    if (on) {
        float4 m, r;
        gn_quad_stats(p, n, c, m, r);
        const float4 gm = gn_ld4(p.gamma + c), bt = gn_ld4(p.beta + c);
        const float* x = p.x + (long long)n * p.x_sn + c;
        const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk);
        for (int px = p0 + prow; px < p1; px += rows) {
            float4 xh;
            const float4 d = gn_dz(p, n, px, c, x, m, r, gm, bt, xh);
            s.x += d.x; s.y += d.y; s.z += d.z; s.w += d.w;
            q.x += d.x * xh.x; q.y += d.y * xh.y; q.z += d.z * xh.z; q.w += d.w * xh.w;
        }
        float* dd = sh + prow * 2 * W + ((int)threadIdx.x % p.cq) * 4;
        dd[0] = s.x; dd[1] = s.y; dd[2] = s.z; dd[3] = s.w;
        dd[W] = q.x; dd[W + 1] = q.y; dd[W + 2] = q.z; dd[W + 3] = q.w;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * W; i += GN_NT) {
        float t = 0.f;
        for (int rr = 0; rr < rows; ++rr) t += sh[rr * 2 * W + i];
        const int cc = blockIdx.z * W + i % W, which = i / W;
        unsafeAtomicAdd(p.ws + ((long long)n * p.C + cc) * 2 + which, (double)t);
    }
}

// per-(sample, group) sum_c gamma_c * sum(dz), sum_c gamma_c * sum(dz * xhat) -> wsg; dbeta / dgamma += the per-(sample, channel) sums
// (rounded to fp32 before the float64 atomic, as the instance norm does: exact, order-independent).  grid (G, N)
__global__ __launch_bounds__(GN_NT) void gn_bwd_fold_kernel(GnP p) {
    __shared__ double sh[GN_NT];
    const int g = blockIdx.x, n = blockIdx.y, c0 = g * p.Cg;
    double a = 0.0, b = 0.0;
    for (int c = c0 + threadIdx.x; c < c0 + p.Cg; c += GN_NT) {
        const double* w = p.ws + ((long long)n * p.C + c) * 2;
        const double s1 = w[0], s2 = w[1];
        a += (double)p.gamma[c] * s1;
        b += (double)p.gamma[c] * s2;
        unsafeAtomicAdd(p.dbeta + c, (double)(float)s1);
        unsafeAtomicAdd(p.dgamma + c, (double)(float)s2);
    }
    a = gn_block_sum(a, sh);
    b = gn_block_sum(b, sh);
    if (threadIdx.x == 0) {
        p.wsg[((long long)n * p.G + g) * 2] = a;
        p.wsg[((long long)n * p.G + g) * 2 + 1] = b;
    }
}

// dx = rstd * (gamma * dz - A / M - xhat * B / M), M = HW * C/G; optionally dsum[c] += sum over the workgroup's pixels of dx
__global__ __launch_bounds__(GN_NT) void gn_bwd_apply_kernel(GnP p) {
    extern __shared__ float sh[];                 // [rows][4 * cq] (dsum only)
    int c4, prow, rows;
    const bool on = gn_lane(p, c4, prow, rows);
    const int n = blockIdx.y, c = c4 * 4, W = 4 * p.cq;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) {
        float4 m, r;
        gn_quad_stats(p, n, c, m, r);
        const double invM = 1.0 / ((double)p.HW * (double)p.Cg);
        float A[4], B[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double* w = p.wsg + ((long long)n * p.G + (c + e) / p.Cg) * 2;
            A[e] = (float)(w[0] * invM); B[e] = (float)(w[1] * invM);
        }
        const float4 gm = gn_ld4(p.gamma + c), bt = gn_ld4(p.beta + c);
        const float* x = p.x + (long long)n * p.x_sn + c;
        const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk);
        for (int px = p0 + prow; px < p1; px += rows) {
            float4 xh;
            const float4 d = gn_dz(p, n, px, c, x, m, r, gm, bt, xh);
            float4 o;
            o.x = r.x * (gm.x * d.x - A[0] - xh.x * B[0]);
            o.y = r.y * (gm.y * d.y - A[1] - xh.y * B[1]);
            o.z = r.z * (gm.z * d.z - A[2] - xh.z * B[2]);
            o.w = r.w * (gm.w * d.w - A[3] - xh.w * B[3]);
            acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
            const long long e = (long long)n * p.dx_sn + (long long)px * p.dx_sp + c;
            if (p.dx16) { gn_st4x(p.dx, e, o, 1); continue; }
            if (p.dx_beta) { const float4 t = gn_ld4(p.dx + e); o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w; }
            gn_st4(p.dx + e, o);
        }
    }
    if (!p.dsum) return;                          // uniform over the block
    if (on) {
        float* d = sh + prow * W + ((int)threadIdx.x % p.cq) * 4;
        d[0] = acc.x; d[1] = acc.y; d[2] = acc.z; d[3] = acc.w;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < W; i += GN_NT) {
        float t = 0.f;
        for (int rr = 0; rr < rows; ++rr) t += sh[rr * W + i];
        unsafeAtomicAdd(p.dsum + blockIdx.z * W + i, (double)t);
    }
}

// the launch geometry shared by every streaming pass
static void gn_geometry(GnP& p, dim3& grid) {
    const int C4 = p.C / 4;
    p.cq = C4 <= GN_NT ? C4 : GN_NT;
    const int rows = GN_NT / p.cq;
    long long ch = ((long long)p.HW * p.N * (C4 / p.cq) + 511) / 512;     // ~512 workgroups, at least one pass of the rows, at most 256 pixels
    if (ch < rows) ch = rows;
    if (ch > 256) ch = 256;
    p.chunk = (int)ch;
    grid = dim3((p.HW + p.chunk - 1) / p.chunk, p.N, C4 / p.cq);
}

static int gn_common(GnP& p, const SavpGnormArgs* ga) {
    const SavpInormArgs* a = &ga->norm;
    if (a->N < 1 || a->HW < 1 || a->C < 4 || a->C % 4 || ga->G < 1 || a->C % ga->G) return SAVP_EINVAL;
    if (a->C / 4 > GN_NT && (a->C / 4) % GN_NT) return SAVP_EINVAL;
    if (!a->ws || (((uintptr_t)a->ws) & 7) || !a->x.p || !a->gamma || !a->beta || !a->mean || !a->rstd) return SAVP_EINVAL;
    if ((a->x.sn & 3) || (a->x.sp & 3) || (((uintptr_t)a->x.p) & 15)) return SAVP_EINVAL;
    p.N = a->N; p.HW = a->HW; p.C = a->C; p.G = ga->G; p.Cg = a->C / ga->G;
    p.x = (const float*)a->x.p; p.x_sn = a->x.sn; p.x_sp = a->x.sp;
    p.gamma = a->gamma; p.beta = a->beta; p.eps = a->eps; p.act = a->act; p.alpha = a->alpha;
    p.mean = a->mean; p.rstd = a->rstd;
    p.ws = (double*)a->ws; p.wsg = ga->ws_group; p.dsum = ga->dsum;
    p.nout = 0; p.ndy = 0;
    p.dx = nullptr; p.dx_sn = p.dx_sp = 0; p.dx_beta = p.dx16 = 0;
    p.dgamma = p.dbeta = nullptr;
    p.unshifted = 0; p.shift = nullptr;
    return SAVP_OK;
}

}  // namespace

extern "C" int savp_groupnorm_act_fwd(void* stream, const SavpGnormArgs* ga) {
    if (!ga) return SAVP_EINVAL;
    const SavpInormArgs* a = &ga->norm;
    GnP p;
    if (gn_common(p, ga) != SAVP_OK || a->nout < 1 || a->nout > 4) return SAVP_EINVAL;
    p.nout = a->nout;
    for (int i = 0; i < a->nout; ++i) {
        p.out[i] = (float*)a->out[i].p; p.o_sn[i] = a->out[i].sn; p.o_sp[i] = a->out[i].sp;
        p.o_c0[i] = a->out_c0[i]; p.o_c1[i] = a->out_nc[i] > 0 ? a->out_c0[i] + a->out_nc[i] : a->C;
        p.o16[i] = (a->out_bf16 >> i) & 1;
        if (!p.out[i] || (p.o_c0[i] & 3) || (p.o_c1[i] & 3) || p.o_c0[i] < 0 || p.o_c1[i] > a->C) return SAVP_EINVAL;
        // float4 / bf16x4 stores: 16-byte (fp32) or 8-byte (bf16) aligned base, strides in whole 4-element groups
        if ((a->out[i].sn & 3) || (a->out[i].sp & 3) || (((uintptr_t)p.out[i]) & (p.o16[i] ? 7 : 15))) return SAVP_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    dim3 grid;
    gn_geometry(p, grid);
    if (a->stats_ready) {
        p.unshifted = 1; p.shift = a->stats_shift;
    } else {
        if (!a->ws_clean) savp_zero_async(a->ws, (size_t)a->N * a->C * 2 * sizeof(double), st);
        const size_t lds = (size_t)(GN_NT / p.cq) * 2 * 4 * p.cq * sizeof(float);
        hipLaunchKernelGGL(gn_stats_kernel, grid, dim3(GN_NT), lds, st, p);
    }
    hipLaunchKernelGGL(gn_fold_kernel, dim3(p.G, p.N), dim3(GN_NT), 0, st, p);
    hipLaunchKernelGGL(gn_apply_kernel, grid, dim3(GN_NT), 0, st, p);
    return hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH;
}

extern "C" int savp_groupnorm_act_bwd(void* stream, const SavpGnormArgs* ga) {
    if (!ga) return SAVP_EINVAL;
    const SavpInormArgs* a = &ga->norm;
    GnP p;
    if (gn_common(p, ga) != SAVP_OK || a->ndy < 1 || a->ndy > 4) return SAVP_EINVAL;
    if (!ga->ws_group || (((uintptr_t)ga->ws_group) & 7) || !a->dx.p || !a->dgamma || !a->dbeta) return SAVP_EINVAL;
    if ((((uintptr_t)a->dgamma) & 7) || (((uintptr_t)a->dbeta) & 7) || (ga->dsum && (((uintptr_t)ga->dsum) & 7))) return SAVP_EINVAL;
    p.ndy = a->ndy;
    for (int i = 0; i < a->ndy; ++i) {
        p.dy[i] = (const float*)a->dy[i].p; p.dy_sn[i] = a->dy[i].sn; p.dy_sp[i] = a->dy[i].sp;
        p.dy_c0[i] = a->dy_c0[i]; p.dy_c1[i] = a->dy_nc[i] > 0 ? a->dy_c0[i] + a->dy_nc[i] : a->C;
        if (!p.dy[i] || (p.dy_c0[i] & 3) || (p.dy_c1[i] & 3) || p.dy_c0[i] < 0 || p.dy_c1[i] > a->C) return SAVP_EINVAL;
        if ((a->dy[i].sn & 3) || (a->dy[i].sp & 3) || (((uintptr_t)p.dy[i]) & 15)) return SAVP_EINVAL;        // float4 loads
    }
    p.dx = (float*)a->dx.p; p.dx_sn = a->dx.sn; p.dx_sp = a->dx.sp; p.dx_beta = a->dx_beta;
    p.dx16 = a->dx_bf16 ? 1 : 0;
    if (p.dx16 && (a->dx_beta || (a->dx.sn & 3) || (a->dx.sp & 3) || (((uintptr_t)a->dx.p) & 7))) return SAVP_EINVAL;
    if (!p.dx16 && ((a->dx.sn & 3) || (a->dx.sp & 3) || (((uintptr_t)a->dx.p) & 15))) return SAVP_EINVAL;
    p.dgamma = a->dgamma; p.dbeta = a->dbeta;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid;
    gn_geometry(p, grid);
    const size_t lds = (size_t)(GN_NT / p.cq) * 2 * 4 * p.cq * sizeof(float);
    if (!a->stats_ready) {
        if (!a->ws_clean) savp_zero_async(a->ws, (size_t)a->N * a->C * 2 * sizeof(double), st);
        hipLaunchKernelGGL(gn_bwd_stats_kernel, grid, dim3(GN_NT), lds, st, p);
    }
    hipLaunchKernelGGL(gn_bwd_fold_kernel, dim3(p.G, p.N), dim3(GN_NT), 0, st, p);
    hipLaunchKernelGGL(gn_bwd_apply_kernel, grid, dim3(GN_NT), ga->dsum ? lds / 2 : 0, st, p);
    return hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH;
}

// plain_act.hip -- the "normaliser" of a site whose norm_layer is the identity (norm_layer = 'none': ops.get_norm_layer('none') is
// tf.identity, ops.py:1062-1074; call sites savp_model.py:463-464,477,499-500,512,525,537,564,627, networks.py:25-27), forward and backward:
//     y  = act(x + add[n, c])                 add: the untiled latent's dense(z)[:, None, None, :] (savp_model.py:983-993), optional
//     dx = act'(x + add) * sum_k dy[k]        the mask / factor recomputed from x + add, no output read
// The convolution in front has already added its bias into x.  Pure streaming: every element is read once and written once, there is no
// statistics pass.  The optional column sums of dx (the gradient of `add` per sample, of the bias in front of the site over the samples)
// are taken without atomics: every workgroup leaves its float64 partial row in the caller's scratch (plain stores) and a fold launch adds
// the rows of a (sample, channel) in chunk order -- one writer per value, the same bits every run.
//
// Two instantiations: E = 4 (C % 4 == 0 and every view 4-element aligned: float4 / bf16x4 accesses) and E = 1 (anything else).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define PA_NT 256

namespace {

template <int E> struct PaVec;
template <> struct PaVec<4> {
    static __device__ __forceinline__ void ld(const float* p, float* v) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    // four consecutive elements at element index idx of a tensor that holds fp32 or (is16) bf16 (round to nearest even)
    static __device__ __forceinline__ void st(void* base, long long idx, const float* v, int is16) {
        if (is16) {
            typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
            const bf16x4_t o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
            *reinterpret_cast<bf16x4_t*>(reinterpret_cast<unsigned short*>(base) + idx) = o;
        } else {
            *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + idx) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
};
template <> struct PaVec<1> {
    static __device__ __forceinline__ void ld(const float* p, float* v) { v[0] = *p; }
    static __device__ __forceinline__ void st(void* base, long long idx, const float* v, int is16) {
        if (is16) reinterpret_cast<__bf16*>(base)[idx] = (__bf16)v[0];
        else reinterpret_cast<float*>(base)[idx] = v[0];
    }
};

__device__ __forceinline__ float pa_act(float v, int act, float alpha) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return v > 0.f ? v : alpha * v;
    if (act == 3) return v > 0.f ? v : expm1f(v);             // tf.nn.elu
    return v;
}
__device__ __forceinline__ float pa_act_grad(float z, int act, float alpha) {      // at z == 0: 0 for ReLU, alpha for LeakyReLU
    if (act == 1) return z > 0.f ? 1.f : 0.f;
    if (act == 2) return z > 0.f ? 1.f : alpha;
    if (act == 3) return z > 0.f ? 1.f : expf(z);
    return 1.f;
}

struct PaP {
    int N, HW, C, V;                // V = C / E columns of E channels
    int chunk, cq, nchunk;          // pixels per workgroup; columns per workgroup; workgroups per (sample, column block)
    const float* x; long long x_sn, x_sp;
    const float* add;               // [N][C] or NULL
    int act; float alpha;
    int nout; void* out[4]; long long o_sn[4], o_sp[4]; int o_c0[4], o_c1[4], o16[4];
    int ndy; const float* dy[4]; long long dy_sn[4], dy_sp[4]; int dy_c0[4], dy_c1[4];
    void* dx; long long dx_sn, dx_sp; int dx_beta, dx16;
    double* part;                   // [N][nchunk][C] partial rows of the column sums, or NULL
};

// thread -> (column, pixel row) of the workgroup's tile; false for the threads past the last whole row and past the last column
__device__ __forceinline__ bool pa_lane(const PaP& p, int& col, int& prow, int& rows) {
    rows = PA_NT / p.cq;
    col = blockIdx.z * p.cq + (int)threadIdx.x % p.cq;
    prow = (int)threadIdx.x / p.cq;
    return prow < rows && col < p.V;
}

template <int E>
__global__ __launch_bounds__(PA_NT) void pa_fwd_kernel(PaP p) {
    int col, prow, rows;
    if (!pa_lane(p, col, prow, rows)) return;
    const int c = col * E;
    const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        float ad[E];
#pragma unroll
        for (int e = 0; e < E; ++e) ad[e] = p.add ? p.add[(long long)n * p.C + c + e] : 0.f;
        const float* x = p.x + (long long)n * p.x_sn + c;
        for (int px = p0 + prow; px < p1; px += rows) {
            float v[E];
            PaVec<E>::ld(x + (long long)px * p.x_sp, v);
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = pa_act(v[e] + ad[e], p.act, p.alpha);
            for (int k = 0; k < p.nout; ++k)
                if (c >= p.o_c0[k] && c < p.o_c1[k])
                    PaVec<E>::st(p.out[k], (long long)n * p.o_sn[k] + (long long)px * p.o_sp[k] + (c - p.o_c0[k]), v, p.o16[k]);
        }
    }
}

template <int E>
__global__ __launch_bounds__(PA_NT) void pa_bwd_kernel(PaP p) {
    __shared__ double sh[PA_NT * E];              // [rows][cq * E] (column sums only)
    int col, prow, rows;
    const bool on = pa_lane(p, col, prow, rows);
    const int c = col * E, W = p.cq * E, lc = ((int)threadIdx.x % p.cq) * E;
    const int p0 = blockIdx.x * p.chunk, p1 = min(p.HW, p0 + p.chunk);
    for (int n = blockIdx.y; n < p.N; n += gridDim.y) {
        double acc[E];
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = 0.0;
        if (on) {
            float ad[E];
#pragma unroll
            for (int e = 0; e < E; ++e) ad[e] = p.add ? p.add[(long long)n * p.C + c + e] : 0.f;
            const float* x = p.x + (long long)n * p.x_sn + c;
            for (int px = p0 + prow; px < p1; px += rows) {
                float d[E], v[E];
#pragma unroll
                for (int e = 0; e < E; ++e) d[e] = 0.f;
                for (int k = 0; k < p.ndy; ++k) {
                    if (c < p.dy_c0[k] || c >= p.dy_c1[k]) continue;
                    PaVec<E>::ld(p.dy[k] + (long long)n * p.dy_sn[k] + (long long)px * p.dy_sp[k] + (c - p.dy_c0[k]), v);
#pragma unroll
                    for (int e = 0; e < E; ++e) d[e] += v[e];
                }
                PaVec<E>::ld(x + (long long)px * p.x_sp, v);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    d[e] *= pa_act_grad(v[e] + ad[e], p.act, p.alpha);
                    acc[e] += (double)d[e];                       // the fp32 gradient, before dx_beta's sum and any rounding to bf16
                }
                const long long o = (long long)n * p.dx_sn + (long long)px * p.dx_sp + c;
                if (p.dx_beta) {
                    PaVec<E>::ld(reinterpret_cast<const float*>(p.dx) + o, v);
#pragma unroll
                    for (int e = 0; e < E; ++e) d[e] += v[e];
                }
                PaVec<E>::st(p.dx, o, d, p.dx16);
            }
        }
        if (!p.part) continue;                        // uniform over the grid
        __syncthreads();                              // the previous sample's rows have been read
        if (on) {
#pragma unroll
            for (int e = 0; e < E; ++e) sh[prow * W + lc + e] = acc[e];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < W; i += PA_NT) {
            const int cc = blockIdx.z * W + i;
            if (cc >= p.C) continue;
            double t = 0.0;
            for (int r = 0; r < rows; ++r) t += sh[r * W + i];    // row order
            p.part[((long long)n * p.nchunk + blockIdx.x) * p.C + cc] = t;
        }
    }
}

// psum[n][c] += part[n][0][c] + part[n][1][c] + ... in chunk order
__global__ __launch_bounds__(PA_NT) void pa_fold_kernel(const double* __restrict__ part, double* __restrict__ psum, int nchunk, int C, long long NC) {
    const long long i = (long long)blockIdx.x * PA_NT + threadIdx.x;
    if (i >= NC) return;
    const long long n = i / C;
    const int c = (int)(i % C);
    double s = 0.0;
    for (int k = 0; k < nchunk; ++k) s += part[(n * nchunk + k) * C + c];
    psum[i] += s;
}

inline bool pa_al(const void* p, int bytes) { return (((uintptr_t)p) & (uintptr_t)(bytes - 1)) == 0; }
inline bool pa_view4(const SavpView& v, int is16) { return !(v.sn & 3) && !(v.sp & 3) && pa_al(v.p, is16 ? 8 : 16); }

// the part of the arguments both directions read; E is chosen by the caller from vec_ok
int pa_common(PaP& p, const SavpPlainActArgs* a, bool& vec_ok) {
    if (!a || a->N < 1 || a->HW < 1 || a->C < 1 || !a->x.p || a->act < 0 || a->act > 3) return SAVP_EINVAL;
    if (!pa_al(a->x.p, 4) || (a->add && !pa_al(a->add, 4))) return SAVP_EINVAL;
    p.N = a->N; p.HW = a->HW; p.C = a->C;
    p.x = (const float*)a->x.p; p.x_sn = a->x.sn; p.x_sp = a->x.sp;
    p.add = a->add; p.act = a->act; p.alpha = a->alpha;
    p.nout = p.ndy = 0;
    p.dx = nullptr; p.dx_sn = p.dx_sp = 0; p.dx_beta = p.dx16 = 0;
    p.part = nullptr; p.nchunk = 0;
    vec_ok = (a->C % 4 == 0) && pa_view4(a->x, 0);
    return SAVP_OK;
}

// the launch geometry of both streaming kernels: ~512 workgroups, each at least one pass of its rows and at most 256 pixels
int pa_geometry(PaP& p, int E, dim3& grid) {
    p.V = p.C / E;
    p.cq = p.V <= PA_NT ? p.V : PA_NT;
    const int rows = PA_NT / p.cq, zb = (p.V + p.cq - 1) / p.cq;
    if (zb > 65535) return SAVP_EINVAL;
    long long ch = ((long long)p.HW * p.N * zb + 511) / 512;
    if (ch < rows) ch = rows;
    if (ch > 256) ch = 256;
    p.chunk = (int)ch;
    grid = dim3((p.HW + p.chunk - 1) / p.chunk, p.N < 65535 ? p.N : 65535, zb);
    return SAVP_OK;
}

}  // namespace

extern "C" int savp_plain_act_fwd(void* stream, const SavpPlainActArgs* a) {
    PaP p;
    bool vec;
    if (pa_common(p, a, vec) != SAVP_OK || a->nout < 1 || a->nout > 4) return SAVP_EINVAL;
    p.nout = a->nout;
    for (int i = 0; i < a->nout; ++i) {
        p.out[i] = a->out[i].p; p.o_sn[i] = a->out[i].sn; p.o_sp[i] = a->out[i].sp;
        p.o_c0[i] = a->out_c0[i]; p.o_c1[i] = a->out_nc[i] > 0 ? a->out_c0[i] + a->out_nc[i] : a->C;
        p.o16[i] = (a->out_bf16 >> i) & 1;
        if (!p.out[i] || p.o_c0[i] < 0 || p.o_c1[i] > a->C || p.o_c0[i] >= p.o_c1[i] || !pa_al(p.out[i], p.o16[i] ? 2 : 4)) return SAVP_EINVAL;
        vec = vec && !(p.o_c0[i] & 3) && !(p.o_c1[i] & 3) && pa_view4(a->out[i], p.o16[i]);
    }
    dim3 grid;
    if (pa_geometry(p, vec ? 4 : 1, grid) != SAVP_OK) return SAVP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(pa_fwd_kernel<4>, grid, dim3(PA_NT), 0, st, p);
    else hipLaunchKernelGGL(pa_fwd_kernel<1>, grid, dim3(PA_NT), 0, st, p);
    return hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH;
}

extern "C" int savp_plain_act_bwd(void* stream, const SavpPlainActArgs* a) {
    PaP p;
    bool vec;
    if (pa_common(p, a, vec) != SAVP_OK || a->ndy < 1 || a->ndy > 4 || !a->dx.p) return SAVP_EINVAL;
    if (a->dx_beta != 0 && a->dx_beta != 1) return SAVP_EINVAL;
    p.ndy = a->ndy;
    for (int i = 0; i < a->ndy; ++i) {
        p.dy[i] = (const float*)a->dy[i].p; p.dy_sn[i] = a->dy[i].sn; p.dy_sp[i] = a->dy[i].sp;
        p.dy_c0[i] = a->dy_c0[i]; p.dy_c1[i] = a->dy_nc[i] > 0 ? a->dy_c0[i] + a->dy_nc[i] : a->C;
        if (!p.dy[i] || p.dy_c0[i] < 0 || p.dy_c1[i] > a->C || p.dy_c0[i] >= p.dy_c1[i] || !pa_al(p.dy[i], 4)) return SAVP_EINVAL;
        vec = vec && !(p.dy_c0[i] & 3) && !(p.dy_c1[i] & 3) && pa_view4(a->dy[i], 0);
    }
    p.dx = a->dx.p; p.dx_sn = a->dx.sn; p.dx_sp = a->dx.sp; p.dx_beta = a->dx_beta;
    p.dx16 = a->dx_bf16 ? 1 : 0;
    if ((p.dx16 && p.dx_beta) || !pa_al(p.dx, p.dx16 ? 2 : 4)) return SAVP_EINVAL;          // a bf16 dx is written, never added to
    vec = vec && pa_view4(a->dx, p.dx16);
    dim3 grid;
    if (pa_geometry(p, vec ? 4 : 1, grid) != SAVP_OK) return SAVP_EINVAL;
    if (a->psum) {
        if (!pa_al(a->psum, 8) || !a->ws || !pa_al(a->ws, 8)) return SAVP_EINVAL;
        const long long row = (long long)p.N * p.C * (long long)sizeof(double);
        const long long fit = a->ws_bytes / row;                 // partial rows per (sample, channel) the scratch holds
        if (fit < 1) return SAVP_EINVAL;
        if ((long long)grid.x > fit) {                            // fewer, longer chunks
            p.chunk = (int)((p.HW + fit - 1) / fit);
            grid.x = (p.HW + p.chunk - 1) / p.chunk;
        }
        p.part = a->ws; p.nchunk = (int)grid.x;
    }
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(pa_bwd_kernel<4>, grid, dim3(PA_NT), 0, st, p);
    else hipLaunchKernelGGL(pa_bwd_kernel<1>, grid, dim3(PA_NT), 0, st, p);
    if (a->psum) {
        const long long NC = (long long)p.N * p.C;
        hipLaunchKernelGGL(pa_fold_kernel, dim3((unsigned)((NC + PA_NT - 1) / PA_NT)), dim3(PA_NT), 0, st, (const double*)p.part, a->psum, p.nchunk, p.C, NC);
    }
    return hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH;
}

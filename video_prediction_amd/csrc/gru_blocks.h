// gru_blocks.h -- what the three families of Conv2DGRUCell gate blocks share: the device helpers, the kernel parameter struct and the
// host code that fills it from SavpGruArgs.  gru.hip (one workgroup per plane, and the pointwise blocks of the cell without a normaliser)
// and gru_two_pass.hip (chunked blocks for a plane of any size, instance norm and layer norm) include it.
// Every family has the same four blocks: gates_fwd, out_fwd, out_bwd, gates_bwd (include/savp_hip.h, SavpGruArgs).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define NT 256
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_(float x) {
    float e = __expf(-2.f * fabsf(x));
    return copysignf((1.f - e) / (1.f + e), x);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void unpack(const float4 v, float (&o)[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ float4 pack(const float (&o)[4]) { return make_float4(o[0], o[1], o[2], o[3]); }
// sum over the 64 lanes of a wave, the same bits in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct GruP {
    int N, HW, F;
    int chunk, nchunks;                                  // two-pass blocks only: pixels per workgroup, workgroups per plane
    float eps;
    const float* pre;                                    // gates stage: [N,HW,2F]; output stage: [N,HW,F]
    const float* h; long long h_sn, h_sp;                // h_prev view (never null: zero state is a zero buffer)
    const float *gamma, *beta;                           // [2F] (reset | update) / [F]
    float *mean, *rstd;                                  // instance norm: [N,2F] / [N,F]; layer norm: [N,2] / [N,1]
    float* u;                                            // [N,HW,F] contiguous (gates: written, output: read)
    float* rh; long long rh_sn, rh_sp;                   // gates fwd: r*h destination view
    int nout; float* out[4]; long long o_sn[4], o_sp[4]; // output fwd: h' destinations
    // backward
    int ndy; const float* dy[4]; long long dy_sn[4], dy_sp[4];
    float* dpre;                                         // [N,HW,F] or [N,HW,2F]
    float* du;                                           // output bwd: d u (post-sigmoid) [N,HW,F]; gates bwd reads it
    float* dh; long long dh_sn, dh_sp;                   // gradient of h_prev: out bwd overwrites it (u*dh'), gates bwd adds d(rh)*r
    const float* drh; long long drh_sn, drh_sp;          // gates bwd: gradient of the r*h slot
    double *dgamma, *dbeta;                              // float64 accumulators (savp_hip.h SavpGruArgs)
    double* ws;                                          // two-pass blocks only: [N][nchunks][4][F] per-chunk partial sums
};

// ---- host ------------------------------------------------------------------------------------------------------------------------
// a float4 at every (sample, pixel, 4-channel group) of a view needs a 16-byte base and strides that are multiples of 4 floats
static inline bool al16(const void* q) { return (((uintptr_t)q) & 15) == 0; }
static inline bool vec_ok(const void* q) { return q && al16(q); }
static inline bool view_ok(const void* q, long long sn, long long sp) { return q && al16(q) && sn % 4 == 0 && sp % 4 == 0; }
static inline bool f32_ok(const void* q) { return q && (((uintptr_t)q) & 3) == 0; }

// What fill_gru refuses (SAVP_EINVAL, before any launch) beside what every family refuses.  The entries add the operands of their block.
enum GruChecks {
    GRU_SMALL,            // gru.hip's one-workgroup blocks: no alignment checks (the entry caps HW)
    GRU_PLAIN,            // the pointwise blocks: N >= 1, float4 access to pre and to every view
    GRU_LARGE,            // two-pass instance norm: GRU_PLAIN, F >= 4, N <= 65535 (a grid dimension), gamma / beta / mean / rstd read as float4
    GRU_LN                // two-pass layer norm: GRU_LARGE with F <= GRU_LN_MAX_F and mean / rstd [N][G] read one float at a time
};
#define GRU_LN_MAX_F 1024             // the layer-norm apply pass holds 4 * F float64 totals in LDS (32 KB at the most)

static inline int fill_gru(GruP& p, const SavpGruArgs* a, GruChecks checks) {
    if (!a || a->F % 4 || a->HW < 1 || !a->pre || !a->h.p) return SAVP_EINVAL;
    if (a->nout < 0 || a->nout > 4 || a->ndy < 0 || a->ndy > 4) return SAVP_EINVAL;
    if (checks != GRU_SMALL) {
        if (a->N < 1 || !al16(a->pre) || !view_ok(a->h.p, a->h.sn, a->h.sp)) return SAVP_EINVAL;
        for (int i = 0; i < a->nout; ++i) if (!view_ok(a->out[i].p, a->out[i].sn, a->out[i].sp)) return SAVP_EINVAL;
        for (int i = 0; i < a->ndy; ++i) if (!view_ok(a->dy[i].p, a->dy[i].sn, a->dy[i].sp)) return SAVP_EINVAL;
    }
    if (checks == GRU_LARGE || checks == GRU_LN) {
        if (a->F < 4 || a->N > 65535 || !vec_ok(a->gamma) || !vec_ok(a->beta)) return SAVP_EINVAL;
        if (checks == GRU_LN ? (a->F > GRU_LN_MAX_F || !f32_ok(a->mean) || !f32_ok(a->rstd)) : (!vec_ok(a->mean) || !vec_ok(a->rstd)))
            return SAVP_EINVAL;
    }
    p.N = a->N; p.HW = a->HW; p.F = a->F; p.eps = a->eps;
    p.pre = a->pre;
    p.h = (const float*)a->h.p; p.h_sn = a->h.sn; p.h_sp = a->h.sp;
    p.gamma = a->gamma; p.beta = a->beta; p.mean = a->mean; p.rstd = a->rstd;
    p.u = a->u;
    p.rh = (float*)a->rh.p; p.rh_sn = a->rh.sn; p.rh_sp = a->rh.sp;
    p.nout = a->nout;
    for (int i = 0; i < a->nout; ++i) { p.out[i] = (float*)a->out[i].p; p.o_sn[i] = a->out[i].sn; p.o_sp[i] = a->out[i].sp; }
    p.ndy = a->ndy;
    for (int i = 0; i < a->ndy; ++i) { p.dy[i] = (const float*)a->dy[i].p; p.dy_sn[i] = a->dy[i].sn; p.dy_sp[i] = a->dy[i].sp; }
    p.dpre = a->dpre; p.du = a->du;
    p.dh = (float*)a->dh.p; p.dh_sn = a->dh.sn; p.dh_sp = a->dh.sp;
    p.drh = (const float*)a->drh.p; p.drh_sn = a->drh.sn; p.drh_sp = a->drh.sp;
    p.dgamma = a->dgamma; p.dbeta = a->dbeta;
    p.chunk = p.nchunks = 0; p.ws = nullptr;             // the two-pass entries set them
    return SAVP_OK;
}

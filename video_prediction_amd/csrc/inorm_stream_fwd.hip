// inorm_stream_fwd.hip -- the coalesced instance norm's forward apply pass, specialised on the channel count, the activation, the pixel rows per
// thread and the number of outputs (inorm_stream.h).  Against inorm_apply_kernel (norm_lstm.hip), which it matches bit for bit:
//   * every x load of a thread is issued first; the statistics loads and their float64 finalisation follow while those are in flight, so a
//     workgroup pays one memory round trip before its first store instead of two;
//   * a thread's R pixel rows are all loaded before anything is stored: no trip waits for the previous trip's stores;
//   * each output's channel-range test is made once per thread, its dtype is a flag that is the same for every lane; rows past the plane are not loaded;
//   * the argument block holds what the specialisation reads (128 / 160 / 192 bytes for 1 / 2 / 3 outputs instead of 440).
#include "inorm_stream.h"

namespace inorm_stream {

template <int NOUT>
struct FwdP {
    const float* x; long long x_sn, x_sp;
    const double* ws; const float* shift;          // shift: the unshifted sums' per-channel offset (NULL: 0)
    const float* gamma; const float* beta;
    float* mean; float* rstd;
    int HW, unshifted; float eps, alpha;
    int m16, pad_;                                  // bit k: output k is a bf16 tensor
    struct { float* p; long long sn, sp; int c0, c1; } o[NOUT];      // sn, sp in elements of the output's dtype
};

// grid (ceil(HW / (R * 256 / C4)), N).  Lane mapping of the generic kernel: C4 adjacent lanes x 16 B cover one pixel row.
template <int C4, int ACT, int R, int NOUT>
__global__ __launch_bounds__(INORM_NT) void inorm_apply_fast_kernel(const FwdP<NOUT> p) {
    // Which multiply-adds the compiler fuses depends on the code around them, and every instantiation is another surrounding.  So nothing is fused
    // here on its own, and the two fused multiply-adds of inorm_apply_kernel's code are written out: w[1] * inv - ms * ms in float64 and
    // xhat * gamma + beta.
#pragma clang fp contract(off)
    constexpr int ROWS = INORM_NT / C4, C = C4 * 4;
    const int n = blockIdx.y, c = (threadIdx.x % C4) * 4, prow = threadIdx.x / C4;
    const int px0 = blockIdx.x * (R * ROWS) + prow;
    const float* xs = p.x + (long long)n * p.x_sn + c;
    float4 v[R];                                    // a row past the plane is neither loaded nor used (a zero fill would make each load a merge
#pragma unroll                                      // of two values, which can cost a register copy with a wait right behind the load)
    for (int j = 0; j < R; ++j)
        if (px0 + j * ROWS < p.HW) v[j] = ld4(xs + (long long)(px0 + j * ROWS) * p.x_sp);
    bool cov[NOUT];
    float* ob[NOUT];
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        cov[k] = c >= p.o[k].c0 && c < p.o[k].c1;
        const long long off = (long long)n * p.o[k].sn + (c - p.o[k].c0);
        ob[k] = (p.m16 >> k) & 1 ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(p.o[k].p) + off) : p.o[k].p + off;
    }
    const float4 g = ld4(p.gamma + c), b = ld4(p.beta + c);
    const float4 k4 = p.unshifted ? (p.shift ? ld4(p.shift + c) : make_float4(0.f, 0.f, 0.f, 0.f)) : ld4(xs);
    const float inv = 1.f / (float)p.HW;
    float m[4], r[4];
    const float kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double* w = p.ws + ((long long)n * C + c + e) * 2;
        const double ms = w[0] * (double)inv;
        const float var = fmaxf((float)fma(w[1], (double)inv, -(ms * ms)), 0.f);
        m[e] = kk[e] + (float)ms; r[e] = rsqrtf(var + p.eps);
    }
    // Every load has been requested and the finalisation above needed the last of them: wait for all of them HERE, once.  The stores below sit
    // in per-row branches; a load still pending there makes the compiler wait with vmcnt(0) in every branch, and on gfx950 that also waits for
    // the previous row's stores (vmcnt counts them).  0x0F70 = vmcnt(0) alone in the gfx9 encoding of s_waitcnt, which gfx950 uses (the build
    // compiles for gfx950 only).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (blockIdx.x == 0 && prow == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { p.mean[(long long)n * C + c + e] = m[e]; p.rstd[(long long)n * C + c + e] = r[e]; }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int px = px0 + j * ROWS;
        if (px >= p.HW) break;
        float4 o;
        o.x = act_fwd<ACT>(fmaf((v[j].x - m[0]) * r[0], g.x, b.x), p.alpha);
        o.y = act_fwd<ACT>(fmaf((v[j].y - m[1]) * r[1], g.y, b.y), p.alpha);
        o.z = act_fwd<ACT>(fmaf((v[j].z - m[2]) * r[2], g.z, b.z), p.alpha);
        o.w = act_fwd<ACT>(fmaf((v[j].w - m[3]) * r[3], g.w, b.w), p.alpha);
#pragma unroll
        for (int k = 0; k < NOUT; ++k)
            if (cov[k]) {                           // the dtype is the same for every lane: a scalar branch, no load is pending here
                if ((p.m16 >> k) & 1) st4t<true>(ob[k], (long long)px * p.o[k].sp, o);
                else st4t<false>(ob[k], (long long)px * p.o[k].sp, o);
            }
    }
}

template <int C4, int ACT, int R, int NOUT>
static int launch_nout(hipStream_t st, const SavpInormArgs* a, int unshifted) {
    FwdP<NOUT> p;
    p.x = (const float*)a->x.p; p.x_sn = a->x.sn; p.x_sp = a->x.sp;
    p.ws = (const double*)a->ws; p.shift = unshifted ? a->stats_shift : nullptr;
    p.gamma = a->gamma; p.beta = a->beta; p.mean = a->mean; p.rstd = a->rstd;
    p.HW = a->HW; p.unshifted = unshifted; p.eps = a->eps; p.alpha = a->alpha;
    for (int k = 0; k < NOUT; ++k) {
        p.o[k].p = (float*)a->out[k].p; p.o[k].sn = a->out[k].sn; p.o[k].sp = a->out[k].sp;
        p.o[k].c0 = a->out_c0[k]; p.o[k].c1 = a->out_nc[k] > 0 ? a->out_c0[k] + a->out_nc[k] : a->C;
    }
    p.m16 = a->out_bf16 & ((1 << NOUT) - 1); p.pad_ = 0;
    constexpr int PX = R * (INORM_NT / C4);
    hipLaunchKernelGGL((inorm_apply_fast_kernel<C4, ACT, R, NOUT>), dim3((a->HW + PX - 1) / PX, a->N), dim3(INORM_NT), 0, st, p);
    return 1;
}

template <int C4, int ACT, int R>
static int launch_r(hipStream_t st, const SavpInormArgs* a, int unshifted) {
    switch (a->nout) {
        case 1: return launch_nout<C4, ACT, R, 1>(st, a, unshifted);
        case 2: return launch_nout<C4, ACT, R, 2>(st, a, unshifted);
        case 3: return launch_nout<C4, ACT, R, 3>(st, a, unshifted);
    }
    return 0;
}

template <int C4, int ACT>
static int launch_act(hipStream_t st, const SavpInormArgs* a, int chunk, int unshifted) {
    // a generic chunk is at most 256 pixels = C4 rows per thread: more rows than that are never picked and not instantiated (C = 8: 1 or 2)
    switch (rows_per_thread(chunk, INORM_NT / C4, 8)) {
        case 1: return launch_r<C4, ACT, 1>(st, a, unshifted);
        case 2: return launch_r<C4, ACT, 2>(st, a, unshifted);
        case 4: if constexpr (C4 >= 4) return launch_r<C4, ACT, 4>(st, a, unshifted); else return 0;
        case 8: if constexpr (C4 >= 8) return launch_r<C4, ACT, 8>(st, a, unshifted); else return 0;
    }
    return 0;
}

template <int C4>
static int launch_c4(hipStream_t st, const SavpInormArgs* a, int chunk, int unshifted) {
    switch (a->act) {
        case 0: return launch_act<C4, 0>(st, a, chunk, unshifted);
        case 1: return launch_act<C4, 1>(st, a, chunk, unshifted);
        case 2: return launch_act<C4, 2>(st, a, chunk, unshifted);
    }
    return 0;                                       // ELU: the generic kernel
}

}  // namespace inorm_stream

int inorm_fast_fwd(hipStream_t st, const SavpInormArgs* a, int chunk, int unshifted) {
    using namespace inorm_stream;
    if (a->nout > 3) return 0;
    switch (a->C) {
        case 8: return launch_c4<2>(st, a, chunk, unshifted);
        case 32: return launch_c4<8>(st, a, chunk, unshifted);
        case 64: return launch_c4<16>(st, a, chunk, unshifted);
        case 128: return launch_c4<32>(st, a, chunk, unshifted);
        case 256: return launch_c4<64>(st, a, chunk, unshifted);
    }
    return 0;
}

// inorm_stream.h -- shape-specialised apply passes of the coalesced instance norm (inorm_stream_fwd.hip / inorm_stream_bwd.hip), dispatched
// from savp_instnorm_act_fwd / _bwd in norm_lstm.hip under option "inorm_fast".  They compute what inorm_apply_kernel /
// inorm_bwd_apply_kernel compute, element by element with the same expressions, so the two paths give the same bits; what a
// specialisation does not cover (returns 0) stays on the generic kernels: C other than 8 / 32 / 64 / 128 / 256, ELU, four outputs or gradient views.
#pragma once
#include <hip/hip_runtime.h>
#include "savp_hip.h"

#define INORM_NT 256

// 1: launched; 0: not covered (nothing launched).  ws: the per-(sample, channel) float64 sums [N][C][2].
// fwd: unshifted / shift as inorm_apply_kernel's (sums around `shift`, NULL = around 0; otherwise around the sample's first pixel).
// chunk: the generic launch's pixels per workgroup (inorm_chunk), from which the rows per thread are chosen.
int inorm_fast_fwd(hipStream_t st, const SavpInormArgs* a, int chunk, int unshifted);
int inorm_fast_bwd(hipStream_t st, const SavpInormArgs* a, int chunk);

#ifdef __HIPCC__
namespace inorm_stream {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// four consecutive elements to a tensor that holds fp32 or (B16) bf16, round to nearest even (norm_lstm.hip: st4x); idx in elements
template <bool B16>
__device__ __forceinline__ void st4t(float* base, long long idx, float4 v) {
    if (B16) {
        typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
        const bf16x4_t o = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
        *reinterpret_cast<bf16x4_t*>(reinterpret_cast<unsigned short*>(base) + idx) = o;
    } else {
        *reinterpret_cast<float4*>(base + idx) = v;
    }
}
// norm_lstm.hip: act_fwd / act_grad_from_out without ELU (act 3 stays on the generic kernels)
template <int ACT> __device__ __forceinline__ float act_fwd(float v, float alpha) {
    if (ACT == 1) return fmaxf(v, 0.f);
    if (ACT == 2) return fmaxf(v, alpha * v);
    return v;
}
template <int ACT> __device__ __forceinline__ float act_grad(float y, float alpha) {
    if (ACT == 1) return y > 0.f ? 1.f : 0.f;
    if (ACT == 2) return y > 0.f ? 1.f : alpha;
    return 1.f;
}

// pixel rows per thread: the smallest of 1, 2, 4, .. RMAX that covers what a thread of the generic launch walks through, so that small planes
// load nothing twice and the large ones have RMAX rows in flight (the grid grows instead where RMAX rows do not reach)
inline int rows_per_thread(int chunk, int rows, int rmax) {
    const int ppt = (chunk + rows - 1) / rows;
    int r = 1;
    while (r < ppt && r < rmax) r *= 2;
    return r;
}

}  // namespace inorm_stream
#endif

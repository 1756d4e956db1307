// ln_lstm.hip -- the pointwise parts of BasicConv2DLSTMCell with separate_norms (conv_rnn_norm_layer = 'layer', rnn_ops.py:147-165):
//   g = [LN(i) | LN(j) | LN(f) | LN(o)]  (savp_groupnorm_act_fwd, G = 4, on the gate convolution's output)
//   c_pre = c * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j)          stage 0 of savp_lnlstm_fwd
//   c' = LN(c_pre)                                                       (savp_groupnorm_act_fwd, G = 1)
//   h' = tanh(c') * sigmoid(o)                                           stage 1 of savp_lnlstm_fwd
// and their gradients (savp_lnlstm_bwd stage 0: dc' and dg[o]; stage 1: dg[i, j, f] and dc_prev from dc_pre).  One thread per
// (sample, pixel, channel); no reductions, so the results are bit-reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"

#define LL_NT 256

namespace {

__device__ __forceinline__ float ll_sig(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float ll_tanh(float x) {
    const float e = __expf(-2.f * fabsf(x));
    return copysignf((1.f - e) / (1.f + e), x);
}
__device__ __forceinline__ float ll_ld(const SavpView& v, long long n, long long px, int c, int is16) {
    const long long i = n * v.sn + px * v.sp + c;
    if (is16) return __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(v.p)[i] << 16);
    return reinterpret_cast<const float*>(v.p)[i];
}
__device__ __forceinline__ void ll_st(const SavpView& v, long long n, long long px, int c, float x, int is16) {
    const long long i = n * v.sn + px * v.sp + c;
    if (is16) reinterpret_cast<__bf16*>(v.p)[i] = (__bf16)x;
    else reinterpret_cast<float*>(v.p)[i] = x;
}

__global__ __launch_bounds__(LL_NT) void ll_fwd_kernel(SavpLnLstmArgs a, int stage) {
    const long long tot = (long long)a.N * a.HW * a.F;
    const long long e = (long long)blockIdx.x * LL_NT + threadIdx.x;
    if (e >= tot) return;
    const int c = (int)(e % a.F);
    const long long np = e / a.F, px = np % a.HW, n = np / a.HW;
    const float* g = a.gn + np * 4 * a.F;
    if (stage == 0) {
        const float cp = a.c_prev.p ? ll_ld(a.c_prev, n, px, c, 0) : 0.f;
        a.c_pre[e] = cp * ll_sig(g[2 * a.F + c] + a.forget_bias) + ll_sig(g[c]) * ll_tanh(g[a.F + c]);
    } else {
        const float h = ll_tanh(a.cn[e]) * ll_sig(g[3 * a.F + c]);
        for (int k = 0; k < a.nh; ++k) ll_st(a.h[k], n, px, c, h, (a.h_bf16 >> k) & 1);
    }
}

__global__ __launch_bounds__(LL_NT) void ll_bwd_kernel(SavpLnLstmArgs a, int stage) {
    const long long tot = (long long)a.N * a.HW * a.F;
    const long long e = (long long)blockIdx.x * LL_NT + threadIdx.x;
    if (e >= tot) return;
    const int c = (int)(e % a.F);
    const long long np = e / a.F, px = np % a.HW, n = np / a.HW;
    const float* g = a.gn + np * 4 * a.F;
    float* dg = a.dgn + np * 4 * a.F;
    if (stage == 0) {
        float dh = 0.f;
        for (int k = 0; k < a.ndh; ++k) dh += ll_ld(a.dh[k], n, px, c, 0);
        const float tc = ll_tanh(a.cn[e]), so = ll_sig(g[3 * a.F + c]);
        a.dcn[e] = (a.dc_new ? a.dc_new[e] : 0.f) + dh * so * (1.f - tc * tc);
        dg[3 * a.F + c] = dh * tc * so * (1.f - so);
    } else {
        const float d = a.dc_pre[e];
        const float si = ll_sig(g[c]), tj = ll_tanh(g[a.F + c]), sf = ll_sig(g[2 * a.F + c] + a.forget_bias);
        const float cp = a.c_prev.p ? ll_ld(a.c_prev, n, px, c, 0) : 0.f;
        dg[c] = d * tj * si * (1.f - si);
        dg[a.F + c] = d * si * (1.f - tj * tj);
        dg[2 * a.F + c] = d * cp * sf * (1.f - sf);
        if (a.dc_prev) a.dc_prev[e] = d * sf;
    }
}

int ll_check(const SavpLnLstmArgs* a, int stage) {
    if (!a || a->N < 1 || a->HW < 1 || a->F < 1 || !a->gn || stage < 0 || stage > 1) return SAVP_EINVAL;
    return SAVP_OK;
}

}  // namespace

extern "C" int savp_lnlstm_fwd(void* stream, const SavpLnLstmArgs* a, int32_t stage) {
    if (ll_check(a, stage) != SAVP_OK) return SAVP_EINVAL;
    if (stage == 0 && !a->c_pre) return SAVP_EINVAL;
    if (stage == 1 && (!a->cn || a->nh < 1 || a->nh > 4)) return SAVP_EINVAL;
    for (int k = 0; stage == 1 && k < a->nh; ++k)
        if (!a->h[k].p) return SAVP_EINVAL;
    const long long tot = (long long)a->N * a->HW * a->F;
    hipLaunchKernelGGL(ll_fwd_kernel, dim3((unsigned)((tot + LL_NT - 1) / LL_NT)), dim3(LL_NT), 0, (hipStream_t)stream, *a, (int)stage);
    return hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH;
}

extern "C" int savp_lnlstm_bwd(void* stream, const SavpLnLstmArgs* a, int32_t stage) {
    if (ll_check(a, stage) != SAVP_OK || !a->dgn) return SAVP_EINVAL;
    if (stage == 0 && (!a->cn || !a->dcn || a->ndh < 0 || a->ndh > 4)) return SAVP_EINVAL;
    for (int k = 0; stage == 0 && k < a->ndh; ++k)
        if (!a->dh[k].p) return SAVP_EINVAL;
    if (stage == 1 && !a->dc_pre) return SAVP_EINVAL;
    const long long tot = (long long)a->N * a->HW * a->F;
    hipLaunchKernelGGL(ll_bwd_kernel, dim3((unsigned)((tot + LL_NT - 1) / LL_NT)), dim3(LL_NT), 0, (hipStream_t)stream, *a, (int)stage);
    return hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH;
}

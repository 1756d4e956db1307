// inorm_stream_bwd.hip -- the coalesced instance norm's backward apply pass, specialised on the channel count, the activation, the pixel rows per
// thread, the number of gradient views and the form of dx (inorm_stream.h).  Against inorm_bwd_apply_kernel (norm_lstm.hip), which it matches
// bit for bit (see the note on fused multiply-adds in the kernel): each view's channel-range test is made once per thread; x, every covering dy and (dx_beta) the old dx of all R pixel rows are
// requested before the statistics are read and before anything is stored; rows past the plane are not loaded; the argument block shrinks
// from 424 to 144 / 176 / 208 bytes.  dgamma / dbeta: the same one float64 atomic per (sample, channel), from the sample's first workgroup.
#include "inorm_stream.h"

namespace inorm_stream {

template <int NDY>
struct BwdP {
    const float* x; long long x_sn, x_sp;
    const double* ws;
    const float* gamma; const float* beta;
    const float* mean; const float* rstd;
    float* dx; long long dx_sn, dx_sp;              // in elements of dx's dtype
    double* dgamma; double* dbeta;
    int HW; float alpha;
    struct { const float* p; long long sn, sp; int c0, c1; } dy[NDY];
};

enum { DX_F32 = 0, DX_F32_ACC = 1, DX_BF16 = 2 };

template <int C4, int ACT, int R, int NDY, int DXM>
__global__ __launch_bounds__(INORM_NT) void inorm_bwd_apply_fast_kernel(const BwdP<NDY> p) {
    // Which multiply-adds the compiler fuses depends on the code around them: with dx_beta and the activation known at compile time it fused
    // s1 * inv into d - s1 and gamma * xhat into + beta, and dx came out one unit in the last place off inorm_bwd_apply_kernel's.  So nothing is
    // fused here on its own, and the ONE fused multiply-add of the generic kernel's code (- xhat * s2 onto d - s1) is written out.
#pragma clang fp contract(off)
    constexpr int ROWS = INORM_NT / C4, C = C4 * 4;
    const int n = blockIdx.y, c = (threadIdx.x % C4) * 4, prow = threadIdx.x / C4;
    const int px0 = blockIdx.x * (R * ROWS) + prow;
    const float* xs = p.x + (long long)n * p.x_sn + c;
    float* dxs = DXM == DX_BF16 ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(p.dx) + ((long long)n * p.dx_sn + c))
                                : p.dx + (long long)n * p.dx_sn + c;
    bool cov[NDY];
    const float* db[NDY];
#pragma unroll
    for (int k = 0; k < NDY; ++k) {
        cov[k] = !(c < p.dy[k].c0 || c >= p.dy[k].c1);
        db[k] = p.dy[k].p + (long long)n * p.dy[k].sn + (c - p.dy[k].c0);
    }
    // a row past the plane, or a view that does not cover the channels, is neither loaded nor used (a zero fill would make each load a merge of
    // two values, which can cost a register copy with a wait right behind the load)
    float4 v[R], t[NDY][R], old[R];
#pragma unroll
    for (int j = 0; j < R; ++j)
        if (px0 + j * ROWS < p.HW) v[j] = ld4(xs + (long long)(px0 + j * ROWS) * p.x_sp);
#pragma unroll
    for (int k = 0; k < NDY; ++k)
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (cov[k] && px0 + j * ROWS < p.HW) t[k][j] = ld4(db[k] + (long long)(px0 + j * ROWS) * p.dy[k].sp);
    if (DXM == DX_F32_ACC) {
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (px0 + j * ROWS < p.HW) old[j] = ld4(dxs + (long long)(px0 + j * ROWS) * p.dx_sp);
    }
    float m[4], r[4], s1[4], s2[4];
    const float inv = 1.f / (float)p.HW;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m[e] = p.mean[(long long)n * C + c + e]; r[e] = p.rstd[(long long)n * C + c + e];
        s1[e] = (float)p.ws[((long long)n * C + c + e) * 2]; s2[e] = (float)p.ws[((long long)n * C + c + e) * 2 + 1];
    }
    const float4 g = ld4(p.gamma + c), bt = ld4(p.beta + c);
    // Every load has been requested: wait for all of them HERE, once.  The stores below sit in per-row branches; a load still pending there makes
    // the compiler wait with vmcnt(0) in every branch, and on gfx950 that also waits for the previous row's stores (vmcnt counts them).
    // 0x0F70 = vmcnt(0) alone in the gfx9 encoding of s_waitcnt, which gfx950 uses (the build compiles for gfx950 only).
    __builtin_amdgcn_s_waitcnt(0x0F70);
    if (blockIdx.x == 0 && prow == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { unsafeAtomicAdd(p.dbeta + c + e, s1[e]); unsafeAtomicAdd(p.dgamma + c + e, s2[e]); }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { s1[e] *= inv; s2[e] *= inv; }
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int px = px0 + j * ROWS;
        if (px >= p.HW) break;
        // dz and xhat as inorm_dz_batch: the views that cover the channels added in view order, times the activation's derivative
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f), xh;
#pragma unroll
        for (int k = 0; k < NDY; ++k)
            if (cov[k]) {
                float4 tk = t[k][j];
                // 0 + t of the first view: the compiler folds an add of a constant into the branch that loaded t, with a wait right behind
                // every load of that view.  The empty asm (after the wait above) hides where tk came from; it emits nothing.
                if (k == 0) asm volatile("" : "+v"(tk.x), "+v"(tk.y), "+v"(tk.z), "+v"(tk.w));
                d.x += tk.x; d.y += tk.y; d.z += tk.z; d.w += tk.w;
            }
        xh.x = (v[j].x - m[0]) * r[0]; xh.y = (v[j].y - m[1]) * r[1]; xh.z = (v[j].z - m[2]) * r[2]; xh.w = (v[j].w - m[3]) * r[3];
        d.x *= act_grad<ACT>((v[j].x - m[0]) * r[0] * g.x + bt.x, p.alpha);
        d.y *= act_grad<ACT>((v[j].y - m[1]) * r[1] * g.y + bt.y, p.alpha);
        d.z *= act_grad<ACT>((v[j].z - m[2]) * r[2] * g.z + bt.z, p.alpha);
        d.w *= act_grad<ACT>((v[j].w - m[3]) * r[3] * g.w + bt.w, p.alpha);
        float4 o;
        o.x = g.x * r[0] * fmaf(-xh.x, s2[0], d.x - s1[0]);
        o.y = g.y * r[1] * fmaf(-xh.y, s2[1], d.y - s1[1]);
        o.z = g.z * r[2] * fmaf(-xh.z, s2[2], d.z - s1[2]);
        o.w = g.w * r[3] * fmaf(-xh.w, s2[3], d.w - s1[3]);
        if (DXM == DX_F32_ACC) { o.x += old[j].x; o.y += old[j].y; o.z += old[j].z; o.w += old[j].w; }
        st4t<DXM == DX_BF16>(dxs, (long long)px * p.dx_sp, o);
    }
}

template <int C4, int ACT, int R, int NDY>
static int launch_ndy(hipStream_t st, const SavpInormArgs* a) {
    BwdP<NDY> p;
    p.x = (const float*)a->x.p; p.x_sn = a->x.sn; p.x_sp = a->x.sp;
    p.ws = (const double*)a->ws; p.gamma = a->gamma; p.beta = a->beta; p.mean = a->mean; p.rstd = a->rstd;
    p.dx = (float*)a->dx.p; p.dx_sn = a->dx.sn; p.dx_sp = a->dx.sp;
    p.dgamma = a->dgamma; p.dbeta = a->dbeta; p.HW = a->HW; p.alpha = a->alpha;
    for (int k = 0; k < NDY; ++k) {
        p.dy[k].p = (const float*)a->dy[k].p; p.dy[k].sn = a->dy[k].sn; p.dy[k].sp = a->dy[k].sp;
        p.dy[k].c0 = a->dy_c0[k]; p.dy[k].c1 = a->dy_nc[k] > 0 ? a->dy_c0[k] + a->dy_nc[k] : a->C;
    }
    constexpr int PX = R * (INORM_NT / C4);
    const dim3 grid((a->HW + PX - 1) / PX, a->N);
    if (a->dx_bf16) hipLaunchKernelGGL((inorm_bwd_apply_fast_kernel<C4, ACT, R, NDY, DX_BF16>), grid, dim3(INORM_NT), 0, st, p);
    else if (a->dx_beta) hipLaunchKernelGGL((inorm_bwd_apply_fast_kernel<C4, ACT, R, NDY, DX_F32_ACC>), grid, dim3(INORM_NT), 0, st, p);
    else hipLaunchKernelGGL((inorm_bwd_apply_fast_kernel<C4, ACT, R, NDY, DX_F32>), grid, dim3(INORM_NT), 0, st, p);
    return 1;
}

template <int C4, int ACT, int R>
static int launch_r(hipStream_t st, const SavpInormArgs* a) {
    switch (a->ndy) {
        case 1: return launch_ndy<C4, ACT, R, 1>(st, a);
        case 2: return launch_ndy<C4, ACT, R, 2>(st, a);
        case 3: return launch_ndy<C4, ACT, R, 3>(st, a);
    }
    return 0;
}

// at most 4 rows: a row is up to five 16-byte loads here (x, three views, the old dx), and 8 rows of them would halve the occupancy
template <int C4, int ACT>
static int launch_act(hipStream_t st, const SavpInormArgs* a, int chunk) {
    switch (rows_per_thread(chunk, INORM_NT / C4, 4)) {
        case 1: return launch_r<C4, ACT, 1>(st, a);
        case 2: return launch_r<C4, ACT, 2>(st, a);
        case 4: if constexpr (C4 >= 4) return launch_r<C4, ACT, 4>(st, a); else return 0;      // C = 8: a chunk is at most 2 rows per thread
    }
    return 0;
}

template <int C4>
static int launch_c4(hipStream_t st, const SavpInormArgs* a, int chunk) {
    switch (a->act) {
        case 0: return launch_act<C4, 0>(st, a, chunk);
        case 1: return launch_act<C4, 1>(st, a, chunk);
        case 2: return launch_act<C4, 2>(st, a, chunk);
    }
    return 0;                                       // ELU: the generic kernel
}

}  // namespace inorm_stream

int inorm_fast_bwd(hipStream_t st, const SavpInormArgs* a, int chunk) {
    using namespace inorm_stream;
    if (a->ndy > 3) return 0;
    switch (a->C) {
        case 8: return launch_c4<2>(st, a, chunk);
        case 32: return launch_c4<8>(st, a, chunk);
        case 64: return launch_c4<16>(st, a, chunk);
        case 128: return launch_c4<32>(st, a, chunk);
        case 256: return launch_c4<64>(st, a, chunk);
    }
    return 0;
}

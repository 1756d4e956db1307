// pix_distribs.hip -- the designated-pixel distributions of SAVPCell (inputs['pix_distribs'], savp_model.py:408-410,598-621,648-653)
// and the dataset's splat that produces them (tf_utils.pixel_distribution, tf_utils.py:562-585).
//
//   pix_distribs_fwd   : the whole recurrence over the T1 steps of an unroll that has already run, ONE launch.  The distributions never
//                        feed back into the image path and no loss reads them, so the pass only needs what the unroll keeps per step (the
//                        CDNA / DNA kernels or flows, the mask logits) and couples steps only within one (sample, designated pixel) map:
//                        one workgroup per map loops over time.  The last_frames source maps and the step's new map stay in LDS where they
//                        fit (64 x 64 with last_frames = 4: 80 KB; 128 x 128 with one source: 128 KB); otherwise the sources are read from
//                        the pix_in / gen rows in global memory and a workgroup barrier separates a step's stores from the next step's loads.
//                        The per-step normalisation is a fixed-order reduction inside the workgroup: no atomics, two runs give the same bits.
//   pixel_distribution : bilinear one-hot splat of (y, x) positions on the FLAT index y * W + x, in gather form (every output element is
//                        written by its own thread).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "savp_hip.h"

#define PD_NT 1024
#define PD_NW (PD_NT / 64)
#define PD_MAXK 256                                  // CDNA: taps x kernels of one sample, staged per step
#define PD_HDR (32 + SAVP_PIX_MAX_SLOTS + PD_MAXK + 16)   // floats in front of the maps: partial sums, slot table, CDNA kernels, source table
#define PD_LDS_MAX (160 * 1024)
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

static_assert(PD_HDR % 4 == 0, "the maps start on a 16-byte boundary");

// tf.pad SYMMETRIC index (clamped: a pad wider than the map must not leave it)
__device__ __forceinline__ int pd_sym(int q, int n) {
    const int s = q < 0 ? -q - 1 : (q >= n ? 2 * n - 1 - q : q);
    return min(max(s, 0), n - 1);
}
__device__ __forceinline__ int pd_clamp(int v, int hi) { return min(max(v, 0), hi); }

// one source map: an LDS slot (unit stride) or a strided row in global memory (null: zeros)
template <bool LDSM>
struct PdSrc {
    const float* p;
    long long sp;
    __device__ __forceinline__ float at(int idx) const {
        if (LDSM) return p[idx];
        return p ? p[(long long)idx * sp] : 0.f;
    }
};

// LDSM: the sources and the new map live in LDS; otherwise the sources are rows of pix_in / gen in global memory.  KS = 5: a 5 x 5 kernel
// window, unrolled; 0: any window (and the flows)
template <bool LDSM, int KS>
__global__ __launch_bounds__(PD_NT) void pix_distribs_kernel(SavpPixDistribArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* red = smem;                                                    // [PD_NW] per-wave partial sums
    int* tab = reinterpret_cast<int*>(smem + 32);                         // [M] slot kind | arg << 8
    float* kb = smem + 32 + SAVP_PIX_MAX_SLOTS;                           // [taps * nk] this step's CDNA kernels
    const float** sptr = reinterpret_cast<const float**>(smem + 32 + SAVP_PIX_MAX_SLOTS + PD_MAXK);      // [L] global sources (null: zeros)
    long long* ssp = reinterpret_cast<long long*>(smem + 32 + SAVP_PIX_MAX_SLOTS + PD_MAXK + 8);         // [L] their pixel strides
    float* maps = smem + PD_HDR;                                          // LDSM: [L + 1][HW]

    const int tid = threadIdx.x;
    const int n = blockIdx.x / a.P, pp = blockIdx.x % a.P;
    const int H = a.H, W = a.W, HW = H * W, L = a.nsrc, K = a.K, nk = L * K, M = a.M;
    const int taps = a.kh * a.kw, pt = (a.kh - 1) / 2, pl = (a.kw - 1) / 2;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < SAVP_PIX_MAX_SLOTS; ++i) tab[i] = a.slot_kind[i] | (a.slot_arg[i] << 8);
    }
    const float* pin = a.pix_in + (long long)n * a.pi_sn + pp;
    float* gen = a.gen + (long long)n * a.g_sn + pp;
    float* newm = maps + (LDSM ? L * HW : 0);
    if (LDSM) {                                      // last_pix_distribs = [pix_distribs[0]] * last_frames (savp_model.py:288-290,350-351)
        for (int px = tid; px < HW; px += PD_NT) {
            const float v = pin[(long long)px * a.pi_sp];
            for (int j = 0; j < L; ++j) maps[j * HW + px] = v;
        }
    }
    for (int t = 0; t < a.T1; ++t) {
        // pix_distrib = where(ground_truth[t], inputs['pix_distribs'], states['gen_pix_distrib']) (:408-409; the state starts as zeros);
        // last_pix_distribs = last_pix_distribs[1:] + [pix_distrib] (:410): source j of this step is ring slot (t + 1 + j) % L
        if (LDSM) {
            const bool gt = a.gt_mask[(long long)t * a.N + n] != 0;
            float* cur = maps + (t % L) * HW;
            const float* g = pin + (long long)t * a.pi_st;
            for (int px = tid; px < HW; px += PD_NT) cur[px] = gt ? g[(long long)px * a.pi_sp] : (t > 0 ? newm[px] : 0.f);
        } else if (tid < L) {
            const int s = max(t - L + 1 + tid, 0);
            const bool gt = a.gt_mask[(long long)s * a.N + n] != 0;
            sptr[tid] = gt ? pin + (long long)s * a.pi_st : (s > 0 ? gen + (long long)(s - 1) * a.g_st : nullptr);
            ssp[tid] = gt ? a.pi_sp : a.g_sp;
        }
        const float* tfb = a.tfp + (long long)t * a.tf_st + (long long)n * a.tf_sn;
        if (a.tf == SAVP_PIX_TF_CDNA)
            for (int i = tid; i < taps * nk; i += PD_NT) kb[i] = tfb[i];
        __syncthreads();

        // source j of this step, oldest first: an LDS ring slot, or a row of pix_in / gen in global memory (null: the zero state)
        auto src = [&](int j) -> PdSrc<LDSM> {
            if (LDSM) return PdSrc<LDSM>{maps + ((t + 1 + j) % L) * HW, 1};
            return PdSrc<LDSM>{sptr[j], ssp[j]};
        };
        const PdSrc<LDSM> scur = src(L - 1);
        const float* lg = a.logits + (long long)t * a.lg_st + (long long)n * a.lg_sn;
        const float* pin_lc = pin + (long long)min(t, a.context_frames - 1) * a.pi_st;
        float* trb = a.transformed ? a.transformed + ((((long long)t * a.N + n) * HW) * a.P + pp) * M : nullptr;
        float* gnow = gen + (long long)t * a.g_st;
        float part = 0.f;
        for (int px = tid; px < HW; px += PD_NT) {
            const int y = px / W, x = px % W;
            const float* l = lg + (long long)px * a.lg_sp;
            float mx = 0.f, den = 1.f;
            if (!a.masks_given) {                    // masks = softmax(logits) (:634), recomputed in fp32
                mx = l[0];
                for (int m = 1; m < M; ++m) mx = fmaxf(mx, l[m]);
                den = 0.f;
                for (int m = 0; m < M; ++m) den += expf(l[m] - mx);
            }
            auto wgt = [&](int m) -> float { return a.masks_given ? l[m] : expf(l[m] - mx) / den; };
            float* tro = trb ? trb + (long long)px * a.P * M : nullptr;
            float acc = 0.f;
            // slots 0 .. nk-1: the transformed maps, group j of the kernels / flows applied to source j (apply_kernels / apply_flows, :926-965)
            if (a.tf == SAVP_PIX_TF_FLOW) {          // flow_ops.image_warp: backward bilinear warp with clamped gathers
                const float* f = tfb + (long long)px * a.tf_sp;
                for (int m = 0; m < nk; ++m) {
                    const PdSrc<LDSM> s = src(m / K);
                    const float fx = f[m], fy = f[nk + m];
                    const float ffx = floorf(fx), ffy = floorf(fy);
                    const float xw = fx - ffx, yw = fy - ffy;
                    const int ix = (int)fminf(fmaxf(ffx, -65536.f), 65536.f), iy = (int)fminf(fmaxf(ffy, -65536.f), 65536.f);
                    const int x0 = pd_clamp(x + ix, W - 1), x1 = pd_clamp(x + ix + 1, W - 1);
                    const int y0 = pd_clamp(y + iy, H - 1), y1 = pd_clamp(y + iy + 1, H - 1);
                    const float v = (1.f - xw) * (1.f - yw) * s.at(y0 * W + x0) + (1.f - xw) * yw * s.at(y1 * W + x0) +
                                    xw * (1.f - yw) * s.at(y0 * W + x1) + xw * yw * s.at(y1 * W + x1);
                    if (tro) tro[m] = v;
                    acc += v * wgt(m);
                }
            } else {                                 // normalised kernels on the SYMMETRIC-padded map (:858-923)
                // every source value is read once per tap for up to four kernels of its group; KS = 5: the 5 x 5 window's mirrored row
                // offsets and columns once per pixel, taps unrolled
                int ry[KS ? KS : 1], cx[KS ? KS : 1];
                if (KS) {
#pragma unroll
                    for (int u = 0; u < KS; ++u) { ry[u] = pd_sym(y + u - pt, H) * W; cx[u] = pd_sym(x + u - pl, W); }
                }
                const float* kpx = a.tf == SAVP_PIX_TF_CDNA ? kb : tfb + (long long)px * a.tf_sp;
                for (int j = 0; j < L; ++j) {
                    const PdSrc<LDSM> s = src(j);
                    for (int k0 = 0; k0 < K; k0 += 4) {
                        const int nv = min(4, K - k0);
                        const float* kp = kpx + j * K + k0;
                        float v[4] = {0.f, 0.f, 0.f, 0.f};
                        if (KS) {
#pragma unroll
                            for (int u = 0; u < KS; ++u)
#pragma unroll
                                for (int w = 0; w < KS; ++w) {
                                    const float sv = s.at(ry[u] + cx[w]);
                                    const float* kq = kp + (u * KS + w) * nk;
#pragma unroll
                                    for (int i = 0; i < 4; ++i)
                                        if (i < nv) v[i] += sv * kq[i];
                                }
                        } else {
                            for (int u = 0; u < a.kh; ++u) {
                                const int row = pd_sym(y + u - pt, H) * W;
                                for (int w = 0; w < a.kw; ++w) {
                                    const float sv = s.at(row + pd_sym(x + w - pl, W));
                                    const float* kq = kp + (u * a.kw + w) * nk;
#pragma unroll
                                    for (int i = 0; i < 4; ++i)
                                        if (i < nv) v[i] += sv * kq[i];
                                }
                            }
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (i < nv) {
                                const int m = j * K + k0 + i;
                                if (tro) tro[m] = v[i];
                                acc += v[i] * wgt(m);
                            }
                    }
                }
            }
            // the slots behind them, from the table: the step's own map, frames of the input
            const float curv = scur.at(px);
            for (int m = nk; m < M; ++m) {
                const int kind = tab[m] & 255, arg = tab[m] >> 8;
                float v;
                if (kind == SAVP_PIX_SLOT_CURRENT) v = curv;
                else if (kind == SAVP_PIX_SLOT_FIXED) v = pin[(long long)arg * a.pi_st + (long long)px * a.pi_sp];
                else v = pin_lc[(long long)px * a.pi_sp];
                if (tro) tro[m] = v;
                acc += v * wgt(m);
            }
            part += acc;
            if (LDSM) newm[px] = acc; else gnow[(long long)px * a.g_sp] = acc;
        }
        // gen_pix_distrib /= reduce_sum(gen_pix_distrib, axis=(1, 2)) (:653): thread partials in pixel order, a shuffle tree per wave,
        // the waves' sums in wave order -- the same tree in every run
        for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
        if ((tid & 63) == 0) red[tid >> 6] = part;
        __syncthreads();
        float tot = 0.f;
        for (int w = 0; w < PD_NW; ++w) tot += red[w];
        for (int px = tid; px < HW; px += PD_NT) {
            const float v = (LDSM ? newm[px] : gnow[(long long)px * a.g_sp]) / tot;
            gnow[(long long)px * a.g_sp] = v;
            if (LDSM) newm[px] = v;
        }
        __threadfence_block();                       // (global sources) this step's stores are the next step's loads, workgroup scope
        __syncthreads();
    }
}

static long long pd_lds_bytes(const SavpPixDistribArgs* a) { return (long long)sizeof(float) * (PD_HDR + ((long long)a->nsrc + 1) * a->H * a->W); }

extern "C" int savp_pix_distribs_lds_resident(const SavpPixDistribArgs* a) {
    if (!a || a->H < 1 || a->W < 1 || a->nsrc < 1) return 0;
    return (!a->force_global && pd_lds_bytes(a) <= PD_LDS_MAX) ? 1 : 0;
}

extern "C" int savp_pix_distribs_fwd(void* stream, const SavpPixDistribArgs* a) {
    if (!a || !a->pix_in || !a->gt_mask || !a->tfp || !a->logits || !a->gen) return SAVP_EINVAL;
    if (a->T1 < 1 || a->N < 1 || a->H < 1 || a->W < 1 || a->P < 1 || a->T_in < a->T1) return SAVP_EINVAL;
    if ((long long)a->H * a->W > (1 << 24) || (long long)a->N * a->P > 0x7fffffffLL) return SAVP_EINVAL;
    if (a->nsrc < 1 || a->nsrc > SAVP_MAX_SOURCES || a->K < 1 || a->M < 1 || a->M > SAVP_PIX_MAX_SLOTS) return SAVP_EINVAL;
    if (a->tf != SAVP_PIX_TF_CDNA && a->tf != SAVP_PIX_TF_DNA && a->tf != SAVP_PIX_TF_FLOW) return SAVP_EINVAL;
    const int nk = a->nsrc * a->K;
    if (a->tf != SAVP_PIX_TF_FLOW && (a->kh < 1 || a->kw < 1 || a->kh > 64 || a->kw > 64)) return SAVP_EINVAL;
    if (a->tf == SAVP_PIX_TF_CDNA && a->kh * a->kw * nk > PD_MAXK) return SAVP_EINVAL;
    if (a->tf != SAVP_PIX_TF_FLOW) {                 // tf.pad SYMMETRIC takes a pad of at most the map's size (pd_sym mirrors once)
        const int pt = (a->kh - 1) / 2, pl = (a->kw - 1) / 2;
        if (max(pt, a->kh - 1 - pt) > a->H || max(pl, a->kw - 1 - pl) > a->W) return SAVP_EINVAL;
    }
    if (a->M < nk) return SAVP_EINVAL;
    for (int m = 0; m < a->M; ++m) {
        const int kind = a->slot_kind[m], arg = a->slot_arg[m];
        if ((m < nk) != (kind == SAVP_PIX_SLOT_TRANSFORMED)) return SAVP_EINVAL;      // the transformed maps come first, in kernel order
        if (kind == SAVP_PIX_SLOT_TRANSFORMED) { if (arg != m) return SAVP_EINVAL; }
        else if (kind == SAVP_PIX_SLOT_FIXED) { if (arg < 0 || arg >= a->T_in) return SAVP_EINVAL; }
        else if (kind == SAVP_PIX_SLOT_LAST_CONTEXT) { if (a->context_frames < 1) return SAVP_EINVAL; }
        else if (kind != SAVP_PIX_SLOT_CURRENT) return SAVP_EINVAL;
    }
    SavpPixDistribArgs p = *a;
    if (p.tf == SAVP_PIX_TF_FLOW) { p.kh = p.kw = 1; }
    for (int m = p.M; m < SAVP_PIX_MAX_SLOTS; ++m) p.slot_kind[m] = p.slot_arg[m] = 0;
    const dim3 grid((unsigned)(a->N * a->P)), block(PD_NT);
    hipStream_t st = (hipStream_t)stream;
    const bool k5 = p.tf != SAVP_PIX_TF_FLOW && p.kh == 5 && p.kw == 5;
    if (savp_pix_distribs_lds_resident(a)) {
        static bool attr = false;
        if (!attr) {
            if (hipFuncSetAttribute((const void*)pix_distribs_kernel<true, 5>, hipFuncAttributeMaxDynamicSharedMemorySize, PD_LDS_MAX) != hipSuccess ||
                hipFuncSetAttribute((const void*)pix_distribs_kernel<true, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, PD_LDS_MAX) != hipSuccess)
                return SAVP_ELAUNCH;
            attr = true;
        }
        if (k5) hipLaunchKernelGGL((pix_distribs_kernel<true, 5>), grid, block, (size_t)pd_lds_bytes(a), st, p);
        else hipLaunchKernelGGL((pix_distribs_kernel<true, 0>), grid, block, (size_t)pd_lds_bytes(a), st, p);
    } else {
        // (the unrolled window with 64-bit global addresses would not fit the 128 registers of a 1024-thread workgroup)
        hipLaunchKernelGGL((pix_distribs_kernel<false, 0>), grid, block, sizeof(float) * PD_HDR, st, p);
    }
    return LAUNCH_OK();
}

// ---------------------------------------------------------------------------------------------------------------
// tf_utils.pixel_distribution
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pixel_distribution_kernel(const float* __restrict__ pos, long long rows, int P, int H, int W,
                                                                 float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long HW = (long long)H * W;
    if (i >= rows * HW * P) return;
    const int p = (int)(i % P);
    const long long px = (i / P) % HW, r = i / (P * HW);
    const float y = pos[(r * P + p) * 2], x = pos[(r * P + p) * 2 + 1];
    const float lim = 1073741824.f;                  // positions that far out touch no pixel; keeps the int casts defined
    const int x0 = (int)fminf(fmaxf(floorf(x), -lim), lim), y0 = (int)fminf(fmaxf(floorf(y), -lim), lim);
    const float x0f = (float)x0, x1f = (float)(x0 + 1), y0f = (float)y0, y1f = (float)(y0 + 1);
    // one_hot(y * W + x, H * W): the FLAT index decides (x1 == W lands at the start of the next row), indices outside [0, HW) give zeros
    const long long ia = (long long)y0 * W + x0, ib = ia + W, ic = ia + 1, id = ia + W + 1;
    const float wa = (x1f - x) * (y1f - y), wb = (x1f - x) * (y - y0f), wc = (x - x0f) * (y1f - y), wd = (x - x0f) * (y - y0f);
    out[i] = wa * (ia == px ? 1.f : 0.f) + wb * (ib == px ? 1.f : 0.f) + wc * (ic == px ? 1.f : 0.f) + wd * (id == px ? 1.f : 0.f);
}

extern "C" int savp_pixel_distribution(void* stream, const float* pos, int64_t rows, int32_t P, int32_t H, int32_t W, float* out) {
    if (!pos || !out || rows < 1 || P < 1 || H < 1 || W < 1) return SAVP_EINVAL;
    const long long total = (long long)rows * H * W * P;
    if (total > 0x7fffffffLL * 256) return SAVP_EINVAL;
    hipLaunchKernelGGL(pixel_distribution_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pos, (long long)rows, P, H,
                       W, out);
    return LAUNCH_OK();
}

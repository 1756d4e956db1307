// warp_dna.hip -- the two alternative pixel transformations of SAVPCell (hparams.transformation):
//   image_warp fwd/bwd : flow_ops.image_warp (flow_ops.py:4-79) + apply_flows (savp_model.py:955-965): backward
//                        bilinear warp with clamped gathers; gradient w.r.t. the flow (through the bilinear weights,
//                        floor() has zero gradient) and w.r.t. the image (scatter-add of the 4 corner weights).
//   dna_apply fwd/bwd  : per-pixel 5x5 kernels (savp_model.py:541-544,556-559,858-890): identity added, relu-shift,
//                        normalised over the taps, applied to the SYMMETRIC-padded image.  The reference goes through
//                        extract_image_patches + batched matmul; here one thread per pixel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"
#include "zero_fill.h"

#define NT 256
#define RELU_SHIFT 1e-12f
#define MAXC 4
#define MAXS SAVP_MAX_SOURCES
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

// one source image of a multi-source launch (last_frames > 1): its image view and where its image gradient goes
struct SrcP {
    const float* img; long long i_sn, i_sp;
    float* dimg; long long di_sn, di_sp; int dimg_beta;
};

// Bind source blockIdx.z of a multi-source launch into the fields p.img / p.dimg / p.koff: static indices only (a runtime index into
// the kernel's argument struct would spill it to scratch); blockIdx.z == 0 leaves a single-source launch as it was.
template <class P>
__device__ __forceinline__ void bind_src(P& p) {
    const int j = blockIdx.z;
#pragma unroll
    for (int i = 1; i < MAXS; ++i)
        if (i == j) {
            p.img = p.src[i].img; p.i_sn = p.src[i].i_sn; p.i_sp = p.src[i].i_sp;
            p.dimg = p.src[i].dimg; p.di_sn = p.src[i].di_sn; p.di_sp = p.src[i].di_sp; p.dimg_beta = p.src[i].dimg_beta;
        }
    p.koff = j * p.K;
}

struct WarpP {
    int N, H, W, C, K;                         // K: flows per source
    int ks, koff;                              // flows per component in flows / dflows (nsrc*K) and the bound source's first one
    const float* img; long long i_sn, i_sp;
    const float* flows;                        // [N,H,W,2ks] contiguous, channel comp*ks + koff + k (comp 0 = x, 1 = y)
    float* out; long long o_sn, o_sp;          // [N,H,W,ks*C] channel (koff+k)*C + c
    const float* dout; long long do_sn, do_sp;
    float* dflows;                             // [N,H,W,2ks]
    float* dimg; long long di_sn, di_sp;       // pre-zeroed (atomics); may be null
    int dimg_beta;                             // 0: zero_src_views_kernel clears the view first (the warp itself always adds)
    int nsrc; SrcP src[MAXS];
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool BWD>
__global__ void image_warp_kernel(WarpP p) {
    bind_src(p);
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const long long total = (long long)p.N * p.H * p.W * p.K;
    if (i >= total) return;
    const int k = (int)(i % p.K);
    long long r = i / p.K;
    const int px = (int)(r % (p.H * p.W));
    const int n = (int)(r / (p.H * p.W));
    const int y = px / p.W, x = px % p.W;
    const float* fl = p.flows + ((long long)n * p.H * p.W + px) * 2 * p.ks + p.koff;
    const float fx = fl[k], fy = fl[p.ks + k];
    const float ffx = floorf(fx), ffy = floorf(fy);
    const float xw = fx - ffx, yw = fy - ffy;
    const int x0 = clampi(x + (int)ffx, 0, p.W - 1), x1 = clampi(x + (int)ffx + 1, 0, p.W - 1);
    const int y0 = clampi(y + (int)ffy, 0, p.H - 1), y1 = clampi(y + (int)ffy + 1, 0, p.H - 1);
    const float* im = p.img + (long long)n * p.i_sn;
    const float* Ia = im + (long long)(y0 * p.W + x0) * p.i_sp;      // top left
    const float* Ib = im + (long long)(y1 * p.W + x0) * p.i_sp;      // bottom left
    const float* Ic = im + (long long)(y0 * p.W + x1) * p.i_sp;      // top right
    const float* Id = im + (long long)(y1 * p.W + x1) * p.i_sp;      // bottom right
    const float wa = (1.f - xw) * (1.f - yw), wb = (1.f - xw) * yw, wc = xw * (1.f - yw), wd = xw * yw;
    if (!BWD) {
        float* o = p.out + (long long)n * p.o_sn + (long long)px * p.o_sp + (p.koff + k) * p.C;
        for (int c = 0; c < p.C; ++c) o[c] = wa * Ia[c] + wb * Ib[c] + wc * Ic[c] + wd * Id[c];
    } else {
        const float* d = p.dout + (long long)n * p.do_sn + (long long)px * p.do_sp + (p.koff + k) * p.C;
        float gx = 0.f, gy = 0.f;
        for (int c = 0; c < p.C; ++c) {
            const float a = Ia[c], b = Ib[c], cc = Ic[c], dd = Id[c], g = d[c];
            gx += g * (-(1.f - yw) * a - yw * b + (1.f - yw) * cc + yw * dd);
            gy += g * (-(1.f - xw) * a + (1.f - xw) * b - xw * cc + xw * dd);
            if (p.dimg) {
                float* di = p.dimg + (long long)n * p.di_sn;
                unsafeAtomicAdd(di + (long long)(y0 * p.W + x0) * p.di_sp + c, wa * g);
                unsafeAtomicAdd(di + (long long)(y1 * p.W + x0) * p.di_sp + c, wb * g);
                unsafeAtomicAdd(di + (long long)(y0 * p.W + x1) * p.di_sp + c, wc * g);
                unsafeAtomicAdd(di + (long long)(y1 * p.W + x1) * p.di_sp + c, wd * g);
            }
        }
        float* df = p.dflows + ((long long)n * p.H * p.W + px) * 2 * p.ks + p.koff;
        df[k] = gx; df[p.ks + k] = gy;
    }
}

static int fill_warp(WarpP& p, const SavpWarpArgs* a) {
    if (!a || a->C < 1 || a->K < 1 || !a->img.p || !a->flows) return SAVP_EINVAL;
    p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C; p.K = a->K;
    p.ks = a->K; p.koff = 0;
    p.img = (const float*)a->img.p; p.i_sn = a->img.sn; p.i_sp = a->img.sp;
    p.flows = a->flows;
    p.out = (float*)a->out.p; p.o_sn = a->out.sn; p.o_sp = a->out.sp;
    p.dout = (const float*)a->dout.p; p.do_sn = a->dout.sn; p.do_sp = a->dout.sp;
    p.dflows = a->dflows; p.dimg = a->dimg;
    p.di_sp = a->C; p.di_sn = (long long)a->H * a->W * a->C;        // contiguous [N,H,W,C]
    p.dimg_beta = 0;
    p.nsrc = 1;
    p.src[0] = SrcP{p.img, p.i_sn, p.i_sp, p.dimg, p.di_sn, p.di_sp, 0};
    return SAVP_OK;
}

// the per-source fields of a multi-source call (nsrc <= MAXS, every live source with an image); p.img / p.dimg start as source 0
template <class P, class A>
static int fill_sources(P& p, const A* a) {
    if (a->nsrc < 1 || a->nsrc > MAXS) return SAVP_EINVAL;
    p.nsrc = a->nsrc;
    for (int j = 0; j < MAXS; ++j) {
        const bool live = j < a->nsrc;
        if (live && !a->img[j].p) return SAVP_EINVAL;
        p.src[j] = live ? SrcP{(const float*)a->img[j].p, a->img[j].sn, a->img[j].sp, (float*)a->dimg[j].p, a->dimg[j].sn, a->dimg[j].sp,
                               a->dimg_beta[j]}
                        : SrcP{nullptr, 0, 0, nullptr, 0, 0, 0};
    }
    p.img = p.src[0].img; p.i_sn = p.src[0].i_sn; p.i_sp = p.src[0].i_sp;
    p.dimg = p.src[0].dimg; p.di_sn = p.src[0].di_sn; p.di_sp = p.src[0].di_sp; p.dimg_beta = p.src[0].dimg_beta;
    p.koff = 0;
    return SAVP_OK;
}

static int fill_warp_multi(WarpP& p, const SavpWarpMultiArgs* a) {
    if (!a || a->C < 1 || a->C > MAXC || a->K < 1 || !a->flows) return SAVP_EINVAL;
    p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C; p.K = a->K;
    p.ks = a->nsrc * a->K;
    p.flows = a->flows;
    p.out = (float*)a->out.p; p.o_sn = a->out.sn; p.o_sp = a->out.sp;
    p.dout = (const float*)a->dout.p; p.do_sn = a->dout.sn; p.do_sp = a->dout.sp;
    p.dflows = a->dflows;
    return fill_sources(p, a);
}

// the image-gradient views of the sources whose dimg_beta is 0 are cleared before the warp's atomics add into them
__global__ void zero_src_views_kernel(WarpP p) {
    bind_src(p);
    if (!p.dimg || p.dimg_beta) return;
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)p.N * p.H * p.W) return;
    const int n = (int)(i / (p.H * p.W)), px = (int)(i % (p.H * p.W));
    float* di = p.dimg + (long long)n * p.di_sn + (long long)px * p.di_sp;
    for (int c = 0; c < p.C; ++c) di[c] = 0.f;
}

extern "C" int savp_image_warp_fwd(void* stream, const SavpWarpArgs* a) {
    WarpP p;
    int rc = fill_warp(p, a);
    if (rc || !p.out) return SAVP_EINVAL;
    long long total = (long long)a->N * a->H * a->W * a->K;
    hipLaunchKernelGGL((image_warp_kernel<false>), dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, p);
    return LAUNCH_OK();
}

extern "C" int savp_image_warp_multi_fwd(void* stream, const SavpWarpMultiArgs* a) {
    WarpP p;
    int rc = fill_warp_multi(p, a);
    if (rc || !p.out) return rc ? rc : SAVP_EINVAL;
    long long total = (long long)a->N * a->H * a->W * a->K;
    hipLaunchKernelGGL((image_warp_kernel<false>), dim3((unsigned)((total + NT - 1) / NT), 1, p.nsrc), dim3(NT), 0, (hipStream_t)stream, p);
    return LAUNCH_OK();
}

extern "C" int savp_image_warp_multi_bwd(void* stream, const SavpWarpMultiArgs* a) {
    WarpP p;
    int rc = fill_warp_multi(p, a);
    if (rc || !p.dout || !p.dflows) return rc ? rc : SAVP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    bool clear = false;
    for (int j = 0; j < p.nsrc; ++j) clear |= p.src[j].dimg && !p.src[j].dimg_beta;
    if (clear) {
        long long px = (long long)a->N * a->H * a->W;
        hipLaunchKernelGGL(zero_src_views_kernel, dim3((unsigned)((px + NT - 1) / NT), 1, p.nsrc), dim3(NT), 0, st, p);
    }
    long long total = (long long)a->N * a->H * a->W * a->K;
    hipLaunchKernelGGL((image_warp_kernel<true>), dim3((unsigned)((total + NT - 1) / NT), 1, p.nsrc), dim3(NT), 0, st, p);
    return LAUNCH_OK();
}

extern "C" int savp_image_warp_bwd(void* stream, const SavpWarpArgs* a) {
    WarpP p;
    int rc = fill_warp(p, a);
    if (rc || !p.dout || !p.dflows) return SAVP_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (p.dimg) savp_zero_async(p.dimg, (size_t)a->N * a->H * a->W * a->C * sizeof(float), st);
    long long total = (long long)a->N * a->H * a->W * a->K;
    hipLaunchKernelGGL((image_warp_kernel<true>), dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, p);
    return LAUNCH_OK();
}

// ---------------------------------------------------------------------------------------------------------------
// DNA
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int symi(int q, int n) { return q < 0 ? -q - 1 : (q >= n ? 2 * n - 1 - q : q); }
__device__ __forceinline__ float ident5(int u, int v, int kh, int kw) {
    float fu, fv;
    if (kh & 1) fu = (u == kh / 2) ? 1.f : 0.f; else fu = (u == kh / 2 - 1 || u == kh / 2) ? 0.5f : 0.f;
    if (kw & 1) fv = (v == kw / 2) ? 1.f : 0.f; else fv = (v == kw / 2 - 1 || v == kw / 2) ? 0.5f : 0.f;
    return fu * fv;
}

struct DnaP {
    int N, H, W, C, K, kh, kw;                 // K: kernels per source
    int ks, koff;                              // kernels per tap in raw / kern / draw (nsrc*K) and the bound source's first one
    const float* img; long long i_sn, i_sp;
    const float* raw;                          // [N,HW,taps*ks] channel t*ks + koff + k (conv output)
    float* kern;                               // [N,HW,taps*ks] normalised kernels (saved by fwd, read by bwd)
    float* out; long long o_sn, o_sp;          // channel (koff+k)*C + c
    const float* dout; long long do_sn, do_sp;
    float* draw;                               // [N,HW,taps*ks]
    float* dimg; long long di_sn, di_sp; int dimg_beta;
    int nsrc; SrcP src[MAXS];
};

__global__ void dna_fwd_kernel(DnaP p) {
    bind_src(p);
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)p.N * p.H * p.W) return;
    const int n = (int)(i / (p.H * p.W)), px = (int)(i % (p.H * p.W));
    const int y = px / p.W, x = px % p.W;
    const int taps = p.kh * p.kw, pt = (p.kh - 1) / 2, pl = (p.kw - 1) / 2;
    const float* r = p.raw + i * taps * p.ks + p.koff;
    float* kn = p.kern + i * taps * p.ks + p.koff;
    const float* im = p.img + (long long)n * p.i_sn;
    float* o = p.out + (long long)n * p.o_sn + (long long)px * p.o_sp + p.koff * p.C;
    for (int k = 0; k < p.K; ++k) {
        float s = 0.f;
        for (int t = 0; t < taps; ++t) s += fmaxf(r[t * p.ks + k] + ident5(t / p.kw, t % p.kw, p.kh, p.kw) - RELU_SHIFT, 0.f) + RELU_SHIFT;
        const float inv = 1.f / s;
        float acc[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) acc[c] = 0.f;
        for (int t = 0; t < taps; ++t) {
            const float w = (fmaxf(r[t * p.ks + k] + ident5(t / p.kw, t % p.kw, p.kh, p.kw) - RELU_SHIFT, 0.f) + RELU_SHIFT) * inv;
            kn[t * p.ks + k] = w;
            const float* q = im + (long long)(symi(y + t / p.kw - pt, p.H) * p.W + symi(x + t % p.kw - pl, p.W)) * p.i_sp;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < p.C) acc[c] += q[c] * w;
        }
        for (int c = 0; c < p.C; ++c) o[k * p.C + c] = acc[c];
    }
}

// per-pixel kernel gradient + normalisation backward
__global__ void dna_bwd_kern_kernel(DnaP p) {
    bind_src(p);
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)p.N * p.H * p.W) return;
    const int n = (int)(i / (p.H * p.W)), px = (int)(i % (p.H * p.W));
    const int y = px / p.W, x = px % p.W;
    const int taps = p.kh * p.kw, pt = (p.kh - 1) / 2, pl = (p.kw - 1) / 2;
    const float* r = p.raw + i * taps * p.ks + p.koff;
    float* dr = p.draw + i * taps * p.ks + p.koff;
    const float* im = p.img + (long long)n * p.i_sn;
    const float* d = p.dout + (long long)n * p.do_sn + (long long)px * p.do_sp + p.koff * p.C;
    // draw = (dkern - sum(dkern * kern)) / s: where one tap holds nearly all of a small s (an even side spreads the identity over 2 or 4
    // taps of 0.5 / 0.25, within reach of the raw values), that tap's dkern and the dot cancel and 1 / s multiplies what is left.  The
    // sum, the dot and the difference are therefore taken in float64, with the kernel as v / s rather than its float32-rounded copy.
    for (int k = 0; k < p.K; ++k) {
        double s = 0.0;
        for (int t = 0; t < taps; ++t)
            s += (double)(fmaxf(r[t * p.ks + k] + ident5(t / p.kw, t % p.kw, p.kh, p.kw) - RELU_SHIFT, 0.f) + RELU_SHIFT);
        const double inv = 1.0 / s;
        double dot = 0.0;
        // first pass: dkern (stored temporarily in draw) and its dot with the normalised kernel
        for (int t = 0; t < taps; ++t) {
            const float* q = im + (long long)(symi(y + t / p.kw - pt, p.H) * p.W + symi(x + t % p.kw - pl, p.W)) * p.i_sp;
            float g = 0.f;
            for (int c = 0; c < p.C; ++c) g += q[c] * d[k * p.C + c];
            dr[t * p.ks + k] = g;
            const float v = fmaxf(r[t * p.ks + k] + ident5(t / p.kw, t % p.kw, p.kh, p.kw) - RELU_SHIFT, 0.f) + RELU_SHIFT;
            dot += (double)g * ((double)v * inv);
        }
        for (int t = 0; t < taps; ++t) {
            const float pre = r[t * p.ks + k] + ident5(t / p.kw, t % p.kw, p.kh, p.kw) - RELU_SHIFT;
            dr[t * p.ks + k] = pre > 0.f ? (float)(((double)dr[t * p.ks + k] - dot) * inv) : 0.f;
        }
    }
}

// image gradient in gather form (mirrored positions as in cdna_composite.hip)
__global__ void dna_bwd_img_kernel(DnaP p) {
    bind_src(p);
    if (!p.dimg) return;                       // (multi-source) this source's gradient is not wanted
    long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)p.N * p.H * p.W) return;
    const int n = (int)(i / (p.H * p.W)), px = (int)(i % (p.H * p.W));
    const int sy = px / p.W, sx = px % p.W;
    const int taps = p.kh * p.kw, pt = (p.kh - 1) / 2, pl = (p.kw - 1) / 2;
    const int pb = p.kh - 1 - pt, pr = p.kw - 1 - pl;
    int qy[3], nqy = 0, qx[3], nqx = 0;
    qy[nqy++] = sy;
    if (-sy - 1 >= -pt) qy[nqy++] = -sy - 1;
    if (2 * p.H - 1 - sy < p.H + pb && 2 * p.H - 1 - sy >= p.H) qy[nqy++] = 2 * p.H - 1 - sy;
    qx[nqx++] = sx;
    if (-sx - 1 >= -pl) qx[nqx++] = -sx - 1;
    if (2 * p.W - 1 - sx < p.W + pr && 2 * p.W - 1 - sx >= p.W) qx[nqx++] = 2 * p.W - 1 - sx;
    float acc[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.f;
    const float* dbase = p.dout + (long long)n * p.do_sn + p.koff * p.C;
    const float* kbase = p.kern + (long long)n * p.H * p.W * taps * p.ks + p.koff;
    for (int a = 0; a < nqy; ++a)
        for (int b = 0; b < nqx; ++b)
            for (int u = 0; u < p.kh; ++u) {
                const int y = qy[a] - u + pt;
                if (y < 0 || y >= p.H) continue;
                for (int v = 0; v < p.kw; ++v) {
                    const int x = qx[b] - v + pl;
                    if (x < 0 || x >= p.W) continue;
                    const long long op = (long long)y * p.W + x;
                    const float* d = dbase + op * p.do_sp;
                    const float* kk = kbase + op * taps * p.ks + (u * p.kw + v) * p.ks;
                    for (int k = 0; k < p.K; ++k) {
                        const float w = kk[k];
#pragma unroll
                        for (int c = 0; c < MAXC; ++c)
                            if (c < p.C) acc[c] += d[k * p.C + c] * w;
                    }
                }
            }
    float* di = p.dimg + (long long)n * p.di_sn + (long long)px * p.di_sp;
    for (int c = 0; c < p.C; ++c) di[c] = p.dimg_beta ? di[c] + acc[c] : acc[c];
}

// tf.pad SYMMETRIC takes a pad of at most the image's size (symi() mirrors once): the SAME pads before / after are (k-1)/2 and the rest
static bool dna_pad_fits(int kh, int kw, int H, int W) {
    if (kh < 1 || kw < 1) return false;
    const int pt = (kh - 1) / 2, pl = (kw - 1) / 2;
    return max(pt, kh - 1 - pt) <= H && max(pl, kw - 1 - pl) <= W;
}

static int fill_dna(DnaP& p, const SavpDnaArgs* a) {
    if (!a || a->C < 1 || a->C > MAXC || a->K < 1 || !a->img.p || !a->raw || !a->kern) return SAVP_EINVAL;
    if (!dna_pad_fits(a->kh, a->kw, a->H, a->W)) return SAVP_EINVAL;
    p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C; p.K = a->K; p.kh = a->kh; p.kw = a->kw;
    p.img = (const float*)a->img.p; p.i_sn = a->img.sn; p.i_sp = a->img.sp;
    p.raw = a->raw; p.kern = a->kern;
    p.out = (float*)a->out.p; p.o_sn = a->out.sn; p.o_sp = a->out.sp;
    p.dout = (const float*)a->dout.p; p.do_sn = a->dout.sn; p.do_sp = a->dout.sp;
    p.draw = a->draw;
    p.dimg = (float*)a->dimg.p; p.di_sn = a->dimg.sn; p.di_sp = a->dimg.sp; p.dimg_beta = a->dimg_beta;
    p.ks = a->K; p.koff = 0;
    p.nsrc = 1;
    p.src[0] = SrcP{p.img, p.i_sn, p.i_sp, p.dimg, p.di_sn, p.di_sp, p.dimg_beta};
    return SAVP_OK;
}

static int fill_dna_multi(DnaP& p, const SavpDnaMultiArgs* a) {
    if (!a || a->C < 1 || a->C > MAXC || a->K < 1 || !a->raw || !a->kern) return SAVP_EINVAL;
    if (!dna_pad_fits(a->kh, a->kw, a->H, a->W)) return SAVP_EINVAL;
    p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C; p.K = a->K; p.kh = a->kh; p.kw = a->kw;
    p.ks = a->nsrc * a->K;
    p.raw = a->raw; p.kern = a->kern;
    p.out = (float*)a->out.p; p.o_sn = a->out.sn; p.o_sp = a->out.sp;
    p.dout = (const float*)a->dout.p; p.do_sn = a->dout.sn; p.do_sp = a->dout.sp;
    p.draw = a->draw;
    return fill_sources(p, a);
}

extern "C" int savp_dna_apply_fwd(void* stream, const SavpDnaArgs* a) {
    DnaP p;
    int rc = fill_dna(p, a);
    if (rc || !p.out) return SAVP_EINVAL;
    long long total = (long long)a->N * a->H * a->W;
    hipLaunchKernelGGL(dna_fwd_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream, p);
    return LAUNCH_OK();
}

extern "C" int savp_dna_apply_bwd(void* stream, const SavpDnaArgs* a) {
    DnaP p;
    int rc = fill_dna(p, a);
    if (rc || !p.dout || !p.draw) return SAVP_EINVAL;
    long long total = (long long)a->N * a->H * a->W;
    dim3 grid((unsigned)((total + NT - 1) / NT));
    hipLaunchKernelGGL(dna_bwd_kern_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
    if (p.dimg) hipLaunchKernelGGL(dna_bwd_img_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
    return LAUNCH_OK();
}

extern "C" int savp_dna_apply_multi_fwd(void* stream, const SavpDnaMultiArgs* a) {
    DnaP p;
    int rc = fill_dna_multi(p, a);
    if (rc || !p.out) return rc ? rc : SAVP_EINVAL;
    long long total = (long long)a->N * a->H * a->W;
    hipLaunchKernelGGL(dna_fwd_kernel, dim3((unsigned)((total + NT - 1) / NT), 1, p.nsrc), dim3(NT), 0, (hipStream_t)stream, p);
    return LAUNCH_OK();
}

extern "C" int savp_dna_apply_multi_bwd(void* stream, const SavpDnaMultiArgs* a) {
    DnaP p;
    int rc = fill_dna_multi(p, a);
    if (rc || !p.dout || !p.draw) return rc ? rc : SAVP_EINVAL;
    long long total = (long long)a->N * a->H * a->W;
    dim3 grid((unsigned)((total + NT - 1) / NT), 1, p.nsrc);
    hipLaunchKernelGGL(dna_bwd_kern_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
    bool dimg = false;
    for (int j = 0; j < p.nsrc; ++j) dimg |= p.src[j].dimg != nullptr;
    if (dimg) hipLaunchKernelGGL(dna_bwd_img_kernel, grid, dim3(NT), 0, (hipStream_t)stream, p);
    return LAUNCH_OK();
}

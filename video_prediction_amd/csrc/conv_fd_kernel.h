// conv_fd_kernel.h -- the body of the implicit-GEMM FPROP / DGRAD kernel (conv_igemm.hip), written once for two argument blocks:
//   * ConvP: every geometry value is a kernel argument (conv_fd_kernel, any problem);
//   * FdFixedP<ID> (conv_fd_fixed.h): the geometry fields are static constexpr members with the same names, worked out at compile time
//     from one line of the fixed-problem table; only pointers, part / part_sz and the epilogue's scalars (beta, act, alpha, aux, bias) are
//     arguments (conv_fd_fixed_kernel<ID>).  `p.field` reads either.
// Tile, K-tile, K order, split-K partition, wave layout, LDS layout, MFMA sequence and the float epilogue are ONE text for both.  What the
// fixed block changes is the gather's integer arithmetic (FdIsFixed<P>): the per-row source offset is worked out once as a 32-bit element
// offset, a row's validity for a tap comes from a per-row tap mask built once instead of three range tests per row and K-tile, and the tap
// counters step by a compile-time recurrence.  Addresses, zero fill and operand values are the same as the generic path's.
#pragma once
#include "conv_common.h"

template <class P> struct FdIsFixed { static constexpr bool value = false; };

// GEMM: C[M = grid pixels][N = dst channels] = A[M][K=(taps,Cred)] * B[K][N]
// BF16 = true: operands are rounded to bf16 (RNE, v_cvt_pk_bf16_f32) while staging into LDS and multiplied on
// v_mfma_f32_32x32x16_bf16 (fp32 accumulate); K-tile 64.  BF16 = false: exact fp32 on v_mfma_f32_32x32x2_f32; K-tile 32.
// WB16 = true (bf16 mode only): the weight operand is read from a pre-packed bf16 copy (16-byte loads of 8 k values,
// no conversion, half the L2 traffic and staging instructions of the fp32 stream).
template <int WM, int WN, bool VEC, bool BF16, bool WB16, class P>
__device__ __forceinline__ void conv_fd_body(const P& p) {
    constexpr bool FX = FdIsFixed<P>::value && VEC;    // the scalar path keeps the generic gather (constants folded, nothing else)
    constexpr int BM = 64 * WM, BN = 64 * WN;
    constexpr int BKT = BF16 ? 64 : 32;                // K-tile
    constexpr int KV = BKT / 4;                        // float4 columns per row
    constexpr int RP = NTHREADS / KV;                  // rows covered per pass
    constexpr int RA = BM / RP, RB = BN / RP;          // float4 rows fetched per thread for A / B
    constexpr int ROWB = BF16 ? (BKT + 8) * 2 : BKP * 4;   // LDS row stride in bytes (padded: conflict-free b128 reads)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* As = reinterpret_cast<char*>(smem);          // [2][BM] rows
    char* Bs = As + 2 * BM * ROWB;                     // [2][BN] rows

    const bool dgrad = (p.mode == SAVP_CONV_DGRAD);
    // blockIdx.z = phase * splitk + split ; phase decode (DGRAD only) -> (fd, fh, fw)
    const int split = blockIdx.z % p.splitk;
    int fz = blockIdx.z / p.splitk;
    int fw = dgrad ? fz % p.sw : 0; fz = dgrad ? fz / p.sw : 0;
    int fh = dgrad ? fz % p.sh : 0; fz = dgrad ? fz / p.sh : 0;
    int fd = fz;
    const DimGeom gd = make_geom(dgrad, fd, p.D, p.Do, p.kd, p.sd, p.pd);
    const DimGeom gh = make_geom(dgrad, fh, p.H, p.Ho, p.kh, p.sh, p.ph);
    const DimGeom gw = make_geom(dgrad, fw, p.W, p.Wo, p.kw, p.sw, p.pw);

    const int Cred = dgrad ? p.Cy : p.Cx;             // reduction channels
    const int Nout = dgrad ? p.Cx : p.Cy;             // destination channels
    const int ntaps = gd.nt * gh.nt * gw.nt;
    const int K = ntaps * Cred;
    const int ldb = p.kd * p.kh * p.kw * Cred;        // packed weight row length
    const int Mtot = p.N * gd.Mdim * gh.Mdim * gw.Mdim;
    // logical tile id: n-tile major so that the tiles sharing a weight block are consecutive (-> same XCD L2)
    const int tlog = xcd_logical(blockIdx.x, p.tm * p.tn);
    const int m0 = (tlog % p.tm) * BM;
    const int n0 = (tlog / p.tm) * BN;
    if (m0 >= Mtot) return;                            // uniform per workgroup (phase with fewer pixels)

    const float* __restrict__ src = dgrad ? p.y : p.x;
    const long long s_sn = dgrad ? p.y_sn : p.x_sn;
    const int s_sd = (int)(dgrad ? p.y_sd : p.x_sd), s_sh = (int)(dgrad ? p.y_sh : p.x_sh),
              s_sw = (int)(dgrad ? p.y_sw : p.x_sw);
    const float* __restrict__ wt = p.w;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int kv = tid % KV, r0 = tid / KV;

    // ---- per-thread A rows --------------------------------------------------------------------------------
    long long a_base[FX ? 1 : RA];
    int a_cd[FX ? 1 : RA], a_ch[FX ? 1 : RA], a_cw[FX ? 1 : RA];
    bool a_ok[FX ? 1 : RA];
    // fixed problems: the row's source offset at tap (0, 0, 0), in elements (FdFixedP asserts that the tensor's extent fits 31 bits), and
    // its tap mask: bit j of byte 0 / 1 / 2 = reduced tap j along W / H / D reads inside the image
    int a_off[FX ? RA : 1];
    unsigned a_msk[FX ? RA : 1];
#pragma unroll
    for (int j = 0; j < RA; ++j) {
        int m = m0 + r0 + RP * j;
        const bool rok = m < Mtot;
        int mm = rok ? m : 0;
        int qw = mm % gw.Mdim; mm /= gw.Mdim;
        int qh = mm % gh.Mdim; mm /= gh.Mdim;
        int qd = mm % gd.Mdim; int n = mm / gd.Mdim;
        if constexpr (FX) {
            const int cd = gd.base + qd * gd.mstep, ch = gh.base + qh * gh.mstep, cw = gw.base + qw * gw.mstep;
            a_off[j] = n * (int)s_sn + cd * s_sd + ch * s_sh + cw * s_sw;
            unsigned msk = 0u;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (t < p.kw && t < gw.nt && (unsigned)(cw + t * gw.jstep) < (unsigned)gw.srcN) msk |= 1u << t;
                if (t < p.kh && t < gh.nt && (unsigned)(ch + t * gh.jstep) < (unsigned)gh.srcN) msk |= 1u << (8 + t);
                if (t < p.kd && t < gd.nt && (unsigned)(cd + t * gd.jstep) < (unsigned)gd.srcN) msk |= 1u << (16 + t);
            }
            a_msk[j] = rok ? msk : 0u;
        } else {
            a_ok[j] = rok;
            a_base[j] = (long long)n * s_sn;
            a_cd[j] = gd.base + qd * gd.mstep;
            a_ch[j] = gh.base + qh * gh.mstep;
            a_cw[j] = gw.base + qw * gw.mstep;
        }
    }
    // ---- per-thread B rows --------------------------------------------------------------------------------
    bool b_ok[RB];
    long long b_base[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
        int n = n0 + r0 + RP * j;
        b_ok[j] = n < Nout;
        b_base[j] = (long long)(b_ok[j] ? n : 0) * ldb;
    }
    // ---- K state (vector path): this thread's float4 sits at k = kt*32 + kv*4 -------------------------------
    // split-K: this workgroup reduces K-tiles [kt_begin, kt_end)
    const int nk_all = (K + BKT - 1) / BKT;
    const int kt_per = (nk_all + p.splitk - 1) / p.splitk;
    const int kt_begin = split * kt_per;
    const int kt_end = min(nk_all, kt_begin + kt_per);
    int kc = 0, jd = 0, jh = 0, jw = 0;     // channel offset, reduced tap indices
    if (VEC) {
        int k = kt_begin * BKT + kv * 4;
        kc = k % Cred; int tap = k / Cred;
        jw = tap % max(gw.nt, 1); tap /= max(gw.nt, 1);
        jh = tap % max(gh.nt, 1); jd = tap / max(gh.nt, 1);
    }

    float4 ra[RA], rb[RB];
    // bf16 weight stream: thread -> (row r0b + 32*j, 8-wide k chunk kvb)
    constexpr int RB16 = BN / 32;
    const int kvb = tid & 7, r0b = tid >> 3;
    uint4 rb16[WB16 ? RB16 : 1];
    long long bb16[WB16 ? RB16 : 1];
    bool bok16[WB16 ? RB16 : 1];
    int kcb = 0, jdb = 0, jhb = 0, jwb = 0;
    if (WB16) {
#pragma unroll
        for (int j = 0; j < RB16; ++j) {
            int n = n0 + r0b + 32 * j;
            bok16[j] = n < Nout;
            bb16[j] = (long long)(bok16[j] ? n : 0) * ldb;
        }
        int k = kt_begin * BKT + kvb * 8;
        kcb = k % Cred; int tap = k / Cred;
        jwb = tap % max(gw.nt, 1); tap /= max(gw.nt, 1);
        jhb = tap % max(gh.nt, 1); jdb = tap / max(gh.nt, 1);
    }

    // advance a (channel offset, tap) position by one K-tile.  Fixed problems: Cred is a constant, so BKT = ADV * Cred + REM steps ADV taps
    // and at most one more -- the same positions as the loop below, without the loop
    auto advance = [&](int& c, int& td, int& th, int& tw) {
        if constexpr (FX) {
            constexpr int CR = (P::mode == SAVP_CONV_DGRAD) ? P::Cy : P::Cx;
            constexpr int ADV = BKT / CR, REM = BKT % CR;
#pragma unroll
            for (int i = 0; i < ADV; ++i)
                if (++tw >= gw.nt) { tw = 0; if (++th >= gh.nt) { th = 0; ++td; } }
            if (REM) {
                c += REM;
                if (c >= CR) {
                    c -= CR;
                    if (++tw >= gw.nt) { tw = 0; if (++th >= gh.nt) { th = 0; ++td; } }
                }
            }
        } else {
            c += BKT;
            while (c >= Cred) {
                c -= Cred;
                if (++tw >= gw.nt) { tw = 0; if (++th >= gh.nt) { th = 0; ++td; } }
            }
        }
    };

    auto fetch = [&](int kt) {
        if (WB16) {
            const bool kokb = (jdb < gd.nt) && (ntaps > 0);
            const int ta = gd.t0 + jdb * gd.tstep, tu = gh.t0 + jhb * gh.tstep, tv = gw.t0 + jwb * gw.tstep;
            if constexpr (FX) {
                const int woff = ((ta * p.kh + tu) * p.kw + tv) * Cred + kcb;
#pragma unroll
                for (int j = 0; j < RB16; ++j) {
                    const bool ok = bok16[j] && kokb;
                    uint4 v = *reinterpret_cast<const uint4*>(p.w16 + (unsigned)(ok ? (int)bb16[j] + woff : 0));
                    rb16[j] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
                }
            } else {
                const long long woff = (long long)((ta * p.kh + tu) * p.kw + tv) * Cred + kcb;
#pragma unroll
                for (int j = 0; j < RB16; ++j) {
                    const bool ok = bok16[j] && kokb;
                    uint4 v = *reinterpret_cast<const uint4*>(p.w16 + (ok ? bb16[j] + woff : 0ll));
                    rb16[j] = ok ? v : make_uint4(0u, 0u, 0u, 0u);
                }
            }
            advance(kcb, jdb, jhb, jwb);
        }
        if constexpr (VEC) {
            const bool kok = (jd < gd.nt) && (ntaps > 0);
            if constexpr (FX) {
                // one tap offset and one tap-bit pattern per K-tile; a row is read where its mask has all three bits
                const unsigned tb = kok ? ((1u << jw) | (1u << (8 + jh)) | (1u << (16 + jd))) : 0xffffffffu;
                const int toff = jd * gd.jstep * s_sd + jh * gh.jstep * s_sh + jw * gw.jstep * s_sw + kc;
#pragma unroll
                for (int j = 0; j < RA; ++j) {
                    const bool ok = (a_msk[j] & tb) == tb;
                    float4 v = ldg4(src + (unsigned)(ok ? a_off[j] + toff : 0));
                    ra[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
                const int zd0 = jd * gd.jstep, zh0 = jh * gh.jstep, zw0 = jw * gw.jstep;
#pragma unroll
                for (int j = 0; j < RA; ++j) {
                    int zd = a_cd[j] + zd0, zh = a_ch[j] + zh0, zw = a_cw[j] + zw0;
                    bool ok = a_ok[j] && kok && (unsigned)zd < (unsigned)gd.srcN && (unsigned)zh < (unsigned)gh.srcN &&
                              (unsigned)zw < (unsigned)gw.srcN;
                    // branch-free: out-of-image taps read a safe address and are zeroed by a select, so all gathers of a K-tile
                    // are issued back to back (a branch per load serialised them and cost an s_cbranch each)
                    const long long off = ok ? (a_base[j] + (long long)zd * s_sd + (long long)zh * s_sh + (long long)zw * s_sw + kc) : 0ll;
                    float4 v = ldg4(src + off);
                    ra[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            const int ta = gd.t0 + jd * gd.tstep, tu = gh.t0 + jh * gh.tstep, tv = gw.t0 + jw * gw.tstep;
            if (!WB16) {
                if constexpr (FX) {
                    const int woff = ((ta * p.kh + tu) * p.kw + tv) * Cred + kc;
#pragma unroll
                    for (int j = 0; j < RB; ++j) {
                        const bool ok = b_ok[j] && kok;
                        float4 v = ldg4(wt + (unsigned)(ok ? (int)b_base[j] + woff : 0));
                        rb[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                } else {
                    const long long woff = (long long)((ta * p.kh + tu) * p.kw + tv) * Cred + kc;
#pragma unroll
                    for (int j = 0; j < RB; ++j) {
                        const bool ok = b_ok[j] && kok;
                        float4 v = ldg4(wt + (ok ? b_base[j] + woff : 0ll));
                        rb[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
            }
            // advance by the K-tile
            advance(kc, jd, jh, jw);
        } else {
            // scalar path: arbitrary Cred (first layers with 3/6/14 channels, the 53-channel mask conv)
            float av[RA][4], bv[RB][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int k = kt * BKT + kv * 4 + e;
                bool kok = k < K;
                int kk = kok ? k : 0;
                int c = kk % Cred; int tap = kk / Cred;
                int tw_ = tap % max(gw.nt, 1); tap /= max(gw.nt, 1);
                int th_ = tap % max(gh.nt, 1); int td_ = tap / max(gh.nt, 1);
#pragma unroll
                for (int j = 0; j < RA; ++j) {
                    int zd = a_cd[j] + td_ * gd.jstep, zh = a_ch[j] + th_ * gh.jstep, zw = a_cw[j] + tw_ * gw.jstep;
                    bool ok = a_ok[j] && kok && (unsigned)zd < (unsigned)gd.srcN && (unsigned)zh < (unsigned)gh.srcN &&
                              (unsigned)zw < (unsigned)gw.srcN;
                    av[j][e] = ok ? src[a_base[j] + (long long)zd * s_sd + (long long)zh * s_sh + (long long)zw * s_sw + c] : 0.f;
                }
                int ta = gd.t0 + td_ * gd.tstep, tu = gh.t0 + th_ * gh.tstep, tv = gw.t0 + tw_ * gw.tstep;
                long long woff = (long long)((ta * p.kh + tu) * p.kw + tv) * Cred + c;
#pragma unroll
                for (int j = 0; j < RB; ++j) bv[j][e] = (b_ok[j] && kok) ? wt[b_base[j] + woff] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < RA; ++j) ra[j] = make_float4(av[j][0], av[j][1], av[j][2], av[j][3]);
#pragma unroll
            for (int j = 0; j < RB; ++j) rb[j] = make_float4(bv[j][0], bv[j][1], bv[j][2], bv[j][3]);
        }
    };
    auto stage = [&](int buf) {
        char* a = As + buf * BM * ROWB;
        char* b = Bs + buf * BN * ROWB;
        if (BF16) {
#pragma unroll
            for (int j = 0; j < RA; ++j) {
                bf16x4 v = {(__bf16)ra[j].x, (__bf16)ra[j].y, (__bf16)ra[j].z, (__bf16)ra[j].w};
                *reinterpret_cast<bf16x4*>(a + (r0 + RP * j) * ROWB + kv * 8) = v;
            }
            if (WB16) {
#pragma unroll
                for (int j = 0; j < RB16; ++j) *reinterpret_cast<uint4*>(b + (r0b + 32 * j) * ROWB + kvb * 16) = rb16[j];
            } else {
#pragma unroll
                for (int j = 0; j < RB; ++j) {
                    bf16x4 v = {(__bf16)rb[j].x, (__bf16)rb[j].y, (__bf16)rb[j].z, (__bf16)rb[j].w};
                    *reinterpret_cast<bf16x4*>(b + (r0 + RP * j) * ROWB + kv * 8) = v;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < RA; ++j) *reinterpret_cast<float4*>(a + (r0 + RP * j) * ROWB + kv * 16) = ra[j];
#pragma unroll
            for (int j = 0; j < RB; ++j) *reinterpret_cast<float4*>(b + (r0 + RP * j) * ROWB + kv * 16) = rb[j];
        }
    };

    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int wm0 = (wave >> 1) * 32 * WM, wn0 = (wave & 1) * 32 * WN;
    const int l31 = lane & 31, khalf = lane >> 5;
    // software pipeline: LDS holds tile kt (cur) while the registers hold tile kt+1 whose global loads were issued one
    // whole iteration earlier (right after the previous stage), so they fly under a barrier + a full MFMA block.
    if (kt_begin < kt_end) {
        fetch(kt_begin);
        stage(0);
        if (kt_begin + 1 < kt_end) fetch(kt_begin + 1);
    }
    __syncthreads();
    for (int kt = kt_begin; kt < kt_end; ++kt) {
        const int cur = (kt - kt_begin) & 1;
        const char* a = As + cur * BM * ROWB;
        const char* b = Bs + cur * BN * ROWB;
        if (BF16) {
#pragma unroll
            for (int ks = 0; ks < BKT / 16; ++ks) {
                bf16x8 af[WM], bf[WN];
#pragma unroll
                for (int i = 0; i < WM; ++i)
                    af[i] = *reinterpret_cast<const bf16x8*>(a + (wm0 + i * 32 + l31) * ROWB + (ks * 16 + khalf * 8) * 2);
#pragma unroll
                for (int j = 0; j < WN; ++j)
                    bf[j] = *reinterpret_cast<const bf16x8*>(b + (wn0 + j * 32 + l31) * ROWB + (ks * 16 + khalf * 8) * 2);
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int c8 = 0; c8 < BKT / 8; ++c8) {
                float4 af[WM], bf[WN];
#pragma unroll
                for (int i = 0; i < WM; ++i)
                    af[i] = *reinterpret_cast<const float4*>(a + (wm0 + i * 32 + l31) * ROWB + (c8 * 8 + khalf * 4) * 4);
#pragma unroll
                for (int j = 0; j < WN; ++j)
                    bf[j] = *reinterpret_cast<const float4*>(b + (wn0 + j * 32 + l31) * ROWB + (c8 * 8 + khalf * 4) * 4);
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                    }
            }
        }
        if (kt + 1 < kt_end) {
            stage(cur ^ 1);
            if (kt + 2 < kt_end) fetch(kt + 2);
        }
        __syncthreads();
    }

    // ---- epilogue: destination row offsets through LDS -------------------------------------------------------
    long long* rowoff = reinterpret_cast<long long*>(smem);     // [BM], -1 = invalid (safe: last barrier of the loop passed)
    float* __restrict__ dst = p.out;
    const long long d_sn = dgrad ? p.x_sn : p.y_sn;
    const long long d_sd = dgrad ? p.x_sd : p.y_sd, d_sh = dgrad ? p.x_sh : p.y_sh, d_sw = dgrad ? p.x_sw : p.y_sw;
    if (tid < BM) {
        int m = m0 + tid;
        long long off = -1;
        if (m < Mtot) {
            int mm = m;
            int qw = mm % gw.Mdim; mm /= gw.Mdim;
            int qh = mm % gh.Mdim; mm /= gh.Mdim;
            int qd = mm % gd.Mdim; int n = mm / gd.Mdim;
            off = (long long)n * d_sn + (long long)(gd.ob + qd * gd.os) * d_sd + (long long)(gh.ob + qh * gh.os) * d_sh +
                  (long long)(gw.ob + qw * gw.os) * d_sw;
        }
        rowoff[tid] = off;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int col = n0 + wn0 + j * 32 + l31;
        if (col >= Nout) continue;
        const float bias = (p.bias && split == 0) ? p.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < WM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                const long long off = rowoff[row];
                if (off < 0) continue;
                float v = acc[i][j][r] + bias;
                float* q = dst + off + col;
                if (p.splitk > 1) {               // this split's share (conv_common.h: deterministic split-K)
                    (p.part + (long long)split * p.part_sz + (dst - p.out))[off + col] = v;
                    continue;
                }
                if (p.beta) v += *q;
                if (p.act == SAVP_ACT_LRELU) v = fmaxf(v, p.alpha * v);
                else if (p.act == SAVP_ACT_SIGMOID) v = 1.f / (1.f + __expf(-v));
                else if (p.act == SAVP_ACT_DLRELU_FROM_OUT) v *= (p.aux[off + col] > 0.f ? 1.f : p.alpha);
                *q = v;
            }
        }
    }
}

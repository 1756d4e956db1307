// conv_ring.hip -- LDS-patch convolution with an LDS-DMA weight ring and a fused "cell" epilogue, gfx950, bf16 MFMA.
//
// Same tiling idea as conv_patch.hip (a workgroup owns NI images x TIH rows x 8 columns of output pixels, the input patch of a
// group of channel slabs is parked in LDS once, every tap's A fragment is that patch read at a tap-shifted address) with the two
// parts of that kernel that its own ablation found on the critical path rebuilt:
//
//   * weight stream: the (tap, slab) weight slabs no longer travel global -> VGPR -> ds_write behind a barrier per slab.  Every
//     wave issues `global_load_lds_dwordx4` (LDS-DMA, inline asm so that hipcc neither counts nor drains it) straight into a
//     FOUR-deep LDS ring; slabs i+2 and i+3 are in flight while slab i is multiplied, the loop waits with a counted `s_waitcnt vmcnt(LW)`
//     and a raw `s_barrier` (DMA requests stay in flight across it).  The LDS image keeps the conflict-free row pitch of
//     conv_patch.hip (16 B x odd): the DMA destination is lane-linear, so the pad slot of every row is simply one more 16-byte
//     lane whose source address is a duplicate.  No VGPRs, no ds_write, no exposed L2 latency per slab.
//   * epilogue "cell" mode (the ConvLSTM gate convolution, rnn_ops.py:121,148-149): the accumulators are (a) reduced to the
//     per-(sample, channel) sum / sum of squares the instance norm over the 4F gate pre-activations needs (registers -> LDS ->
//     ONE global atomic per (image, channel) per workgroup; the separate statistics pass over the gate tensor disappears) and
//     (b) rounded to bf16, transposed through LDS and stored as full 16-byte pieces of contiguous pixel rows (the fp32 epilogue
//     of conv_patch.hip stores 16 strided dwords per lane).  The gate tensor makes its HBM round trip in half the bytes.
//
// Applies to stride-1 and strided 2-D / 3-D FPROP and DGRAD problems in SAVP_PREC_BF16 exactly like conv_patch.hip (same ConvP
// geometry fields, filled by conv_ring_try); the plain fp32 epilogue (bias / LeakyReLU / sigmoid / beta / split-K) is kept.
#define SAVP_RING_MAIN_TU        // developer stamps builds: this translation unit exports the stamp readers
#include "conv_ring_kernel.h"
#include "conv_ring_fixed.h"

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(16))) unsigned g_ring_zero[4] = {0u, 0u, 0u, 0u};      // source of the DMA-staged patch's zero slots

template <int NW, int WM, int WN, int NKS>
static hipError_t launch_ring(const ConvP& p, dim3 grid, size_t lds, hipStream_t st) {
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
        hipFuncSetAttribute((const void*)conv_ring_kernel<NW, WM, WN, NKS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_lds = lds;
    }
    if (g_savp_prof_start) {                                     // bench.py: kernel-only timing of this one launch (common.hip)
        hipExtLaunchKernelGGL((conv_ring_kernel<NW, WM, WN, NKS>), grid, dim3(64 * NW), lds, st, g_savp_prof_start, g_savp_prof_stop, 0, p);
        g_savp_prof_start = g_savp_prof_stop = nullptr;
    } else {
        hipLaunchKernelGGL((conv_ring_kernel<NW, WM, WN, NKS>), grid, dim3(64 * NW), lds, st, p);
    }
    return hipGetLastError();
}

template <int NW, int WM, int WN>
static hipError_t launch_ring_nks(const ConvP& p, int nks, dim3 grid, size_t lds, hipStream_t st) {
    switch (nks) {
        case 1: return launch_ring<NW, WM, WN, 1>(p, grid, lds, st);
        case 2: return launch_ring<NW, WM, WN, 2>(p, grid, lds, st);
        case 3: return launch_ring<NW, WM, WN, 3>(p, grid, lds, st);
        case 4: return launch_ring<NW, WM, WN, 4>(p, grid, lds, st);
        case 5: return launch_ring<NW, WM, WN, 5>(p, grid, lds, st);
        default: return launch_ring<NW, WM, WN, 6>(p, grid, lds, st);
    }
}

template <int NW>
static hipError_t launch_ring_tile(const ConvP& p, int wm, int wn, int nks, dim3 grid, size_t lds, hipStream_t st) {
    if (wm == 2 && wn == 2) return launch_ring_nks<NW, 2, 2>(p, nks, grid, lds, st);
    if (wm == 2 && wn == 1) return launch_ring_nks<NW, 2, 1>(p, nks, grid, lds, st);
    if (wm == 1 && wn == 2) return launch_ring_nks<NW, 1, 2>(p, nks, grid, lds, st);
    // wide slabs (tile bit 0x1000): 8 / 9 k-steps per entry, instantiated for the 32 x 32 wave tile only (two fragment sets of a wider
    // wave tile would not fit 256 VGPRs)
    if (nks == 8) return launch_ring<NW, 1, 1, 8>(p, grid, lds, st);
    if (nks == 9) return launch_ring<NW, 1, 1, 9>(p, grid, lds, st);
    return launch_ring_nks<NW, 1, 1>(p, nks, grid, lds, st);
}

struct RingPlan { int nw, wm, wn, nks; size_t lds; dim3 grid; };

// Geometry of one (nw, wm, wn) choice; false = this choice cannot run the problem (LDS, cell-mode tiling constraints, ...).
static bool ring_plan(ConvP& p, const SavpConvArgs* a, int nw, int wm, int wn, RingPlan& pl) {
    const bool dg = a->mode == SAVP_CONV_DGRAD;
    const int Cred = dg ? a->Cy : a->Cx, Nout = dg ? a->Cx : a->Cy;
    const int Dm = dg ? a->D : a->Do;
    const int phases = dg ? a->sh * a->sw : 1;
    const int Hm = dg ? (a->H + a->sh - 1) / a->sh : a->Ho, Wm = dg ? (a->W + a->sw - 1) / a->sw : a->Wo;
    const long long dH = dg ? a->H : a->Ho, dW_ = dg ? a->W : a->Wo;
    const long long d_sn = dg ? a->x_sn : a->y_sn, d_sh = dg ? a->x_sh : a->y_sh, d_sw = dg ? a->x_sw : a->y_sw;
    const long long d_sd = dg ? a->x_sd : a->y_sd;
    const int tW = (Wm + 7) / 8;
    // slab split, tile rows, patch and ring footprint: constexpr code shared with the fixed-problem table (conv_ring_fixed.h)
    RingTiling t{};
    if (!ring_tiling(a, nw, wm, wn, t)) return false;
    const int nch = t.nch, nks = t.nks, tih = t.tih, ni = t.ni, PH = t.PH, PW = t.PW, spp = t.spp, pitch = t.pitch, BM = t.BM, BN = t.BN;
    size_t lds = (size_t)t.lds;
    const size_t budget = 160 * 1024;
    const bool cell = a->out_bf16 != 0;
    if (cell) {
        const size_t epi = (size_t)ring_cell_lds(t);
        if (epi > lds) lds = epi;
        if (lds > budget) return false;
        const long long nimg = (long long)a->N * Dm;
        if (a->bias || a->act != SAVP_ACT_NONE || a->beta || Hm % tih || Wm % 8 || Nout % BN || nimg % ni || (d_sw % 8) || (d_sh % 8) ||
            (d_sn % 8) || (d_sd % 8) || ((((uintptr_t)(dg ? a->x : a->y)) & 15) != 0) || phases != 1)
            return false;
    }
    if ((long long)a->N * Dm >= (1 << 24)) return false;
    if ((long long)ni * PH * PW * spp * nks * 4 >= (1 << 24)) return false;
    p.cell = cell ? 1 : 0;
    p.stats = (double*)a->stats;
    if (a->stats && !cell) {
        // statistics of an fp32 destination: whole tiles only (every accumulator is a real output), no split-K, nothing after the bias
        const long long nimg = (long long)a->N * Dm;
        const bool even = !dg || (a->H % a->sh == 0 && a->W % a->sw == 0);       // every output phase has the same extent
        if (a->act != SAVP_ACT_NONE || a->beta || Hm % tih || Wm % 8 || nimg % ni || !even || (a->splitk > 1) ||
            (size_t)(BM / 32) * BN * 2 * 4 > lds)
            return false;
    }
    if (a->nb_ws) {
        // norm-backward statistics: whole tiles (every accumulator is a real output of one image), unit strides (destination pixel (y, x)
        // is pixel y * Wm + x of nb_x), depth 1, no split-K, nothing after the accumulators, an fp32 destination
        const long long nimg = (long long)a->N * Dm;
        // (split-K is fine: both sums are linear in the accumulators -- the mask depends on x only -- so every split adds its share)
        if (cell || a->stats || a->act != SAVP_ACT_NONE || a->beta || Hm % tih || Wm % 8 || nimg % ni || phases != 1 || Dm != 1 ||
            a->sh != 1 || a->sw != 1 || a->nb_c0 + a->nb_nc > Nout || (size_t)(BM / 32) * BN * 2 * 4 > lds)
            return false;
    }
    ring_tiling_fields(p, a, t);       // patch geometry, its fast-division magics, tile counts
    // LDS-DMA patch staging: bf16 source whose pixel rows are 16-byte aligned runs (option "ring_dma" = 0: the VGPR path, for A/B)
    {
        const long long ssn = dg ? a->y_sn : a->x_sn, ssd = dg ? a->y_sd : a->x_sd, ssh = dg ? a->y_sh : a->x_sh, ssw = dg ? a->y_sw : a->x_sw;
        const void* sptr = dg ? a->y : a->x;
        p.dma_patch = (savp_opt(OPT_RING_DMA) && a->src_bf16 && (ssn % 8 == 0) && (ssd % 8 == 0) && (ssh % 8 == 0) && (ssw % 8 == 0) &&
                       ((((uintptr_t)sptr) & 15) == 0) && p.zero16 && (long long)ni * PH * (pitch / 8) < (1 << 24) && (long long)PH * (pitch / 8) < 65536 && (pitch % 8 == 0) &&
                       (nks <= 2 || (pitch / 8 <= 512 && ssw * (long long)(a->W + a->kw) + Cred < (1ll << 30)))) ? 1 : 0;       // row-wise staging (nks >= 3): <= 8 DMA instructions per patch row, 32-bit in-row offsets
    }
    const long long tiles = (long long)p.tm * p.tn;
    const long long iters = (long long)(dg ? (a->kh / a->sh) * (a->kw / a->sw) : a->kh * a->kw) * nch * a->kd;
    int splitk = a->splitk;
    if (a->act != SAVP_ACT_NONE || cell || a->stats) splitk = 1;
    else if (splitk <= 0) {
        splitk = 1;
        if (tiles <= 192 && iters >= 16) {
            long long s1 = 512 / tiles, s2 = iters / 8;
            splitk = (int)(s1 < s2 ? s1 : s2);
            if (splitk < 1) splitk = 1;
            if (splitk > 16) splitk = 16;
        }
    }
    if (splitk > iters) splitk = (int)iters;
    if (splitk > 1) {
        const long long dD = Dm;
        // the destination must be one dense block: split s stores its share at the same offsets of its slice of the scratch (a column
        // gap's channels are cleared by the fold: nobody reads them)
        const long long Cd = Nout + p.gap;
        const bool dense = (d_sw == Cd) && (d_sh == dW_ * Cd) && (dD == 1 || d_sd == dH * dW_ * Cd) &&
                           (d_sn == dD * dH * dW_ * Cd);
        if (!dense) splitk = 1;
        else {
            p.part_sz = (long long)a->N * dD * dH * dW_ * Cd;
            splitk = splitk_fit(a, splitk, p.part_sz);
            p.part = (float*)a->ws;
        }
    }
    p.splitk = splitk;
    patch_launch_constants(p, a, phases, tih, nch, spp, tW, splitk);
    p.wwarm = savp_opt(OPT_RING_WWARM) ? 1 : 0;
    p.early = savp_opt(OPT_RING_EARLY) ? 1 : 0;
    pl.nw = nw; pl.wm = wm; pl.wn = wn; pl.nks = nks; pl.lds = lds;
    pl.grid = dim3((unsigned)(p.tm * p.tn), (unsigned)phases, (unsigned)splitk);
    return true;
}

// Returns true when the ring kernel handled the call (*rc = status); false = not applicable (the caller falls back).
// SavpConvArgs.out_bf16 selects the cell epilogue: bf16 destination + optional statistics; with an automatic tile the first
// (waves, tile) choice whose tiling can honour it is taken, a forced tile that cannot is refused (false).
bool conv_ring_try(ConvP& p, const SavpConvArgs* a, int wm, int wn, hipStream_t st, int* rc, bool dry) {
    const bool dg = a->mode == SAVP_CONV_DGRAD;
    const int Cred = dg ? a->Cy : a->Cx, Nout = dg ? a->Cx : a->Cy;
    const long long ssn = dg ? a->y_sn : a->x_sn, ssh = dg ? a->y_sh : a->x_sh, ssw = dg ? a->y_sw : a->x_sw;
    const void* sptr = dg ? a->y : a->x;
    const int sal = p.src16 ? 8 : 4;                             // source alignment in elements (8 / 16 bytes per load)
    const bool src_al = (ssn % sal == 0) && (ssh % sal == 0) && (ssw % sal == 0) && ((((uintptr_t)sptr) & (p.src16 ? 7 : 15)) == 0);
    const long long ssd = dg ? a->y_sd : a->x_sd;
    if (!(p.bf16 && p.w16 && a->sd == 1 && a->sh <= 4 && a->sw <= 4 && a->kh >= a->sh && a->kw >= a->sw && (Cred % 8 == 0) &&
          src_al && ssd % sal == 0))
        return false;
    const int Hm = dg ? (a->H + a->sh - 1) / a->sh : a->Ho, Wm = dg ? (a->W + a->sw - 1) / a->sw : a->Wo;
    const long long dH = dg ? a->H : a->Ho;
    const long long d_sh = dg ? a->x_sh : a->y_sh;
    if (ssh * (a->H + a->kh) >= (1ll << 30) || d_sh * (dH + 16) >= (1ll << 30) || (long long)(Nout + p.gap) * a->kh * a->kw * a->kd * Cred >= (1ll << 30))
        return false;
    if (p.gap && (a->out_bf16 || a->stats)) return false;        // the gap lives in the plain epilogue only
    if ((long long)Hm * Wm < 16) return false;
    // address of g_ring_zero: a device symbol has one address PER DEVICE, so the cache is indexed by the current device's ordinal (a
    // process that drives several GPUs -- SAVP_DIST_BACKEND=gloo with differing device indices, library users outside the
    // one-process-per-GPU runners -- must not hand device 0's pointer to a kernel on device 1)
    static const void* zero16_of[64] = {nullptr};
    int dev_ord = 0;
    if (hipGetDevice(&dev_ord) != hipSuccess || dev_ord < 0 || dev_ord >= 64) dev_ord = 0;
    if (!dry && !zero16_of[dev_ord] && hipGetSymbolAddress((void**)&zero16_of[dev_ord], HIP_SYMBOL(g_ring_zero)) != hipSuccess) zero16_of[dev_ord] = nullptr;
    p.zero16 = zero16_of[dev_ord];
    RingPlan pl;
    bool ok = false;
    if (wm) {
        ok = ring_plan(p, a, (a->tile & 0x400) ? 8 : 4, wm, wn, pl);
    } else {
        const int tW = (Wm + 7) / 8;
        const int wn0 = Nout > 64 ? 2 : 1;
        const long long t16 = (long long)a->N * ((Hm + 15) / 16) * tW * ((Nout + 64 * wn0 - 1) / (64 * wn0));
        const int wm0 = (t16 >= 256 && Hm >= 16) ? 2 : 1;
        const int cand[5][3] = {{8, wm0, wn0}, {8, 1, wn0}, {4, 1, wn0}, {8, 1, 1}, {4, 1, 1}};
        for (int i = 0; i < 5 && !ok; ++i) ok = ring_plan(p, a, cand[i][0], cand[i][1], cand[i][2], pl);
    }
    if (!ok) return false;
    if (dry) return true;                                        // savp_conv_stats_ok: the plan exists, nothing is launched
    ablate_init();
#ifdef SAVP_RING_LOG
    // developer build: one line per ring launch -- the planned problem as the constexpr table of conv_ring_fixed.h lists it, and the call
    // site's views / epilogue switches (tests/tools/ring_problems.py counts the distinct lines of a step)
    fprintf(stderr, "RINGLOG mode=%d N=%d in=%d,%d,%d,%d out=%d,%d,%d,%d k=%d,%d,%d s=%d,%d,%d p=%d,%d,%d nw=%d wm=%d wn=%d nks=%d splitk=%d src16=%d cell=%d "
            "dma=%d pre=%d gap=%d,%d wwarm=%d early=%d beta=%d act=%d alpha=%g bias=%d stats=%d aux=%d nb=%d,%d,%d,%d,%g nbx=%lld,%lld xs=%lld,%lld,%lld,%lld "
            "ys=%lld,%lld,%lld,%lld atile=0x%x asplitk=%d\n",
            p.mode, p.N, p.D, p.H, p.W, p.Cx, p.Do, p.Ho, p.Wo, p.Cy, p.kd, p.kh, p.kw, p.sd, p.sh, p.sw, p.pd, p.ph, p.pw, pl.nw, pl.wm, pl.wn, pl.nks,
            p.splitk, p.src16, p.cell, p.dma_patch, p.pre, p.gap_at, p.gap, p.wwarm, p.early, p.beta, p.act, (double)p.alpha, p.bias != nullptr,
            p.stats != nullptr, p.aux != nullptr, p.nb_ws != nullptr, p.nb_c0, p.nb_nc, p.nb_act, (double)p.nb_alpha, p.nb_x_sn, p.nb_x_sp,
            p.x_sn, p.x_sd, p.x_sh, p.x_sw, p.y_sn, p.y_sd, p.y_sh, p.y_sw, a->tile, a->splitk);
    fprintf(stderr, "RINGFIXED %d\n", savp_opt(OPT_RING_FIXED) ? ring_fixed_find(p, pl.nw, pl.wm, pl.wn, pl.nks, pl.lds, (int)pl.grid.y) : -1);
#endif
    // option "ring_fixed": a call whose planned geometry equals a fixed problem's in every folded value runs that problem's instantiation
    // (same body, geometry as compile-time constants, conv_ring_fixed.h); every other call the generic kernel
    const int fixed = savp_opt(OPT_RING_FIXED) ? ring_fixed_find(p, pl.nw, pl.wm, pl.wn, pl.nks, pl.lds, (int)pl.grid.y) : -1;
    hipError_t err;
    if (fixed >= 0) {
        savp_opt_count(OPT_RING_FIXED_TAKEN);
        err = fixed % 3 == 0 ? ring_fixed_launch_a(fixed, p, pl.grid, pl.lds, st)
            : fixed % 3 == 1 ? ring_fixed_launch_b(fixed, p, pl.grid, pl.lds, st) : ring_fixed_launch_c(fixed, p, pl.grid, pl.lds, st);
    } else {
        err = (pl.nw == 8) ? launch_ring_tile<8>(p, pl.wm, pl.wn, pl.nks, pl.grid, pl.lds, st)
                           : launch_ring_tile<4>(p, pl.wm, pl.wn, pl.nks, pl.grid, pl.lds, st);
    }
    if (p.splitk > 1 && err == hipSuccess) {
        splitk_fold(p.out, p.part, p.splitk, p.part_sz, a->beta, Nout + p.gap, p.gap ? p.gap_at : 0, p.gap, st);
        err = hipGetLastError();
    }
    *rc = (err == hipSuccess) ? SAVP_OK : SAVP_ELAUNCH;
    return true;
}

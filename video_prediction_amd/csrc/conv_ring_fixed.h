// conv_ring_fixed.h -- the ring convolution's tiling as constexpr code, and the table of FIXED problems built from it.
//
// The train step launches the same handful of ring problems once or twice per time step (the generator's ladder convolutions, their data
// gradients, the ConvLSTM gate data gradients): H, W, channels, kernel, stride, padding, tile geometry, fast-division magics, slab counts,
// grid decomposition and the staging switches are fixed by the layer.  conv_ring_kernel re-reads all of it from a 550-byte argument block in
// every workgroup of every launch.  conv_ring_fixed_kernel<ID> is the SAME body (conv_ring_kernel.h) with those values folded: its argument
// block RingFixedP<ID> carries pointers and the epilogue's scalars only.
//
//   * ring_tiling / ring_tiling_fields / patch_launch_constants are the code ring_plan (conv_ring.hip) runs for every call; the table's entries
//     are those functions evaluated at compile time on the problem list below -- there is no second copy of the arithmetic to drift.
//   * conv_ring_try plans a call as always and then compares the planned ConvP field by field with the table (ring_fixed_find): only an exact
//     match of every folded value launches the fixed instantiation, anything else -- another N, tile, split count, an unaligned or fp32 source,
//     option ring_dma / ring_wwarm / ring_early off -- takes conv_ring_kernel as before.  Option "ring_fixed" 0 switches the routing off.
//   * What stays an argument: pointers, beta / act / alpha and the nb_* fields -- the float epilogue is compiled from the same runtime
//     switches in both kernels, so hipcc contracts the same products (same bits).  The tensors' strides ARE folded: these call sites pass
//     dense tensors, a view into a wider buffer takes the generic kernel.
#pragma once
#include "conv_common.h"
#include <utility>

// ---- tiling of one (waves, wave tile) choice: the pure-integer part of ring_plan ------------------------------------------------------------
struct RingTiling { int nch, nks, tih, ni, PH, PW, spp, pitch, BM, BN; unsigned long long lds; };

static constexpr inline bool ring_tiling(const SavpConvArgs* a, int nw, int wm, int wn, RingTiling& t) {
    const bool dg = a->mode == SAVP_CONV_DGRAD;
    const int Cred = dg ? a->Cy : a->Cx;
    const int Hm = dg ? (a->H + a->sh - 1) / a->sh : a->Ho;
    // channel slabs: with the DMA ring a slab costs (k-steps + ~0.5), so exact fits beat fewer, wider slabs
    const int Cp16 = (Cred + 15) & ~15;
    // Wide slabs (tile bit 0x1000, 32 x 32 wave tile): up to 9 k-steps per (tap, slab) entry -- 144 channels are ONE slab (25 entries
    // instead of 75 for the 16x16 gate convolution), 256 / 512 channels split 2 x 8 / 4 x 8 without padding.  The per-entry costs that
    // do not scale with the slab (barrier, table, address arithmetic) are paid a third as often; the ring needs more LDS per slot.
    const int kmax = ((a->tile & 0x1000) && wm == 1 && wn == 1) ? 9 : 6;
    int nch = 0, nks = 0;
    double best = 1e30;
    for (int c = (Cp16 + 16 * kmax - 1) / (16 * kmax); c <= (Cp16 + 95) / 96 + 3; ++c) {
        const int k = (Cp16 / 16 + c - 1) / c;
        if (k < 1 || k > kmax || k == 7) continue;
        const double cost = c * (k + 0.5);
        if (cost < best) { best = cost; nch = c; nks = k; }
    }
    if (!nch) return false;
    if ((a->tile & 0x1000) && nks <= 6) return false;          // nothing wide to offer: let the tuner's plain candidate stand for it
    const int TH = 2 * nw * wm;
    int tih = 4;
    while (tih < TH && tih < Hm) tih *= 2;
    const int ni = TH / tih;
    const int PH = dg ? tih + (a->kh + a->sh - 1) / a->sh - 1 : (tih - 1) * a->sh + a->kh;
    const int PW = dg ? 8 + (a->kw + a->sw - 1) / a->sw - 1 : 7 * a->sw + a->kw;
    const int BM = 16 * nw * wm, BN = 64 * wn, NT = 64 * nw;
    const int RS = 2 * nks + 1;
    const int LW = (BN * RS + NT - 1) / NT;
    const unsigned long long ringb = (unsigned long long)4 * LW * NT * 16;
    const unsigned long long budget = 160 * 1024;
    int spp = nch, pitch = 0;
    unsigned long long lds = 0;
    for (; spp >= 1; --spp) {
        const int CP = spp * nks * 16 + 8;
        const int x = (8 - (PW * (CP / 8)) % 16 + 16) % 16;
        pitch = PW * CP + 8 * x;
        // + dummy slot of stage_patch + entry table of one group (8 bytes per (tap, slab) entry)
        lds = ringb + (unsigned long long)ni * PH * pitch * 2 + 16 +
              (unsigned long long)8 * (dg ? ((a->kh + a->sh - 1) / a->sh) * ((a->kw + a->sw - 1) / a->sw) : a->kh * a->kw) * spp;
        if (lds <= budget) break;
    }
    if (spp < 1) return false;
    t.nch = nch; t.nks = nks; t.tih = tih; t.ni = ni; t.PH = PH; t.PW = PW; t.spp = spp; t.pitch = pitch; t.BM = BM; t.BN = BN; t.lds = lds;
    return true;
}

// the ConvP fields that follow from the tiling alone (patch geometry, its fast-division magics, the tile counts)
static constexpr inline void ring_tiling_fields(ConvP& p, const SavpConvArgs* a, const RingTiling& t) {
    const bool dg = a->mode == SAVP_CONV_DGRAD;
    const int Nout = dg ? a->Cx : a->Cy;
    const int Dm = dg ? a->D : a->Do;
    const int Hm = dg ? (a->H + a->sh - 1) / a->sh : a->Ho, Wm = dg ? (a->W + a->sw - 1) / a->sw : a->Wo;
    const int tW = (Wm + 7) / 8;
    const int CP = t.spp * t.nks * 16 + 8;
    p.s1_ph = t.PH; p.s1_pw = t.PW; p.s1_th = (Hm + t.tih - 1) / t.tih; p.s1_tw = tW; p.s1_tih = t.tih;
    p.s1_pitch = t.pitch; p.s1_nch = t.nch; p.s1_spp = t.spp;
    p.s1_magPI = magic40(t.PH * t.PW * t.spp * t.nks * 4); p.s1_magPW = magic40(t.PW); p.s1_magC4 = magic40(t.spp * t.nks * 4);
    p.s1_magDm = magic40(Dm);
    p.s1_magPI8 = magic40(t.PH * (t.pitch / 8)); p.s1_magP8 = magic40(t.pitch / 8); p.s1_magC8 = magic40(CP / 8);
    p.tm = (int)(((long long)a->N * Dm + t.ni - 1) / t.ni) * p.s1_th * tW; p.tn = (Nout + t.BN - 1) / t.BN;
}

// LDS of the cell epilogue (bf16 tile rows + per-block statistics), which may exceed the main loop's
static constexpr inline unsigned long long ring_cell_lds(const RingTiling& t) {
    return (unsigned long long)t.BM * (t.BN / 2 + 4) * 4 + (unsigned long long)(t.BM / 32) * t.BN * 2 * 4;
}

// ---- the fixed problems ------------------------------------------------------------------------------------------------------------------
// One line per (problem, mode) that the default BAIR train step (64 x 64 x 3, batch 16 -> N = 32 with the VAE branch, bf16) launches once or
// twice per time step, with its shipped tile from tuning_gfx950_bf16.json (tests/tools/ring_problems.py lists them from a step run on a
// -DSAVP_RING_LOG build).  Nothing depends on this list being right or complete: a line that no call matches is never launched, a call that
// matches no line takes the generic kernel.
struct RingFixedDesc {
    int mode, N, H, W, Cx, Ho, Wo, Cy, k, s, pad;      // 2-D square kernels: D = Do = kd = sd = 1, pd = 0
    int nw, wm, wn, wide;                              // tile: waves, wave tile, wide slabs (tile bit 0x1000)
    int splitk, src16, dma_patch, gap_at, gap;         // as planned: K splits, bf16 source, LDS-DMA patch staging, column gap (0x7fffffff, 0: none)
};
#define RING_NOGAP 0x7fffffff, 0
static constexpr RingFixedDesc kRingFixed[] = {
    // ConvLSTM gate data gradients (5x5, source dgates bf16, destination [x | h] without the tiled-z channels)
    {SAVP_CONV_DGRAD, 32, 32, 32, 64, 32, 32, 128, 5, 1, 2,  8, 1, 1, 0,  1, 1, 1, 32, 8},
    {SAVP_CONV_DGRAD, 32, 16, 16, 128, 16, 16, 256, 5, 1, 2,  4, 1, 1, 0,  1, 1, 1, 64, 8},
    {SAVP_CONV_DGRAD, 32, 8, 8, 256, 8, 8, 512, 5, 1, 2,  4, 1, 1, 1,  2, 1, 1, 128, 8},
    // 3x3 at 64 x 64
    {SAVP_CONV_FPROP, 32, 64, 64, 32, 64, 64, 64, 3, 1, 1,  8, 2, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_DGRAD, 32, 64, 64, 32, 64, 64, 64, 3, 1, 1,  8, 2, 1, 0,  1, 1, 1, RING_NOGAP},
    // stride-2 ladder: encoder convolutions (FPROP), their data gradients, the decoder's transposed convolutions (DGRAD as a forward op)
    {SAVP_CONV_FPROP, 32, 64, 64, 16, 32, 32, 32, 6, 2, 2,  4, 1, 1, 0,  1, 0, 0, RING_NOGAP},
    {SAVP_CONV_DGRAD, 32, 64, 64, 16, 32, 32, 32, 6, 2, 2,  8, 2, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_FPROP, 32, 32, 32, 40, 16, 16, 64, 4, 2, 1,  4, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_DGRAD, 32, 32, 32, 40, 16, 16, 64, 4, 2, 1,  8, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_FPROP, 32, 16, 16, 72, 8, 8, 128, 4, 2, 1,  4, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_DGRAD, 32, 16, 16, 72, 8, 8, 128, 4, 2, 1,  4, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_FPROP, 32, 16, 16, 64, 8, 8, 136, 6, 2, 2,  4, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_DGRAD, 32, 16, 16, 64, 8, 8, 136, 6, 2, 2,  4, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_FPROP, 32, 32, 32, 32, 16, 16, 136, 6, 2, 2,  4, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_DGRAD, 32, 32, 32, 32, 16, 16, 136, 6, 2, 2,  8, 1, 1, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_FPROP, 32, 64, 64, 32, 32, 32, 72, 6, 2, 2,  8, 1, 2, 0,  1, 1, 1, RING_NOGAP},
    {SAVP_CONV_DGRAD, 32, 64, 64, 32, 32, 32, 72, 6, 2, 2,  8, 2, 1, 0,  1, 1, 1, RING_NOGAP},
};
#undef RING_NOGAP
static constexpr int kRingFixedCount = (int)(sizeof(kRingFixed) / sizeof(kRingFixed[0]));

// A table entry: the ConvP that ring_plan produces for the problem (geometry fields only; pointers, strides and epilogue scalars stay zero)
struct RingFixedEntry { ConvP p; int nw, wm, wn, nks; unsigned long long lds; int phases; bool ok; };

static constexpr inline RingFixedEntry ring_fixed_entry(int id) {
    const RingFixedDesc& d = kRingFixed[id];
    SavpConvArgs a{};
    a.mode = d.mode; a.N = d.N; a.D = 1; a.H = d.H; a.W = d.W; a.Cx = d.Cx; a.Do = 1; a.Ho = d.Ho; a.Wo = d.Wo; a.Cy = d.Cy;
    a.kd = 1; a.kh = d.k; a.kw = d.k; a.sd = 1; a.sh = d.s; a.sw = d.s; a.pd = 0; a.ph = d.pad; a.pw = d.pad;
    a.tile = d.wide ? 0x1000 : 0;
    RingFixedEntry e{};
    ConvP& p = e.p;
    p.mode = a.mode; p.N = a.N; p.D = a.D; p.H = a.H; p.W = a.W; p.Cx = a.Cx; p.Do = a.Do; p.Ho = a.Ho; p.Wo = a.Wo; p.Cy = a.Cy;
    p.kd = a.kd; p.kh = a.kh; p.kw = a.kw; p.sd = a.sd; p.sh = a.sh; p.sw = a.sw; p.pd = a.pd; p.ph = a.ph; p.pw = a.pw;
    RingTiling t{};
    e.ok = ring_tiling(&a, d.nw, d.wm, d.wn, t);
    if (!e.ok) return e;
    ring_tiling_fields(p, &a, t);
    const bool dg = d.mode == SAVP_CONV_DGRAD;
    e.phases = dg ? d.s * d.s : 1;
    p.cell = 0; p.src16 = d.src16; p.dma_patch = d.dma_patch; p.gap_at = d.gap_at; p.gap = d.gap; p.splitk = d.splitk;
    p.wwarm = 1; p.early = 1;                                  // the shipped option values; another setting matches no entry
    // both tensors dense, as every one of these call sites passes them (a data gradient's destination holds the gap's channels too)
    const long long xc = d.Cx + (dg ? d.gap : 0), yc = d.Cy + (dg ? 0 : d.gap);
    p.x_sw = xc; p.x_sh = xc * d.W; p.x_sn = xc * d.W * d.H; p.x_sd = 0;
    p.y_sw = yc; p.y_sh = yc * d.Wo; p.y_sn = yc * d.Wo * d.Ho; p.y_sd = 0;
    const int Wm = dg ? (d.W + d.s - 1) / d.s : d.Wo;
    patch_launch_constants(p, &a, e.phases, t.tih, t.nch, t.spp, (Wm + 7) / 8, d.splitk);
    e.nw = d.nw; e.wm = d.wm; e.wn = d.wn; e.nks = t.nks; e.lds = t.lds;
    return e;
}

template <size_t... I>
static constexpr auto ring_fixed_entries(std::index_sequence<I...>) {
    struct Tab { RingFixedEntry e[sizeof...(I)]; };
    return Tab{{ring_fixed_entry((int)I)...}};
}
static constexpr auto kRingFixedTab = ring_fixed_entries(std::make_index_sequence<kRingFixedCount>{});

// ---- argument block of conv_ring_fixed_kernel<ID>: ConvP's names, the geometry as compile-time constants ----------------------------------
#define RING_FIXED_FIELDS(F)                                                                                                             \
    F(int, mode) F(int, N) F(int, D) F(int, H) F(int, W) F(int, Cx) F(int, Do) F(int, Ho) F(int, Wo) F(int, Cy)                             \
    F(int, kd) F(int, kh) F(int, kw) F(int, sd) F(int, sh) F(int, sw) F(int, pd) F(int, ph) F(int, pw)                                      \
    F(int, splitk) F(int, tm) F(int, tn) F(int, s1_pitch) F(int, s1_nch) F(int, s1_spp) F(int, s1_ph) F(int, s1_pw) F(int, s1_th)           \
    F(int, s1_tw) F(int, s1_tih) F(unsigned long long, s1_magDm) F(unsigned long long, s1_magPI) F(unsigned long long, s1_magPW)           \
    F(unsigned long long, s1_magC4) F(int, src16) F(int, cell) F(int, dma_patch) F(unsigned long long, s1_magPI8)                          \
    F(unsigned long long, s1_magP8) F(unsigned long long, s1_magC8) F(int, pre) F(int, gap_at) F(int, gap) F(int, wwarm) F(int, early)     \
    F(int, s1_tih_sh) F(int, s1_ngs)                                                                                                      \
    F(long long, x_sn) F(long long, x_sd) F(long long, x_sh) F(long long, x_sw) F(long long, y_sn) F(long long, y_sd) F(long long, y_sh) F(long long, y_sw)
// (valid only with pre = 1: a strided data gradient's depend on the output phase and are derived in the kernel, from constants now)
#define RING_FIXED_PRE_FIELDS(F)                                                                                                         \
    F(int, s1_itper) F(unsigned long long, s1_magTm) F(unsigned long long, s1_magTHW) F(unsigned long long, s1_magTW)                      \
    F(unsigned long long, s1_magKw) F(unsigned long long, s1_magSpp) F(unsigned long long, s1_magTail)
#define RING_FIXED_GEOM_FIELDS(F) F(Mdim) F(base) F(mstep) F(jstep) F(nt) F(t0) F(tstep) F(ob) F(os) F(srcN)

template <int ID>
struct RingFixedP {
    static constexpr RingFixedEntry E = kRingFixedTab.e[ID];
#define F(T, f) static constexpr T f = E.p.f;
    RING_FIXED_FIELDS(F)
    RING_FIXED_PRE_FIELDS(F)
#undef F
    static constexpr DimGeom gD = E.p.gD, gH = E.p.gH, gW = E.p.gW;
    // ---- what a call decides ----
    int beta, act;
    float alpha;
    const float* x;
    const float* y;
    const unsigned short* w16;
    float* out;
    const float* bias;
    const float* aux;
    float* part; long long part_sz;
    double* stats;
    const void* zero16;
    const float* nb_x; long long nb_x_sn, nb_x_sp; const float *nb_mean, *nb_rstd, *nb_gamma, *nb_beta; double* nb_ws;
    int nb_c0, nb_nc, nb_act; float nb_alpha;
};

template <class Q>
static inline void ring_fixed_args(Q& q, const ConvP& p) {
    q.beta = p.beta; q.act = p.act; q.alpha = p.alpha;
    q.x = p.x; q.y = p.y;
    q.w16 = p.w16; q.out = p.out; q.bias = p.bias; q.aux = p.aux; q.part = p.part; q.part_sz = p.part_sz; q.stats = p.stats; q.zero16 = p.zero16;
    q.nb_ws = p.nb_ws;
    if (p.nb_ws) {                                             // (savp_conv fills the rest only with a workspace)
        q.nb_x = p.nb_x; q.nb_x_sn = p.nb_x_sn; q.nb_x_sp = p.nb_x_sp; q.nb_mean = p.nb_mean; q.nb_rstd = p.nb_rstd; q.nb_gamma = p.nb_gamma;
        q.nb_beta = p.nb_beta; q.nb_c0 = p.nb_c0; q.nb_nc = p.nb_nc; q.nb_act = p.nb_act; q.nb_alpha = p.nb_alpha;
    } else {
        q.nb_x = nullptr; q.nb_x_sn = q.nb_x_sp = 0; q.nb_mean = q.nb_rstd = q.nb_gamma = q.nb_beta = nullptr;
        q.nb_c0 = q.nb_nc = q.nb_act = 0; q.nb_alpha = 0.f;
    }
}

// The planned call against one entry: EVERY folded value (the tensors' strides among them), the instantiation and the launch shape; the fixed
// kernels are offered 16-byte aligned tensors only.  (Pointers and the epilogue's scalars are arguments of both kernels and not compared.)
static inline bool ring_fixed_match(const RingFixedEntry& e, const ConvP& p, int nw, int wm, int wn, int nks, unsigned long long lds, int phases) {
    if (!aligned16(p.x) || !aligned16(p.y) || !aligned16(p.w16)) return false;
    if (!e.ok || e.nw != nw || e.wm != wm || e.wn != wn || e.nks != nks || e.lds != lds || e.phases != phases) return false;
#define F(T, f) if (e.p.f != p.f) return false;
    RING_FIXED_FIELDS(F)
    if (p.pre) {
        RING_FIXED_PRE_FIELDS(F)
#undef F
#define F(f) if (e.p.gD.f != p.gD.f || e.p.gH.f != p.gH.f || e.p.gW.f != p.gW.f) return false;
        RING_FIXED_GEOM_FIELDS(F)
#undef F
    }
    return true;
}

// index of the entry the planned call matches, or -1
static inline int ring_fixed_find(const ConvP& p, int nw, int wm, int wn, int nks, unsigned long long lds, int phases) {
    for (int i = 0; i < kRingFixedCount; ++i)
        if (ring_fixed_match(kRingFixedTab.e[i], p, nw, wm, wn, nks, lds, phases)) return i;
    return -1;
}

// conv_ring_fixed_{a,b,c}.hip: the instantiations, split three ways by ID % 3 so that they compile side by side
hipError_t ring_fixed_launch_a(int id, const ConvP& p, dim3 grid, size_t lds, hipStream_t st);
hipError_t ring_fixed_launch_b(int id, const ConvP& p, dim3 grid, size_t lds, hipStream_t st);
hipError_t ring_fixed_launch_c(int id, const ConvP& p, dim3 grid, size_t lds, hipStream_t st);

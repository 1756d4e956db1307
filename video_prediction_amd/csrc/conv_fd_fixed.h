// conv_fd_fixed.h -- the implicit-GEMM FPROP / DGRAD launcher's planning as constexpr code, and the table of FIXED problems built from it.
//
// conv_fd_kernel (conv_igemm.hip) serves whatever no problem-specific kernel takes.  In the train step that is a short list of problems that
// recur in every step -- the video discriminator's 4x4x4 ladder and its data gradients, the image discriminator's stride-2 data gradient,
// the dense data gradient of every generator time step -- and the kernel re-derives their geometry (output phase, taps, divisions by the
// grid extents, 64-bit strides) in every workgroup and every K-tile.  conv_fd_fixed_kernel<ID> is the SAME body (conv_fd_kernel.h) with
// those values folded: its argument block FdFixedP<ID> carries pointers, part / part_sz and the epilogue's scalars only.
//
//   * fd_pick_tile / fd_plan are the code savp_conv runs for every call; a table entry is fd_plan evaluated at compile time on one line of
//     the list below -- there is no second copy of the arithmetic to drift.
//   * savp_conv plans a call as always and then compares the planned ConvP field by field with the table (fd_fixed_find): only an exact
//     match of every folded value -- dims, both tensors' (dense) strides, kernel, stride, padding, tile, tile counts, split-K, the kernel
//     instantiation -- with 16-byte aligned bases launches the fixed instantiation; anything else takes conv_fd_kernel as before.  Option
//     "fd_fixed" 0 switches the routing off.
//   * beta / act / alpha / aux / bias stay arguments: the float epilogue is compiled from the same runtime switches in both kernels.
#pragma once
#include "conv_common.h"
#include <utility>

// ---- the planner of the generic FPROP / DGRAD path --------------------------------------------------------------------------------------
static constexpr inline void fd_pick_tile(long long M, long long N, int& wm, int& wn) {
    // cost model: rounds over the 256 CUs x tile area x a re-read penalty for small tiles
    const int opts[4][2] = {{2, 2}, {2, 1}, {1, 2}, {1, 1}};
    double best = 1e300;
    for (int i = 0; i < 4; ++i) {
        long long bm = 64 * opts[i][0], bn = 64 * opts[i][1];
        long long tm = (M + bm - 1) / bm, tn = (N + bn - 1) / bn;
        double wgs = (double)tm * tn;
        double rounds = wgs <= 256.0 ? 1.0 : wgs / 256.0;
        double eff = (bm * bn == 128 * 128) ? 1.0 : (bm * bn == 64 * 64 ? 1.3 : 1.12);
        double cost = rounds * (double)(bm * bn) * eff;
        if (cost < best) { best = cost; wm = opts[i][0]; wn = opts[i][1]; }
    }
}

// Tile, tile counts, output phases and the split count the call asks for (`splitk`: before splitk_fit cuts it to the caller's scratch;
// `dense`: the destination is one dense block, which split-K needs; part_sz: elements of that block).  wm = 0: the planner picks the tile.
struct FdPlan { int wm, wn, phases, splitk, tm, tn; long long Mmax, part_sz; bool dense; };

static constexpr inline void fd_plan(const SavpConvArgs* a, bool bf16, int wm, int wn, FdPlan& g) {
    const bool dg = a->mode == SAVP_CONV_DGRAD;
    const int Cred = dg ? a->Cy : a->Cx;
    const int Nout = dg ? a->Cx : a->Cy;
    long long Mmax = 0;
    int phases = 1;
    if (dg) {
        phases = a->sd * a->sh * a->sw;
        Mmax = (long long)a->N * ((a->D + a->sd - 1) / a->sd) * ((a->H + a->sh - 1) / a->sh) * ((a->W + a->sw - 1) / a->sw);
    } else {
        Mmax = (long long)a->N * a->Do * a->Ho * a->Wo;
    }
    if (!wm) fd_pick_tile(Mmax * phases, Nout, wm, wn);
    const int BM = 64 * wm, BN = 64 * wn;
    // split-K (plain epilogue only): fills the chip when M*N is small and K is long (8x8 / 16x16 ConvLSTM layers)
    int splitk = a->splitk;
    const long long tiles = ((Mmax + BM - 1) / BM) * ((Nout + BN - 1) / BN) * phases;
    const long long taps_max = (long long)a->kd * a->kh * a->kw / (dg ? phases : 1);
    const long long nkt = (taps_max * Cred + (bf16 ? 63 : 31)) / (bf16 ? 64 : 32);
    const bool can_split = (a->act == SAVP_ACT_NONE);
    if (!can_split) splitk = 1;
    else if (splitk <= 0) {
        splitk = 1;
        if (tiles <= 192 && nkt >= 16) {
            long long s1 = 512 / tiles, s2 = nkt / 8;
            splitk = (int)(s1 < s2 ? s1 : s2);
            if (splitk < 1) splitk = 1;
            if (splitk > 16) splitk = 16;
        }
    }
    g.dense = false; g.part_sz = 0;
    if (splitk > 1) {
        // the destination must be one dense block: split s stores its share at the same offsets of its slice of the scratch
        const long long dD = dg ? a->D : a->Do, dH = dg ? a->H : a->Ho, dW_ = dg ? a->W : a->Wo;
        const long long s_n = dg ? a->x_sn : a->y_sn, s_d = dg ? a->x_sd : a->y_sd, s_h = dg ? a->x_sh : a->y_sh,
                        s_w = dg ? a->x_sw : a->y_sw;
        g.dense = (s_w == Nout) && (s_h == dW_ * Nout) && (dD == 1 || s_d == dH * dW_ * Nout) && (s_n == dD * dH * dW_ * Nout);
        if (!g.dense) splitk = 1;
        else g.part_sz = (long long)a->N * dD * dH * dW_ * Nout;
    }
    g.wm = wm; g.wn = wn; g.phases = phases; g.splitk = splitk; g.Mmax = Mmax;
    g.tm = (int)((Mmax + BM - 1) / BM); g.tn = (int)((Nout + BN - 1) / BN);
}

// ---- the fixed problems ------------------------------------------------------------------------------------------------------------------
// One line per (problem, mode) that the default BAIR train step (64 x 64 x 3, batch 16, sequence 30, bf16 datapath, shipped tuning table)
// launches on conv_fd_kernel in every step (tests/tools/fd_problems.py lists them from a step run on a -DSAVP_FD_LOG build), and a few
// small probe problems that only tests/test_gpu_fd_fixed.py calls.  Nothing depends on this list being right or complete: a line that no
// call matches is never launched, a call that matches no line takes the generic kernel.
enum { FD_VEC = 1, FD_BF16 = 2, FD_WB16 = 4 };         // conv_fd_kernel's VEC / BF16 / WB16 template switches
struct FdFixedDesc {
    int mode, N, D, H, W, Cx, Do, Ho, Wo, Cy;
    int kd, kh, kw, sd, sh, sw, pd, ph, pw;
    int wm, wn, splitk, flags;                         // as planned: wave tile, K splits (after the scratch fit), instantiation
    int rank;                                          // how the call site views both tensors: 5 = dense [N][D][H][W][C]; 4 = [N][H][W][C] (depth stride 0); 2 = [N][C] (all spatial strides 0)
};
#define FD_K444 4, 4, 4
#define FD_VB (FD_VEC | FD_BF16)
#define FD_VBW (FD_VEC | FD_BF16 | FD_WB16)
static constexpr FdFixedDesc kFdFixed[] = {
    // ---- the step's problems, in the order of their first launch (N = 32: real + generated clips together; 16: one of them; 464 = 16 x 29
    // frames of the image discriminator) ----
    // video discriminator, 4x4x4 ladder: forward (bias + leaky ReLU) ...
    {SAVP_CONV_FPROP, 32, 10, 64, 64, 32, 9, 32, 32, 64,  FD_K444, 1, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    {SAVP_CONV_FPROP, 32, 9, 32, 32, 64, 8, 16, 16, 128,  FD_K444, 1, 2, 2, 1, 1, 1,  2, 2, 1, FD_VBW, 5},
    {SAVP_CONV_FPROP, 32, 8, 16, 16, 128, 4, 8, 8, 256,  FD_K444, 2, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    {SAVP_CONV_FPROP, 16, 10, 64, 64, 32, 9, 32, 32, 64,  FD_K444, 1, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    {SAVP_CONV_FPROP, 16, 8, 16, 16, 128, 4, 8, 8, 256,  FD_K444, 2, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    // ... and data gradients (through the leaky ReLU of the layer below)
    {SAVP_CONV_DGRAD, 32, 8, 16, 16, 128, 4, 8, 8, 256,  FD_K444, 2, 2, 2, 1, 1, 1,  2, 2, 1, FD_VBW, 5},
    {SAVP_CONV_DGRAD, 32, 9, 32, 32, 64, 8, 16, 16, 128,  FD_K444, 1, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    {SAVP_CONV_DGRAD, 16, 8, 16, 16, 128, 4, 8, 8, 256,  FD_K444, 2, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    {SAVP_CONV_DGRAD, 16, 9, 32, 32, 64, 8, 16, 16, 128,  FD_K444, 1, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    // image discriminator: the 4x4 stride-2 data gradient.  (Its first layer, 464 x 64 x 64 x 6 -> 32 x 32 x 64 on the scalar path, recurs too
    // but was 15 % SLOWER with its geometry folded, 131 against 114 us, and stays on conv_fd_kernel: profiles/fd_fixed.md)
    {SAVP_CONV_DGRAD, 464, 1, 32, 32, 64, 1, 16, 16, 128,  1, 4, 4, 1, 2, 2, 0, 1, 1,  1, 1, 1, FD_VBW, 4},
    // dense layers as 1x1x1 convolutions over [N][C] matrices: the data gradient of every generator time step (8192 <- 100), the
    // discriminators' heads and their data gradients (one reduction channel: the scalar path)
    {SAVP_CONV_DGRAD, 32, 1, 1, 1, 8192, 1, 1, 1, 100,  1, 1, 1, 1, 1, 1, 0, 0, 0,  1, 1, 1, FD_VB, 2},
    {SAVP_CONV_FPROP, 464, 1, 1, 1, 256, 1, 1, 1, 8,  1, 1, 1, 1, 1, 1, 0, 0, 0,  1, 1, 1, FD_VBW, 2},
    {SAVP_CONV_DGRAD, 464, 1, 1, 1, 256, 1, 1, 1, 8,  1, 1, 1, 1, 1, 1, 0, 0, 0,  1, 1, 1, FD_VBW, 2},
    {SAVP_CONV_DGRAD, 32, 1, 1, 1, 65536, 1, 1, 1, 1,  1, 1, 1, 1, 1, 1, 0, 0, 0,  1, 1, 1, FD_BF16, 2},
    {SAVP_CONV_DGRAD, 16, 1, 1, 1, 65536, 1, 1, 1, 1,  1, 1, 1, 1, 1, 1, 0, 0, 0,  1, 2, 1, FD_BF16, 2},
    // ---- probe problems of tests/test_gpu_fd_fixed.py (no call site has these shapes): 4x4x4 stride (1,2,2) / (2,2,2), forward and data
    // gradient (odd H: output phases of different extents, one of them without a second row tile), Nout = 72, M = 36, split-K 2, and a
    // dense data gradient over 100 channels (the K tail inside the last K-tile)
    {SAVP_CONV_FPROP, 2, 3, 6, 6, 8, 2, 3, 3, 72,  FD_K444, 1, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    {SAVP_CONV_FPROP, 2, 3, 6, 6, 8, 1, 3, 3, 72,  FD_K444, 2, 2, 2, 1, 1, 1,  1, 1, 2, FD_VB, 5},
    {SAVP_CONV_DGRAD, 2, 3, 7, 6, 8, 2, 3, 3, 72,  FD_K444, 1, 2, 2, 1, 1, 1,  1, 1, 1, FD_VBW, 5},
    {SAVP_CONV_DGRAD, 3, 3, 7, 6, 8, 1, 3, 3, 72,  FD_K444, 2, 2, 2, 1, 1, 1,  1, 1, 2, FD_VBW, 5},
    {SAVP_CONV_DGRAD, 3, 1, 1, 1, 72, 1, 1, 1, 100,  1, 1, 1, 1, 1, 1, 0, 0, 0,  1, 1, 2, FD_VB, 5},
};
#undef FD_K444
#undef FD_VB
#undef FD_VBW
static constexpr int kFdFixedCount = (int)(sizeof(kFdFixed) / sizeof(kFdFixed[0]));

// the call a table line stands for: dense tensors, the tile and the split count given explicitly
static constexpr inline SavpConvArgs fd_fixed_args(const FdFixedDesc& d) {
    SavpConvArgs a{};
    a.mode = d.mode; a.N = d.N; a.D = d.D; a.H = d.H; a.W = d.W; a.Cx = d.Cx; a.Do = d.Do; a.Ho = d.Ho; a.Wo = d.Wo; a.Cy = d.Cy;
    a.kd = d.kd; a.kh = d.kh; a.kw = d.kw; a.sd = d.sd; a.sh = d.sh; a.sw = d.sw; a.pd = d.pd; a.ph = d.ph; a.pw = d.pw;
    a.splitk = d.splitk; a.tile = (d.wm << 4) | d.wn;
    a.precision = (d.flags & FD_BF16) ? SAVP_PREC_BF16 : SAVP_PREC_F32;
    a.x_sw = d.Cx; a.x_sh = a.x_sw * d.W; a.x_sd = a.x_sh * d.H; a.x_sn = a.x_sd * d.D;
    a.y_sw = d.Cy; a.y_sh = a.y_sw * d.Wo; a.y_sd = a.y_sh * d.Ho; a.y_sn = a.y_sd * d.Do;
    if (d.rank <= 4) a.x_sd = a.y_sd = 0;
    if (d.rank == 2) a.x_sh = a.x_sw = a.y_sh = a.y_sw = 0;
    return a;
}

// the ConvP fields savp_conv copies from the call and the ones the plan decides (geometry only; pointers and epilogue scalars are not folded)
static constexpr inline void fd_geometry_fields(ConvP& p, const SavpConvArgs* a, const FdPlan& g) {
    p.mode = a->mode;
    p.N = a->N; p.D = a->D; p.H = a->H; p.W = a->W; p.Cx = a->Cx;
    p.Do = a->Do; p.Ho = a->Ho; p.Wo = a->Wo; p.Cy = a->Cy;
    p.kd = a->kd; p.kh = a->kh; p.kw = a->kw; p.sd = a->sd; p.sh = a->sh; p.sw = a->sw;
    p.pd = a->pd; p.ph = a->ph; p.pw = a->pw;
    p.x_sn = a->x_sn; p.x_sd = a->x_sd; p.x_sh = a->x_sh; p.x_sw = a->x_sw;
    p.y_sn = a->y_sn; p.y_sd = a->y_sd; p.y_sh = a->y_sh; p.y_sw = a->y_sw;
    p.splitk = g.splitk; p.tm = g.tm; p.tn = g.tn;
}

// A table entry: the ConvP that savp_conv plans for the line.  ok: the planner keeps the line's tile and split count (a line whose split
// count the planner would refuse, or with more splits than K-tiles allow a dense destination for, matches no call and is a mistake)
struct FdFixedEntry { ConvP p; int wm, wn, flags, phases; bool ok; };

static constexpr inline FdFixedEntry fd_fixed_entry(int id) {
    const FdFixedDesc& d = kFdFixed[id];
    const SavpConvArgs a = fd_fixed_args(d);
    FdFixedEntry e{};
    FdPlan g{};
    fd_plan(&a, (d.flags & FD_BF16) != 0, d.wm, d.wn, g);
    fd_geometry_fields(e.p, &a, g);
    e.p.bf16 = (d.flags & FD_BF16) ? 1 : 0;
    e.wm = g.wm; e.wn = g.wn; e.flags = d.flags; e.phases = g.phases;
    const int Cred = d.mode == SAVP_CONV_DGRAD ? d.Cy : d.Cx;
    e.ok = (d.mode == SAVP_CONV_FPROP || d.mode == SAVP_CONV_DGRAD) && g.wm == d.wm && g.wn == d.wn && g.splitk == d.splitk && d.splitk >= 1 &&
           g.Mmax > 0 && (!(d.flags & FD_VEC) || Cred % 4 == 0) && (!(d.flags & FD_WB16) || ((d.flags & FD_VEC) && (d.flags & FD_BF16) && Cred % 8 == 0)) &&
           d.kd <= 8 && d.kh <= 8 && d.kw <= 8 && (d.rank == 5 || (d.rank == 4 && d.D == 1 && d.Do == 1) ||
           (d.rank == 2 && d.D * d.H * d.W == 1 && d.Do * d.Ho * d.Wo == 1));
    return e;
}

template <size_t... I>
static constexpr auto fd_fixed_entries(std::index_sequence<I...>) {
    struct Tab { FdFixedEntry e[sizeof...(I)]; };
    return Tab{{fd_fixed_entry((int)I)...}};
}
static constexpr auto kFdFixedTab = fd_fixed_entries(std::make_index_sequence<kFdFixedCount>{});

// ---- argument block of conv_fd_fixed_kernel<ID>: ConvP's names, the geometry as compile-time constants -----------------------------------
#define FD_FIXED_FIELDS(F)                                                                                                               \
    F(int, mode) F(int, N) F(int, D) F(int, H) F(int, W) F(int, Cx) F(int, Do) F(int, Ho) F(int, Wo) F(int, Cy)                             \
    F(int, kd) F(int, kh) F(int, kw) F(int, sd) F(int, sh) F(int, sw) F(int, pd) F(int, ph) F(int, pw)                                      \
    F(int, splitk) F(int, tm) F(int, tn) F(int, bf16)                                                                                      \
    F(long long, x_sn) F(long long, x_sd) F(long long, x_sh) F(long long, x_sw) F(long long, y_sn) F(long long, y_sd) F(long long, y_sh) F(long long, y_sw)

template <int ID>
struct FdFixedP {
    static constexpr FdFixedEntry E = kFdFixedTab.e[ID];
#define F(T, f) static constexpr T f = E.p.f;
    FD_FIXED_FIELDS(F)
#undef F
    // the gather of the fixed body counts elements in 32 bits: both (dense) tensors and the packed weights must fit
    static_assert((long long)N * x_sn <= 0x7fffffffLL, "x-side tensor exceeds 32-bit element offsets");
    static_assert((long long)N * y_sn <= 0x7fffffffLL, "y-side tensor exceeds 32-bit element offsets");
    static_assert((long long)Cx * Cy * kd * kh * kw <= 0x7fffffffLL, "packed weights exceed 32-bit element offsets");
    // ---- what a call decides ----
    int beta, act;
    float alpha;
    const float* x;
    const float* y;
    const float* w;
    const unsigned short* w16;
    float* out;
    const float* bias;
    const float* aux;
    float* part; long long part_sz;
};

template <class Q>
static inline void fd_fixed_call_args(Q& q, const ConvP& p) {
    q.beta = p.beta; q.act = p.act; q.alpha = p.alpha;
    q.x = p.x; q.y = p.y; q.w = p.w; q.w16 = p.w16; q.out = p.out; q.bias = p.bias; q.aux = p.aux; q.part = p.part; q.part_sz = p.part_sz;
}

// The planned call against one entry: EVERY folded value (the tensors' strides among them), the tile and the instantiation; the fixed
// kernels are offered 16-byte aligned tensors only.  (Pointers and the epilogue's scalars are arguments of both kernels and not compared.)
static inline bool fd_fixed_match(const FdFixedEntry& e, const ConvP& p, int wm, int wn, int flags, int phases) {
    if (!aligned16(p.x) || !aligned16(p.y) || !aligned16(p.w) || ((flags & FD_WB16) && !aligned16(p.w16))) return false;
    if (!e.ok || e.wm != wm || e.wn != wn || e.flags != flags || e.phases != phases) return false;
    if (p.splitk > 1 && (!p.part || !aligned16(p.part))) return false;
#define F(T, f) if (e.p.f != p.f) return false;
    FD_FIXED_FIELDS(F)
#undef F
    return true;
}

// index of the entry the planned call matches, or -1
static inline int fd_fixed_find(const ConvP& p, int wm, int wn, int flags, int phases) {
    for (int i = 0; i < kFdFixedCount; ++i)
        if (fd_fixed_match(kFdFixedTab.e[i], p, wm, wn, flags, phases)) return i;
    return -1;
}

// conv_fd_fixed_{a,b}.hip: the instantiations, split by ID % 2 so that they compile side by side
hipError_t fd_fixed_launch_a(int id, const ConvP& p, dim3 grid, hipStream_t st);
hipError_t fd_fixed_launch_b(int id, const ConvP& p, dim3 grid, hipStream_t st);
// the constants FdFixedP<id> folds, in FD_FIXED_FIELDS order (count, or -1)
int fd_fixed_folded_a(int id, long long* out, int n);
int fd_fixed_folded_b(int id, long long* out, int n);

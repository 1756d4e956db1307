// conv_fd_fixed_inst.h -- conv_fd_fixed_kernel<ID> and its launcher; included by conv_fd_fixed_{a,b}.hip, each of which instantiates the
// table entries with ID % 2 == its residue.
#pragma once
#include "conv_fd_kernel.h"
#include "conv_fd_fixed.h"

template <int ID> struct FdIsFixed<FdFixedP<ID>> { static constexpr bool value = true; };

template <int ID>
__global__ __launch_bounds__(NTHREADS) void conv_fd_fixed_kernel(FdFixedP<ID> p) {
    constexpr FdFixedEntry E = FdFixedP<ID>::E;
    static_assert(E.ok, "a fixed implicit-GEMM problem is not planned as its table line says");
    conv_fd_body<E.wm, E.wn, (E.flags & FD_VEC) != 0, (E.flags & FD_BF16) != 0, (E.flags & FD_WB16) != 0>(p);
}

template <int ID>
static hipError_t launch_fd_fixed(const ConvP& p, dim3 grid, hipStream_t st) {
    constexpr FdFixedEntry E = FdFixedP<ID>::E;
    // the same LDS footprint as launch_fd1 (conv_igemm.hip)
    constexpr int BKT = (E.flags & FD_BF16) ? 64 : 32;
    constexpr size_t rowb = (E.flags & FD_BF16) ? (BKT + 8) * 2 : BKP * 4;
    size_t lds = (size_t)2 * (64 * E.wm + 64 * E.wn) * rowb;
    if (lds < (size_t)64 * E.wm * sizeof(long long)) lds = (size_t)64 * E.wm * sizeof(long long);
    static bool attr_done = false;
    if (!attr_done) {
        hipFuncSetAttribute((const void*)conv_fd_fixed_kernel<ID>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_done = true;
    }
    FdFixedP<ID> q;
    fd_fixed_call_args(q, p);
    hipLaunchKernelGGL((conv_fd_fixed_kernel<ID>), grid, dim3(NTHREADS), lds, st, q);
    return hipGetLastError();
}

template <int R, int I = R>
static hipError_t fd_fixed_dispatch(int id, const ConvP& p, dim3 grid, hipStream_t st) {
    if constexpr (I < kFdFixedCount) {
        if (id == I) return launch_fd_fixed<I>(p, grid, st);
        return fd_fixed_dispatch<R, I + 2>(id, p, grid, st);
    } else {
        return hipErrorInvalidValue;
    }
}

// the constants FdFixedP<id> folds, in FD_FIXED_FIELDS order (savp_fd_fixed_probe: the host test compares them with a planner run)
template <int R, int I = R>
static int fd_fixed_folded(int id, long long* out, int n) {
    if constexpr (I < kFdFixedCount) {
        if (id != I) return fd_fixed_folded<R, I + 2>(id, out, n);
        int k = 0;
#define F(T, f) if (k < n) out[k] = (long long)FdFixedP<I>::f; ++k;
        FD_FIXED_FIELDS(F)
#undef F
        return k;
    } else {
        return -1;
    }
}

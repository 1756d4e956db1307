// conv_ring_fixed_inst.h -- conv_ring_fixed_kernel<ID> and its launcher; included by conv_ring_fixed_{a,b,c}.hip, each of which instantiates
// the table entries with ID % 3 == its residue.
#pragma once
#include "conv_ring_kernel.h"
#include "conv_ring_fixed.h"
#include <hip/hip_ext.h>

template <int ID>
__global__ __launch_bounds__(64 * RingFixedP<ID>::E.nw, (ring_min_waves<RingFixedP<ID>::E.nw, RingFixedP<ID>::E.wm, RingFixedP<ID>::E.wn, RingFixedP<ID>::E.nks>()))
void conv_ring_fixed_kernel(RingFixedP<ID> p) {
    constexpr RingFixedEntry E = RingFixedP<ID>::E;
    static_assert(E.ok, "a fixed ring problem has no tiling");
    conv_ring_body<E.nw, E.wm, E.wn, E.nks>(p);
}

template <int ID>
static hipError_t launch_ring_fixed(const ConvP& p, dim3 grid, size_t lds, hipStream_t st) {
    static size_t attr_lds = 0;
    if (lds > attr_lds) {
        hipFuncSetAttribute((const void*)conv_ring_fixed_kernel<ID>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_lds = lds;
    }
    RingFixedP<ID> q;
    ring_fixed_args(q, p);
    constexpr int NT = 64 * RingFixedP<ID>::E.nw;
    if (g_savp_prof_start) {                                     // bench.py: kernel-only timing of this one launch (common.hip)
        hipExtLaunchKernelGGL((conv_ring_fixed_kernel<ID>), grid, dim3(NT), lds, st, g_savp_prof_start, g_savp_prof_stop, 0, q);
        g_savp_prof_start = g_savp_prof_stop = nullptr;
    } else {
        hipLaunchKernelGGL((conv_ring_fixed_kernel<ID>), grid, dim3(NT), lds, st, q);
    }
    return hipGetLastError();
}

template <int R, int I = R>
static hipError_t ring_fixed_dispatch(int id, const ConvP& p, dim3 grid, size_t lds, hipStream_t st) {
    if constexpr (I < kRingFixedCount) {
        if (id == I) return launch_ring_fixed<I>(p, grid, lds, st);
        return ring_fixed_dispatch<R, I + 3>(id, p, grid, lds, st);
    } else {
        return hipErrorInvalidValue;
    }
}

// health.hip -- the opt-in guard of a long training run: what is in an optimiser group's gradient arena, and an Adam that acts on it.
//
//   savp_arena_health : per-variable sum of squares (float64, finite elements only) and count of non-finite elements (NaN, +Inf, -Inf) of
//                       one flat fp32 arena, their totals, the flag `ok` = (no non-finite element) and three counters kept on the device.
//                       Two launches:
//                         items pass : one workgroup per work-list item (segment, start, count <= HL_CHUNK floats of one variable).  A
//                                      thread loads its <= HL_V4 float4 of the item before it adds anything, so a wave has all its 16-byte
//                                      requests in flight at once; the 1..3 floats behind the last whole float4 are a scalar tail.  The
//                                      square of an fp32 is exact in float64.  The workgroup's (sum, count) is folded in a fixed order
//                                      (lanes by a shuffle tree, waves in order) and STORED to ws[item].
//                         fold pass  : ONE workgroup.  A thread per segment adds the segment's items in list order; thread 0 then adds
//                                      the segments in order and writes the totals, `ok` and the counters.
//                       No atomics, no completion counter, nothing to clear, no allocation: equal input gives equal bits, and both
//                       launches are plain kernel nodes of a captured step.
//   savp_adam_guarded : savp_adam (util_ops.hip) behind that flag: *ok == 0 -> no thread stores anything; otherwise the very same
//                       update (adam_update.h holds the arithmetic for both).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "savp_hip.h"
#include "adam_update.h"

#define NT 256
#define HL_V4 8                               // float4 loads per thread and item
#define HL_CHUNK (NT * HL_V4 * 4)             // floats per work-list item at the most: 8192 (32 KiB)
#define HL_STAGE 3072                         // the fold pass keeps up to this many item partials in LDS (48 KiB with their segment indices)
#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? SAVP_OK : SAVP_ELAUNCH)

namespace {

struct HealthPartial {                        // ws[item]: 16 bytes, written whole
    double sumsq;
    int32_t nonfinite;
    int32_t pad;
};

__device__ __forceinline__ bool finite_bits(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void take(float f, double& s, int& c) {
    if (finite_bits(f)) {
        const double d = (double)f;
        s += d * d;
    } else {
        ++c;
    }
}

__global__ __launch_bounds__(NT) void health_items_kernel(const float* __restrict__ x, int64_t n, const int64_t* __restrict__ seg, int S,
                                                          const int64_t* __restrict__ items, HealthPartial* __restrict__ ws) {
    __shared__ double sh_s[NT / 64];
    __shared__ int sh_c[NT / 64];
    const int64_t* it = items + 3 * (int64_t)blockIdx.x;
    const int64_t sg = it[0], start = it[1];
    int64_t count = it[2];
    // whatever the list says, nothing outside the arena is read and nothing past what one workgroup covers
    const bool listed = sg >= 0 && sg < S && start >= 0;
    const int64_t at = listed ? seg[2 * sg] + start : 0;           // segment offsets and item starts are multiples of 4 floats
    if (!listed || at < 0 || (at & 3) || at >= n) count = 0;
    if (count > HL_CHUNK) count = HL_CHUNK;
    if (count > n - at) count = n - at;
    if (count < 0) count = 0;
    const float* base = x + at;
    const int n4 = (int)(count >> 2), tail = (int)(count & 3);
    const int t = threadIdx.x;
    float4 v[HL_V4];
#pragma unroll
    for (int k = 0; k < HL_V4; ++k) {
        const int i = t + k * NT;
        v[k] = i < n4 ? reinterpret_cast<const float4*>(base)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float last = t < tail ? base[4 * n4 + t] : 0.f;
    double s = 0.0;
    int c = 0;
#pragma unroll
    for (int k = 0; k < HL_V4; ++k) {
        take(v[k].x, s, c);
        take(v[k].y, s, c);
        take(v[k].z, s, c);
        take(v[k].w, s, c);
    }
    take(last, s, c);
    // lanes: a shuffle tree of fixed shape; waves: in order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_down(s, d, 64);
        c += __shfl_down(c, d, 64);
    }
    if ((t & 63) == 0) {
        sh_s[t >> 6] = s;
        sh_c[t >> 6] = c;
    }
    __syncthreads();
    if (t == 0) {
        HealthPartial o;
        o.sumsq = 0.0;
        o.nonfinite = 0;
        o.pad = 0;
        for (int w = 0; w < NT / 64; ++w) {
            o.sumsq += sh_s[w];
            o.nonfinite += sh_c[w];
        }
        ws[blockIdx.x] = o;
    }
}

// first item of the list whose segment index is >= s (the list is in segment order); `seg_of` reads item i's segment index
template <typename SegOf>
__device__ __forceinline__ int first_item_of(SegOf seg_of, int n_items, int64_t s) {
    int lo = 0, hi = n_items;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_of(mid) < s) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(NT) void health_fold_kernel(const int64_t* __restrict__ items, int n_items, int S,
                                                         const HealthPartial* __restrict__ ws, double* sumsq, int32_t* nonfinite,
                                                         double* __restrict__ total_sumsq,
                                                         int32_t* __restrict__ total_nonfinite, int32_t* __restrict__ ok,
                                                         int32_t* __restrict__ counters) {
    // A list of up to HL_STAGE items (every arena of the shipped models) is brought into LDS by the whole workgroup first: the searches and
    // the in-order adds below are chains of dependent reads, a microsecond each from global memory
    __shared__ double st_s[HL_STAGE];
    __shared__ int st_c[HL_STAGE];
    __shared__ int st_seg[HL_STAGE];
    const bool staged = n_items <= HL_STAGE;
    if (staged) {
        for (int i = threadIdx.x; i < n_items; i += NT) {
            const HealthPartial p = ws[i];
            st_s[i] = p.sumsq;
            st_c[i] = p.nonfinite;
            st_seg[i] = (int)items[3 * (int64_t)i];
        }
        __syncthreads();
    }
    for (int s = threadIdx.x; s < S; s += NT) {
        double a = 0.0;
        int c = 0;
        if (staged) {
            auto seg_of = [&](int i) { return (int64_t)st_seg[i]; };
            const int i0 = first_item_of(seg_of, n_items, s), i1 = first_item_of(seg_of, n_items, (int64_t)s + 1);
#pragma unroll 8
            for (int i = i0; i < i1; ++i) {
                a += st_s[i];
                c += st_c[i];
            }
        } else {
            auto seg_of = [&](int i) { return items[3 * (int64_t)i]; };
            const int i0 = first_item_of(seg_of, n_items, s), i1 = first_item_of(seg_of, n_items, (int64_t)s + 1);
#pragma unroll 4
            for (int i = i0; i < i1; ++i) {
                const HealthPartial p = ws[i];
                a += p.sumsq;
                c += p.nonfinite;
            }
        }
        sumsq[s] = a;
        nonfinite[s] = c;
    }
    __syncthreads();                                               // the block's own global stores are visible to thread 0 behind it
    if (threadIdx.x == 0) {
        double a = 0.0;
        int c = 0, bad = -1;
        for (int s = 0; s < S; ++s) {
            a += sumsq[s];
            const int cs = nonfinite[s];
            c += cs;
            if (cs && bad < 0) bad = s;
        }
        *total_sumsq = a;
        *total_nonfinite = c;
        *ok = c == 0 ? 1 : 0;
        if (c == 0) {
            counters[1] = 0;
        } else {
            counters[0] += 1;
            counters[1] += 1;
        }
        counters[2] = bad;
    }
}

__global__ void adam_guarded_kernel(long long n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                    float* __restrict__ v, float lr_host, float b1, float b2, float eps, float gscale, const float* lr_dev,
                                    const int32_t* __restrict__ ok) {
    if (*ok == 0) return;                                          // uniform over the grid: every thread leaves, nothing is stored
    savp_adam_update(n, p, g, m, v, lr_host, b1, b2, eps, gscale, lr_dev, blockIdx.x * (long long)blockDim.x + threadIdx.x,
                     (long long)gridDim.x * blockDim.x);
}

}  // namespace

extern "C" int32_t savp_arena_health_chunk(void) { return HL_CHUNK; }

extern "C" int64_t savp_arena_health_ws_bytes(int64_t n_items) {
    return n_items < 1 ? 0 : n_items * (int64_t)sizeof(HealthPartial);
}

extern "C" int savp_arena_health(void* stream, const SavpHealthArgs* a) {
    if (!a || !a->x || !a->segments || !a->items || !a->sumsq || !a->nonfinite || !a->total_sumsq || !a->total_nonfinite || !a->ok ||
        !a->counters || !a->ws)
        return SAVP_EINVAL;
    if (a->S < 1 || a->n_items < 1 || a->n < 1 || a->S > INT32_MAX || a->n_items > INT32_MAX) return SAVP_EINVAL;
    if ((((uintptr_t)a->x | (uintptr_t)a->ws) & 15) != 0) return SAVP_EINVAL;
    if ((((uintptr_t)a->segments | (uintptr_t)a->items | (uintptr_t)a->sumsq | (uintptr_t)a->total_sumsq) & 7) != 0) return SAVP_EINVAL;
    if (a->ws_bytes < savp_arena_health_ws_bytes(a->n_items)) return SAVP_EINVAL;
    hipLaunchKernelGGL(health_items_kernel, dim3((unsigned)a->n_items), dim3(NT), 0, (hipStream_t)stream, a->x, a->n, a->segments, (int)a->S,
                       a->items, (HealthPartial*)a->ws);
    if (hipGetLastError() != hipSuccess) return SAVP_ELAUNCH;
    hipLaunchKernelGGL(health_fold_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, a->items, (int)a->n_items, (int)a->S,
                       (const HealthPartial*)a->ws, a->sumsq, a->nonfinite, a->total_sumsq, a->total_nonfinite, a->ok, a->counters);
    return LAUNCH_OK();
}

extern "C" int savp_adam_guarded(void* stream, int64_t n, float* p, const float* g, float* m, float* v, float lr_t, float beta1,
                                 float beta2, float eps, float gscale, const float* lr_t_dev, const int32_t* ok) {
    if (!p || !g || !m || !v || !ok || n < 1) return SAVP_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0 || ((uintptr_t)ok & 3) != 0) return SAVP_EINVAL;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3(savp_adam_blocks(n)), dim3(SAVP_ADAM_NT), 0, (hipStream_t)stream, (long long)n, p, g, m,
                       v, lr_t, beta1, beta2, eps, gscale, lr_t_dev, ok);
    return LAUNCH_OK();
}

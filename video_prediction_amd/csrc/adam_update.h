// adam_update.h -- the arithmetic of tf.train.AdamOptimizer on a flat arena, shared by savp_adam (util_ops.hip) and savp_adam_guarded
// (health.hip) so that the two cannot drift apart: one grid-stride walk, float4 body and scalar tail.
// TF Adam: lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is computed on the host and passed in;
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2 ; p -= lr_t * m / (sqrt(v) + eps)       (epsilon outside the sqrt)
// gscale multiplies the gradient first (1/world_size after a sum all-reduce).
#pragma once
#include <hip/hip_runtime.h>

#define SAVP_ADAM_NT 256

// workgroups of an Adam launch over n floats, as savp_adam sizes its own (the result does not depend on it)
static inline unsigned savp_adam_blocks(long long n) {
    long long b = (n / 4 + 1 + SAVP_ADAM_NT - 1) / SAVP_ADAM_NT;
    if (b < 1) b = 1;
    if (b > 4096) b = 4096;
    return (unsigned)b;
}

__device__ __forceinline__ void savp_adam_update(long long n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, float lr_host, float b1, float b2, float eps, float gscale,
                                                 const float* lr_dev, long long first, long long stride) {
    // first, stride: this thread's global index and the grid's thread count, taken by the KERNEL (read there, blockDim / gridDim compile to
    // the uniform-workgroup form a __global__ function is entitled to)
    const float lr_t = lr_dev ? *lr_dev : lr_host;
    long long n4 = n / 4;
    for (long long i = first; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
#define ADAM1(f)                                       \
    {                                                  \
        float gr = gg.f * gscale;                      \
        mm.f = b1 * mm.f + (1.f - b1) * gr;            \
        vv.f = b2 * vv.f + (1.f - b2) * gr * gr;       \
        pp.f -= lr_t * mm.f / (sqrtf(vv.f) + eps);     \
    }
        ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
    for (long long i = n4 * 4 + first; i < n; i += stride) {
        float gr = g[i] * gscale;
        float mi = b1 * m[i] + (1.f - b1) * gr;
        float vi = b2 * v[i] + (1.f - b2) * gr * gr;
        m[i] = mi; v[i] = vi;
        p[i] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}

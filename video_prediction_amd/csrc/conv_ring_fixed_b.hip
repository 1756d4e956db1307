// conv_ring_fixed_b.hip -- the fixed ring problems with ID % 3 == 1 (conv_ring_fixed.h)
#include "conv_ring_fixed_inst.h"

hipError_t ring_fixed_launch_b(int id, const ConvP& p, dim3 grid, size_t lds, hipStream_t st) {
    return ring_fixed_dispatch<1>(id, p, grid, lds, st);
}

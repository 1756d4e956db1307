// conv_ring_fixed_c.hip -- the fixed ring problems with ID % 3 == 2 (conv_ring_fixed.h)
#include "conv_ring_fixed_inst.h"

hipError_t ring_fixed_launch_c(int id, const ConvP& p, dim3 grid, size_t lds, hipStream_t st) {
    return ring_fixed_dispatch<2>(id, p, grid, lds, st);
}

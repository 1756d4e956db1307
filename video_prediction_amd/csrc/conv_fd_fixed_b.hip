// conv_fd_fixed_b.hip -- the fixed implicit-GEMM problems with ID % 2 == 1 (conv_fd_fixed.h)
#include "conv_fd_fixed_inst.h"

hipError_t fd_fixed_launch_b(int id, const ConvP& p, dim3 grid, hipStream_t st) {
    return fd_fixed_dispatch<1>(id, p, grid, st);
}
int fd_fixed_folded_b(int id, long long* out, int n) { return fd_fixed_folded<1>(id, out, n); }

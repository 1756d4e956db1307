// conv_fd_fixed_a.hip -- the fixed implicit-GEMM problems with ID % 2 == 0 (conv_fd_fixed.h)
#include "conv_fd_fixed_inst.h"

hipError_t fd_fixed_launch_a(int id, const ConvP& p, dim3 grid, hipStream_t st) {
    return fd_fixed_dispatch<0>(id, p, grid, st);
}
int fd_fixed_folded_a(int id, long long* out, int n) { return fd_fixed_folded<0>(id, out, n); }

#!/bin/bash
# developer build: video_prediction_amd/ab/libsavp_hip_fdlog.so = the shipped objects with csrc/conv_igemm.hip recompiled under
# -DSAVP_FD_LOG (one line per conv_fd_kernel launch on stderr; tests/tools/fd_problems.py)
cd "$(dirname "$0")/../../video_prediction_amd/csrc" || exit 1
mkdir -p ../ab
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include -Wno-unused-value -DSAVP_FD_LOG -c conv_igemm.hip -o /tmp/conv_igemm_fdlog.o || exit 1
objs=$(ls build/*.o | grep -v conv_igemm.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../ab/libsavp_hip_fdlog.so $objs /tmp/conv_igemm_fdlog.o -ldl

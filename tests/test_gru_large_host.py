"""Host side of the large-plane instance-norm ConvGRU blocks (csrc/gru_two_pass.hip), no GPU: the chunk and workspace arithmetic kernels.py
restates against the library's own, the ctypes mirror of SavpGruLargeArgs against the header, the entries' refusals that need no launch,
and the generator's per-layer choice between the one-workgroup and the chunked blocks as a function of the frame size."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('savp_convgru_large_gates_fwd', 'savp_convgru_large_out_fwd', 'savp_convgru_large_out_bwd', 'savp_convgru_large_gates_bwd')


def test_chunk_and_workspace_arithmetic(hip_lib):
    from video_prediction_amd import kernels as K
    # (N, HW) -> pixels per workgroup: ceil(N * HW / 512) clamped to [32, 256], then raised until a plane has at most 64 chunks
    want = {(32, 4800): 256, (32, 1200): 75, (2, 1280): 32, (1, 4800): 75, (2, 2304): 36, (1, 1): 32, (1, 1025): 32, (4, 2049): 33,
            (1, 1 << 20): 16384, (64, 1 << 14): 256}
    for (N, HW), c in want.items():
        assert K.convgru_large_chunk(N, HW) == c == hip_lib.savp_convgru_large_chunk(N, HW), (N, HW)
    assert K.convgru_large_chunk(0, 16) == K.convgru_large_chunk(2, 0) == 0 == hip_lib.savp_convgru_large_chunk(0, 16)
    # float64 [N, chunks, 4, F]
    assert K.convgru_large_ws_bytes(32, 4800, 32) == 32 * 19 * 4 * 32 * 8 == hip_lib.savp_convgru_large_ws_bytes(32, 4800, 32)
    assert K.convgru_large_ws_bytes(1, 1, 4) == 1 * 1 * 4 * 4 * 8 == hip_lib.savp_convgru_large_ws_bytes(1, 1, 4)
    assert K.convgru_large_ws_bytes(0, 16, 8) == 0 == hip_lib.savp_convgru_large_ws_bytes(0, 16, 8)
    for N in (1, 2, 3, 16, 32, 100):
        for HW in (1, 2, 31, 32, 33, 97, 1024, 1025, 1280, 2304, 4800, 16384, 16385, 70000, 1 << 20):
            c = K.convgru_large_chunk(N, HW)
            assert c == hip_lib.savp_convgru_large_chunk(N, HW) and c >= 1
            chunks = (HW + c - 1) // c
            assert 1 <= chunks <= K.GRU_LARGE_MAX_CHUNKS and (chunks - 1) * c < HW
            for F in (4, 12, 32, 260):
                b = K.convgru_large_ws_bytes(N, HW, F)
                assert b == N * chunks * K.GRU_LARGE_PARTIALS * F * 8 == hip_lib.savp_convgru_large_ws_bytes(N, HW, F)


def test_ctypes_struct_matches_the_header(tmp_path):
    """SavpGruLargeArgs wraps an unchanged SavpGruArgs at offset 0 and appends the workspace pointer and its size."""
    from video_prediction_amd import lib
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    c = lib.SavpGruLargeArgs
    assert [f[0] for f in c._fields_] == ['g', 'ws', 'ws_bytes'] and c._fields_[0][1] is lib.SavpGruArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "savp_hip.h"', 'int main() {',
             'printf("%zu %zu", sizeof(SavpGruLargeArgs), sizeof(SavpGruArgs));']
    lines += ['printf(" %%zu", offsetof(SavpGruLargeArgs, %s));' % f[0] for f in c._fields_]
    lines += ['printf(" %%zu", offsetof(SavpGruLargeArgs, g.%s));' % f[0] for f in lib.SavpGruArgs._fields_]
    lines += ['printf("\\n"); return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(c), ctypes.sizeof(lib.SavpGruArgs)] + [getattr(c, f[0]).offset for f in c._fields_] + \
           [getattr(lib.SavpGruArgs, f[0]).offset for f in lib.SavpGruArgs._fields_]
    assert got == want, (got, want)
    assert c.g.offset == 0 and c.ws.offset == ctypes.sizeof(lib.SavpGruArgs)


def _args(lib, N=1, HW=1280, F=8, ws_bytes=None):
    """A gates-forward problem over made-up (never dereferenced) aligned addresses."""
    a = lib.SavpGruLargeArgs()
    a.g.N, a.g.HW, a.g.F, a.g.eps = N, HW, F, 1e-6
    a.g.pre, a.g.gamma, a.g.beta, a.g.mean, a.g.rstd, a.g.u = 0x100000, 0x200000, 0x210000, 0x220000, 0x230000, 0x300000
    a.g.h.p, a.g.h.sn, a.g.h.sp = 0x400000, HW * F, F
    a.g.rh.p, a.g.rh.sn, a.g.rh.sp = 0x500000, HW * F, F
    a.ws = 0x600000
    a.ws_bytes = 8 * N * ((HW + 31) // 32) * 4 * F if ws_bytes is None else ws_bytes
    return a


def test_entries_refuse_without_a_launch(hip_lib):
    """Every refusal is decided on the host before anything is launched, so it is the same answer without a GPU."""
    from video_prediction_amd import lib
    for nm in ENTRIES:
        assert getattr(hip_lib, nm)(None, None) == -1
    fwd = hip_lib.savp_convgru_large_gates_fwd
    need = hip_lib.savp_convgru_large_ws_bytes(1, 1280, 8)
    assert _args(lib).ws_bytes == need

    def bad(**edit):
        a = _args(lib, **{k: v for k, v in edit.items() if k in ('N', 'HW', 'F', 'ws_bytes')})
        for k, v in edit.items():
            if k not in ('N', 'HW', 'F', 'ws_bytes'):
                obj, leaf = a, k.split('.')
                for part in leaf[:-1]:
                    obj = getattr(obj, part)
                setattr(obj, leaf[-1], v)
        return fwd(None, ctypes.byref(a))
    assert bad(F=6) == -1 and bad(F=0) == -1 and bad(N=0) == -1 and bad(HW=0) == -1
    assert bad(ws_bytes=need - 8) == -1 and bad(ws=None) == -1 and bad(ws=0x600004) == -1
    assert bad(**{'g.pre': None}) == -1 and bad(**{'g.u': None}) == -1 and bad(**{'g.mean': None}) == -1 and bad(**{'g.h.p': None}) == -1
    assert bad(**{'g.pre': 0x100008}) == -1 and bad(**{'g.h.p': 0x400008}) == -1 and bad(**{'g.rh.sp': 10}) == -1 and bad(**{'g.h.sn': 1282}) == -1


def test_per_layer_choice_is_a_function_of_the_frame():
    from video_prediction_amd import kernels as K
    from video_prediction_amd.models.savp_cell import gru_large_layers
    assert K.GRU_SMALL_MAX_HW == 1024
    for side in (64, 128, 256):
        assert gru_large_layers(side, side) == []
    assert gru_large_layers(64, 80) == [0, 4]             # 32 x 40 in the first encoder and the second decoder layer
    assert gru_large_layers(96, 96) == [0, 4]             # 48 x 48
    assert gru_large_layers(120, 160) == [0, 1, 3, 4]     # 60 x 80 and 30 x 40, twice each
    assert gru_large_layers(192, 192) == [1, 5]           # the 128-and-above table: 96 x 96 has no conv-RNN, 48 x 48 has

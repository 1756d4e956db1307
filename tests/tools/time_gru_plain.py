"""Times of the ConvGRU gate blocks without a normaliser (savp_convgru_plain_*) beside the instance-normalised ones (savp_convgru_*) at the
c2 GRU shapes (N = 32: 32x32x32, 16x16x64, 8x8x128), and of a c2-shaped train step with conv_rnn = 'gru', normalised against 'none'.

    python tests/tools/time_gru_plain.py kernels [--reps 200]     # launches every block `reps` times per shape; prints event-timed us / launch
    python tests/tools/time_gru_plain.py step [--steps 10] [--warmup 3]
    python tests/tools/time_gru_plain.py table TRACE.csv          # per-launch kernel time from a rocprofv3 kernel trace of `kernels`

Kernel time proper comes from the trace:  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tests/tools/time_gru_plain.py kernels
then `table OUT/.../*_kernel_trace.csv`.  Each (kernel, shape) pair has its own grid size, which is how the table tells the shapes apart.
The event-timed figures of `kernels` include the launch gaps of back-to-back launches: an upper bound, printed for orientation.

Bytes per pixel-channel (fp32), nout = ndy = 2 as in the unroll (the next layer and the next step's state slot):
gates fwd 5 (pre 2, h | rh, u), out fwd 3 + nout (pre, h, u | h' x nout), out bwd 6 + ndy (pre, h, u, dy x ndy | dpre, du, dh),
gates bwd 9 (pre 2, h, drh, du, dh | dh, dpre 2).  The normalised blocks move the same tensors (they hold `pre` in registers between their
passes) plus per-(sample, channel) statistics."""
import argparse
import collections
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(32, 32, 32, 32), (32, 16, 16, 64), (32, 8, 8, 128)]          # N, H, W, F
NIO = 2
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12          # bytes / s: the measured float4-copy rate and the specification
# floats moved per (pixel, channel)
FLOATS = {'gates_fwd': 5, 'out_fwd': 3 + NIO, 'out_bwd': 6 + NIO,'gates_bwd': 9}
KERNELS = {'gru_plain_gates_fwd_kernel': ('plain', 'gates_fwd'), 'gru_plain_out_fwd_kernel': ('plain', 'out_fwd'),
           'gru_plain_out_bwd_kernel': ('plain', 'out_bwd'), 'gru_plain_gates_bwd_kernel': ('plain', 'gates_bwd'),
           'gru_gates_fwd_kernel': ('norm', 'gates_fwd'), 'gru_out_fwd_kernel': ('norm', 'out_fwd'),
           'gru_out_bwd_kernel': ('norm', 'out_bwd'), 'gru_gates_bwd_kernel': ('norm', 'gates_bwd')}


def grid_threads(kind, N, H, W, F):
    """Total threads (rocprofv3's Grid_Size_X) of a block's launch at a shape: both families use 256-thread workgroups."""
    if kind == 'norm':
        return N * (F // 4) * 256
    return min((N * H * W * (F // 4) + 255) // 256, 2048) * 256


def run_kernels(reps):
    import torch
    from video_prediction_amd import kernels as K
    dev = 'cuda:0'
    for (N, H, W, F) in SHAPES:
        g = torch.Generator().manual_seed(1)
        r = lambda *s: torch.randn(*s, generator=g).to(dev)         # noqa: E731
        pre_g, pre_c = r(N, H, W, 2 * F), r(N, H, W, F)
        a = r(N, H, W, 3 * F + 8)                                   # [x (F + 8) | h | r*h] like the cell's input buffer
        h, rh = a[..., F + 8:2 * F + 8], a[..., 2 * F + 8:]
        u, du = torch.empty(N, H, W, F, device=dev), torch.empty(N, H, W, F, device=dev)
        outs = [torch.empty(N, H, W, F, device=dev) for _ in range(NIO)]
        dys = [r(N, H, W, F) for _ in range(NIO)]
        ag = r(N, H, W, 3 * F + 8)
        dh_tmp, dh, drh = torch.empty(N, H, W, F, device=dev), ag[..., F + 8:2 * F + 8], ag[..., 2 * F + 8:]
        dpc, dpg = torch.empty(N, H, W, F, device=dev), torch.empty(N, H, W, 2 * F, device=dev)
        g1, b1, g2, b2 = torch.ones(2 * F, device=dev), torch.zeros(2 * F, device=dev), torch.ones(F, device=dev), torch.zeros(F, device=dev)
        m1, r1 = torch.empty(N, 2 * F, device=dev), torch.empty(N, 2 * F, device=dev)
        m2, r2 = torch.empty(N, F, device=dev), torch.empty(N, F, device=dev)
        acc = [torch.zeros(c, dtype=torch.float64, device=dev) for c in (2 * F, 2 * F, F, F)]
        calls = [
            ('plain', 'gates_fwd', lambda: K.convgru_plain_gates_fwd(pre_g, h, u, rh)),
            ('plain', 'out_fwd', lambda: K.convgru_plain_out_fwd(pre_c, h, u, outs)),
            ('plain', 'out_bwd', lambda: K.convgru_plain_out_bwd(pre_c, h, u, dys, dpc, du, dh_tmp)),
            ('plain', 'gates_bwd', lambda: K.convgru_plain_gates_bwd(pre_g, h, du, drh, dpg, dh)),
            ('norm', 'gates_fwd', lambda: K.convgru_gates_fwd(pre_g, h, g1, b1, m1, r1, u, rh)),
            ('norm', 'out_fwd', lambda: K.convgru_out_fwd(pre_c, h, g2, b2, m2, r2, u, outs)),
            ('norm', 'out_bwd', lambda: K.convgru_out_bwd(pre_c, h, g2, b2, m2, r2, u, dys, dpc, du, dh_tmp, acc[2], acc[3])),
            ('norm', 'gates_bwd', lambda: K.convgru_gates_bwd(pre_g, h, g1, b1, m1, r1, du, drh, dpg, dh, acc[0], acc[1])),
        ]
        for kind, block, fn in calls:
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({'shape': [N, H, W, F], 'family': kind, 'block': block, 'reps': reps,
                              'us_per_launch_with_gaps': e0.elapsed_time(e1) * 1e3 / reps,
                              'bytes': 4 * FLOATS[block] * N * H * W * F}), flush=True)


def run_step(steps, warmup):
    import torch
    from bench import make_hparams, synthetic_batch
    from video_prediction_amd import kernels as K
    from video_prediction_amd.models.savp_model import SAVPEngine
    dev = torch.device('cuda:0')
    for cl in ('instance', 'none'):
        K.set_conv_precision('bf16')
        table = os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json')
        if os.path.exists(table):
            K.load_tuning(table)
        model = make_hparams(16, over=dict(conv_rnn='gru', conv_rnn_norm_layer=cl))
        eng = SAVPEngine(model.hparams, (64, 64, 3), 16, mode='train', seed=4, device=str(dev))
        eng.set_images(synthetic_batch(16, 1234, dev))
        info = None
        for _ in range(warmup):
            info = eng.train_step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            info = eng.train_step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({'conv_rnn': 'gru', 'conv_rnn_norm_layer': cl, 'ms_per_step': dt / steps * 1e3, 'steps': steps, 'warmup': warmup,
                          'graph': eng.graph is not None, 'losses': {'d_loss': float(info['d_loss']), 'g_loss': float(info['g_loss'])}}),
              flush=True)
        del eng
        torch.cuda.empty_cache()


def table(path):
    by = collections.defaultdict(list)
    for row in csv.DictReader(open(path)):
        name = row['Kernel_Name'].split('(')[0]
        if name in KERNELS:
            by[(name, int(row['Grid_Size_X']))].append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) * 1e-3)
    print('| shape N x H x W x F | block | family | launches | median us | MB moved | TB/s | of 6.3 TB/s | of 8 TB/s |')
    print('|---|---|---|---|---|---|---|---|---|')
    for (N, H, W, F) in SHAPES:
        for block in ('gates_fwd', 'out_fwd', 'out_bwd', 'gates_bwd'):
            for name, (kind, blk) in KERNELS.items():
                if blk != block:
                    continue
                d = sorted(by.get((name, grid_threads(kind, N, H, W, F)), []))
                if not d:
                    continue
                d = d[len(d) // 10:]                       # the first launches of a shape are warm-up
                med = d[len(d) // 2]
                nbytes = 4 * FLOATS[block] * N * H * W * F
                rate = nbytes / (med * 1e-6)
                print('| %dx%dx%dx%d | %s | %s | %d | %.2f | %.2f | %.2f | %.0f %% | %.0f %% |'
                      % (N, H, W, F, block, kind, len(d), med, nbytes / 1e6, rate / 1e12, 100 * rate / HBM_ACHIEVABLE, 100 * rate / HBM_PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernels', 'step', 'table'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if args.mode == 'kernels':
        run_kernels(args.reps)
    elif args.mode == 'step':
        run_step(args.steps, args.warmup)
    else:
        table(args.trace)


if __name__ == '__main__':
    main()

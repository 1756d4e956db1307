"""Times of the chunked two-pass instance-norm ConvGRU gate blocks (savp_convgru_large_*, csrc/gru_large.hip) beside their yardstick, the
bare cell's pointwise blocks (savp_convgru_plain_*), at the two large layers of a 120 x 160 model with N = 32: 60x80 x F 32 and 30x40 x F 64.

    python tests/tools/time_gru_large.py kernels [--shape 0|1] [--rounds 15] [--reps 40]
    python tests/tools/time_gru_large.py table TRACE.csv --shape 0|1
    python tests/tools/time_gru_large.py forward [--steps 10] [--warmup 3]

`kernels` alternates the two families block by block: each round times `reps` back-to-back launches of one block with device events, and
the median over the rounds is printed as us per call.  A call of a large block is two kernels, of a plain block one; back-to-back calls
include the launch gaps, so these figures are upper bounds.  Kernel time proper comes from a trace of one shape:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tests/tools/time_gru_large.py kernels --shape 0
then `table OUT/.../*_kernel_trace.csv --shape 0` adds the two passes of each large block and prints median us, the ratio to the plain twin
and the achieved bytes / s against the block's ALGORITHMIC bytes: the floats the mathematics has to move once, which is what the plain
block moves (gates fwd 5, out fwd 3 + nout, out bwd 6 + ndy, gates bwd 9 per pixel-channel; nout = ndy = 2 as in the unroll).  The large
blocks read their operands a second time in the apply pass, so their rate against these bytes is at most about half the copy rate.
`forward` times the generator's posterior + prior unroll of a 120 x 160 x 1 model (B = 16, T = 10) with conv_rnn = gru and lstm on both
datapaths (training at such a frame is refused for the normalised GRU, see profiles/gru_large.md)."""
import argparse
import collections
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(32, 60, 80, 32), (32, 30, 40, 64)]          # N, H, W, F
NIO = 2
BLOCKS = ('gates_fwd', 'out_fwd', 'out_bwd', 'gates_bwd')
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12          # bytes / s: the measured float4-copy rate and the specification
FLOATS = {'gates_fwd': 5, 'out_fwd': 3 + NIO, 'out_bwd': 6 + NIO, 'gates_bwd': 9}      # floats moved per (pixel, channel)
BUDGET = 2.5                                        # a large block may take this many times its plain twin
KERNELS = {'gru_plain_%s_kernel' % b: ('plain', b) for b in BLOCKS}
KERNELS.update({'grul_%s_sums' % b: ('large', b) for b in BLOCKS})
KERNELS.update({'grul_%s_apply' % b: ('large', b) for b in BLOCKS})
NAME_RE = re.compile(r'\b(' + '|'.join(sorted(KERNELS, key=len, reverse=True)) + r')\b')


def algorithmic_bytes(block, N, H, W, F):
    return 4 * FLOATS[block] * N * H * W * F


def make_calls(shape):
    import torch
    from video_prediction_amd import kernels as K
    dev = 'cuda:0'
    N, H, W, F = shape
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)         # noqa: E731
    pre_g, pre_c = r(N, H, W, 2 * F), r(N, H, W, F)
    a = r(N, H, W, 3 * F + 8)                                   # [x (F + 8) | h | r*h] like the cell's input buffer
    h, rh = a[..., F + 8:2 * F + 8], a[..., 2 * F + 8:]
    u, du = torch.rand(N, H, W, F, generator=g).to(dev), torch.empty(N, H, W, F, device=dev)
    outs = [torch.empty(N, H, W, F, device=dev) for _ in range(NIO)]
    dys = [r(N, H, W, F) for _ in range(NIO)]
    ag = r(N, H, W, 3 * F + 8)
    dh_tmp, dh, drh = torch.empty(N, H, W, F, device=dev), ag[..., F + 8:2 * F + 8], ag[..., 2 * F + 8:]
    dpc, dpg = torch.empty(N, H, W, F, device=dev), torch.empty(N, H, W, 2 * F, device=dev)
    g1, b1, g2, b2 = torch.ones(2 * F, device=dev), torch.zeros(2 * F, device=dev), torch.ones(F, device=dev), torch.zeros(F, device=dev)
    m1, r1 = torch.empty(N, 2 * F, device=dev), torch.empty(N, 2 * F, device=dev)
    m2, r2 = torch.empty(N, F, device=dev), torch.empty(N, F, device=dev)
    acc = [torch.zeros(c, dtype=torch.float64, device=dev) for c in (2 * F, 2 * F, F, F)]
    ws = K.convgru_large_ws(dev, N, H * W, F)
    return collections.OrderedDict([
        (('gates_fwd', 'plain'), lambda: K.convgru_plain_gates_fwd(pre_g, h, u, rh)),
        (('gates_fwd', 'large'), lambda: K.convgru_large_gates_fwd(pre_g, h, g1, b1, m1, r1, u, rh, ws)),
        (('out_fwd', 'plain'), lambda: K.convgru_plain_out_fwd(pre_c, h, u, outs)),
        (('out_fwd', 'large'), lambda: K.convgru_large_out_fwd(pre_c, h, g2, b2, m2, r2, u, outs, ws)),
        (('out_bwd', 'plain'), lambda: K.convgru_plain_out_bwd(pre_c, h, u, dys, dpc, du, dh_tmp)),
        (('out_bwd', 'large'), lambda: K.convgru_large_out_bwd(pre_c, h, g2, b2, m2, r2, u, dys, dpc, du, dh_tmp, acc[2], acc[3], ws)),
        (('gates_bwd', 'plain'), lambda: K.convgru_plain_gates_bwd(pre_g, h, du, drh, dpg, dh)),
        (('gates_bwd', 'large'), lambda: K.convgru_large_gates_bwd(pre_g, h, g1, b1, m1, r1, du, drh, dpg, dh, acc[0], acc[1], ws)),
    ])


def run_kernels(shapes, rounds, reps):
    import torch
    for shape in shapes:
        calls = make_calls(shape)
        for fn in calls.values():                      # warm-up: code objects, clocks
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        times = collections.defaultdict(list)
        for _ in range(rounds):                        # the families alternate inside every round
            for key, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3 / reps)
        for block in BLOCKS:
            med = {fam: sorted(times[(block, fam)])[rounds // 2] for fam in ('plain', 'large')}
            nbytes = algorithmic_bytes(block, *shape)
            print(json.dumps({'shape': list(shape), 'block': block, 'rounds': rounds, 'reps': reps,
                              'plain_us_per_call_with_gaps': round(med['plain'], 2), 'large_us_per_call_with_gaps': round(med['large'], 2),
                              'ratio': round(med['large'] / med['plain'], 3), 'budget': BUDGET, 'within_budget': med['large'] <= BUDGET * med['plain'],
                              'algorithmic_bytes': nbytes, 'large_TB_per_s': round(nbytes / med['large'] * 1e-6, 3),
                              'plain_TB_per_s': round(nbytes / med['plain'] * 1e-6, 3)}), flush=True)


def table(path, shape):
    by = collections.defaultdict(list)
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp']))
    for row in rows:
        m = NAME_RE.search(row['Kernel_Name'])
        if m:
            by[m.group(1)].append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) * 1e-3)

    def median(name):
        d = by.get(name, [])
        d = sorted(d[len(d) // 10:])                   # the first launches are warm-up
        return d[len(d) // 2] if d else float('nan')
    N, H, W, F = shape
    print('| shape N x H x W x F | block | plain us | large sums us | large apply us | large us | ratio | budget %.1f | MB (algorithmic) | '
          'plain TB/s | large TB/s | large of 6.3 TB/s |' % BUDGET)
    print('|---|---|---|---|---|---|---|---|---|---|---|---|')
    for block in BLOCKS:
        p, s, a = median('gru_plain_%s_kernel' % block), median('grul_%s_sums' % block), median('grul_%s_apply' % block)
        nbytes = algorithmic_bytes(block, N, H, W, F)
        print('| %dx%dx%dx%d | %s | %.2f | %.2f | %.2f | %.2f | %.2f | %s | %.1f | %.2f | %.2f | %.0f %% |'
              % (N, H, W, F, block, p, s, a, s + a, (s + a) / p, 'within' if s + a <= BUDGET * p else 'OVER', nbytes / 1e6,
                 nbytes / p * 1e-6, nbytes / (s + a) * 1e-6, 100 * nbytes / (s + a) * 1e6 / HBM_ACHIEVABLE))


def run_forward(steps, warmup):
    import torch
    from tests import gpu_model_checks as MC
    from video_prediction_amd import kernels as K, variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    B, T, H, W, C = 16, 10, 120, 160, 1
    for prec in ('f32', 'bf16'):
        for rnn in ('gru', 'lstm'):
            K.set_conv_precision(prec)
            hp = MC.make_hparams(context_frames=2, sequence_length=T, nz=8, conv_rnn=rnn, schedule_sampling='inverse_sigmoid')
            vals = V.init_variables(V.variable_specs(hp, (H, W, C), mode='test'), seed=4)
            eng = SAVPEngine(hp, (H, W, C), B, mode='test', values=vals, device='cuda:0')
            eng.mode = 'train'                         # the posterior + prior unroll of batch 2B
            eng.set_images(MC.synth(hp, B, H, W, C, 0).float().to('cuda:0'), time_major=True)
            noise = MC.make_noise(hp, B, sampling=True)
            for i in range(warmup + steps):
                if i == warmup:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                eng.prep_generator_weights()
                eng.forward_generator(noise)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({'what': 'generator forward, posterior + prior, eager launches', 'frame': [H, W, C], 'B': B, 'T': T, 'conv_rnn': rnn,
                              'datapath': prec, 'ms_per_forward': round(dt / steps * 1e3, 2), 'steps': steps, 'warmup': warmup}), flush=True)
            del eng
            torch.cuda.empty_cache()
    K.set_conv_precision('f32')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernels', 'table', 'forward'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--shape', type=int, choices=[0, 1])
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if args.mode == 'kernels':
        run_kernels(SHAPES if args.shape is None else [SHAPES[args.shape]], args.rounds, args.reps)
    elif args.mode == 'forward':
        run_forward(args.steps, args.warmup)
    else:
        if args.shape is None:
            ap.error('table needs --shape: a trace holds one shape')
        table(args.trace, SHAPES[args.shape])


if __name__ == '__main__':
    main()

"""Times of the ConvGRU gate blocks (gates_fwd, out_fwd, out_bwd, gates_bwd), one family beside its yardstick:

    --family plain   the pointwise blocks of the cell without a normaliser (savp_convgru_plain_*) beside the one-workgroup instance-norm
                     blocks (savp_convgru_*), at the c2 GRU shapes (N = 32: 32x32x32, 16x16x64, 8x8x128)
    --family large   the chunked two-pass instance-norm blocks (savp_convgru_large_*) beside the plain ones, at the two large layers of a
                     120 x 160 model with N = 32: 60x80 x F 32 and 30x40 x F 64
    --family ln      the two-pass layer-norm blocks (savp_convgru_ln_*) beside the composition of launches they replace --
                     groupnorm_act_fwd / groupnorm_act_bwd (act = 'none', a stored normalised tensor and its gradient) plus the plain
                     blocks -- at the c2 shapes and 60x80x32

    python tests/tools/time_gru_blocks.py --family FAMILY kernels [--shape I] [--rounds R] [--reps K]
    python tests/tools/time_gru_blocks.py --family plain|large table TRACE.csv [--shape I]
    python tests/tools/time_gru_blocks.py --family plain|ln step [--steps 10] [--warmup W]
    python tests/tools/time_gru_blocks.py --family large forward [--steps 10] [--warmup 3]

`kernels` times `reps` back-to-back calls of one block with device events per round and prints the median over the rounds as us per
call.  plain: one round of 200 calls, each call warmed up right before it; large, ln: all calls warmed up, then 15 rounds of 40 in which
the two columns alternate block by block; ln also prints the spread, max - min over the rounds as a fraction of the median.  A call of a
two-pass block is two kernels, of a plain block one, of the composition the norm's launches plus one; back-to-back calls include the
launch gaps, so these figures are upper bounds.
Kernel time proper comes from a trace:  rocprofv3 --kernel-trace --output-format csv -d OUT -- python tests/tools/time_gru_blocks.py
--family FAMILY kernels [--shape I], then `table OUT/.../*_kernel_trace.csv`.  plain: every (kernel, shape) pair has its own grid size,
which is how the table tells the shapes apart; large: a trace holds one shape (--shape), the two passes of a block are added, and the
ratio to the plain twin is held against BUDGET.  Rates are against the block's ALGORITHMIC bytes, the floats the mathematics has to move
once (per pixel-channel, fp32, nout = ndy = 2 as in the unroll: gates fwd 5 (pre 2, h | rh, u), out fwd 3 + nout (pre, h, u | h' x nout),
out bwd 6 + ndy (pre, h, u, dy x ndy | dpre, du, dh), gates bwd 9 (pre 2, h, drh, du, dh | dh, dpre 2)); the two-pass blocks read their
operands a second time in the apply pass, so their rate against these bytes is at most about half the copy rate.
`step` times a c2-shaped train step with conv_rnn = 'gru': plain, the normalised cell against 'none'; ln, the opt-in layer-norm model next
to gru + instance on both datapaths (eager warm-up, then captured-graph replays).  `forward` times the generator's posterior + prior
unroll of a 120 x 160 x 1 model (B = 16, T = 10) with conv_rnn = gru and lstm on both datapaths (training at such a frame is refused for
the normalised GRU, see profiles/gru_large.md)."""
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

C2_SHAPES = [(32, 32, 32, 32), (32, 16, 16, 64), (32, 8, 8, 128)]          # N, H, W, F
LARGE_SHAPES = [(32, 60, 80, 32), (32, 30, 40, 64)]
# per family: the shapes, (yardstick, subject) columns, and the defaults of kernels' --rounds / --reps and of its warm-up calls
FAMILIES = {'plain': (C2_SHAPES, ('plain', 'norm'), 1, 200, 10),
            'large': (LARGE_SHAPES, ('plain', 'large'), 15, 40, 20),
            'ln': (C2_SHAPES + LARGE_SHAPES[:1], ('composition', 'fused'), 15, 40, 20)}
NIO = 2
BLOCKS = ('gates_fwd', 'out_fwd', 'out_bwd', 'gates_bwd')
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12          # bytes / s: the measured float4-copy rate and the specification
FLOATS = {'gates_fwd': 5, 'out_fwd': 3 + NIO, 'out_bwd': 6 + NIO, 'gates_bwd': 9}      # floats moved per (pixel, channel)
BUDGET = 2.5                                        # a large block may take this many times its plain twin
KERNELS = {'gru_plain_%s_kernel' % b: ('plain', b) for b in BLOCKS}
KERNELS.update({'gru_%s_kernel' % b: ('norm', b) for b in BLOCKS})
SUMS = dict(gates_fwd='gru2p_gates_fwd_sums', out_fwd='gru2p_out_fwd_sums', out_bwd='gru2p_out_bwd_sums<false>',
            gates_bwd='gru2p_gates_bwd_sums<false>')          # pass 1 of the large blocks; pass 2 is grul_<block>_apply


def algorithmic_bytes(block, N, H, W, F):
    return 4 * FLOATS[block] * N * H * W * F


def make_calls(family, shape):
    """{(block, column): a call} of the family's two columns over one set of tensors."""
    import torch
    from video_prediction_amd import kernels as K
    dev = 'cuda:0'
    N, H, W, F = shape
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)         # noqa: E731
    e = lambda *s: torch.empty(*s, device=dev)                  # noqa: E731
    pre_g, pre_c = r(N, H, W, 2 * F), r(N, H, W, F)
    a = r(N, H, W, 3 * F + 8)                                   # [x (F + 8) | h | r*h] like the cell's input buffer
    h, rh = a[..., F + 8:2 * F + 8], a[..., 2 * F + 8:]
    u, du = torch.rand(N, H, W, F, generator=g).to(dev), e(N, H, W, F)
    outs = [e(N, H, W, F) for _ in range(NIO)]
    dys = [r(N, H, W, F) for _ in range(NIO)]
    ag = r(N, H, W, 3 * F + 8)
    dh_tmp, dh, drh = e(N, H, W, F), ag[..., F + 8:2 * F + 8], ag[..., 2 * F + 8:]
    dpc, dpg = e(N, H, W, F), e(N, H, W, 2 * F)
    beta1 = torch.ones if family == 'ln' else torch.zeros          # the variables' initial values: the layer norm's reset / update beta is 1
    g1, b1, g2, b2 = torch.ones(2 * F, device=dev), beta1(2 * F, device=dev), torch.ones(F, device=dev), torch.zeros(F, device=dev)
    s1, s2 = ((N, 2), (N, 1)) if family == 'ln' else ((N, 2 * F), (N, F))          # statistics per (sample, group) or (sample, channel)
    m1, r1, m2, r2 = e(*s1), e(*s1), e(*s2), e(*s2)
    acc = [torch.zeros(c, dtype=torch.float64, device=dev) for c in (2 * F, 2 * F, F, F)]
    ws = () if family == 'plain' else (K.convgru_large_ws(dev, N, H * W, F),)
    # nothing but the timed call inside a lambda: many of these calls are bounded by the host
    gates_fwd, out_fwd, out_bwd, gates_bwd = (getattr(K, 'convgru_%s%s' % ({'plain': '', 'large': 'large_', 'ln': 'ln_'}[family], b)) for b in BLOCKS)
    subject = {'gates_fwd': lambda: gates_fwd(pre_g, h, g1, b1, m1, r1, u, rh, *ws),
               'out_fwd': lambda: out_fwd(pre_c, h, g2, b2, m2, r2, u, outs, *ws),
               'out_bwd': lambda: out_bwd(pre_c, h, g2, b2, m2, r2, u, dys, dpc, du, dh_tmp, acc[2], acc[3], *ws),
               'gates_bwd': lambda: gates_bwd(pre_g, h, g1, b1, m1, r1, du, drh, dpg, dh, acc[0], acc[1], *ws)}
    # the yardstick: the plain blocks on the raw tensors ...
    yard = {'gates_fwd': lambda: K.convgru_plain_gates_fwd(pre_g, h, u, rh),
            'out_fwd': lambda: K.convgru_plain_out_fwd(pre_c, h, u, outs),
            'out_bwd': lambda: K.convgru_plain_out_bwd(pre_c, h, u, dys, dpc, du, dh_tmp),
            'gates_bwd': lambda: K.convgru_plain_gates_bwd(pre_g, h, du, drh, dpg, dh)}
    if family == 'ln':          # ... or on the normalised gates / candidate the group norm stores, and their gradients
        ng, nc, dng, dnc = e(N, H, W, 2 * F), e(N, H, W, F), e(N, H, W, 2 * F), e(N, H, W, F)

        def comp_gates_fwd():
            K.groupnorm_act_fwd(pre_g, g1, b1, [ng], m1, r1, groups=2, act='none')
            K.convgru_plain_gates_fwd(ng, h, u, rh)

        def comp_out_fwd():
            K.groupnorm_act_fwd(pre_c, g2, b2, [nc], m2, r2, groups=1, act='none')
            K.convgru_plain_out_fwd(nc, h, u, outs)

        def comp_out_bwd():
            K.convgru_plain_out_bwd(nc, h, u, dys, dnc, du, dh_tmp)
            K.groupnorm_act_bwd(pre_c, g2, b2, m2, r2, [dnc], dpc, acc[2], acc[3], groups=1, act='none')

        def comp_gates_bwd():
            K.convgru_plain_gates_bwd(ng, h, du, drh, dng, dh)
            K.groupnorm_act_bwd(pre_g, g1, b1, m1, r1, [dng], dpg, acc[0], acc[1], groups=2, act='none')
        yard = dict(gates_fwd=comp_gates_fwd, out_fwd=comp_out_fwd, out_bwd=comp_out_bwd, gates_bwd=comp_gates_bwd)
    cols = FAMILIES[family][1]
    return collections.OrderedDict(((b, c), fns[b]) for b in BLOCKS for c, fns in zip(cols, (yard, subject)))


def run_kernels(family, shapes, rounds, reps):
    import torch
    cols, warm = FAMILIES[family][1], FAMILIES[family][4]
    for shape in shapes:
        calls = make_calls(family, shape)
        for fn in calls.values() if rounds > 1 else ():          # warm-up: code objects, clocks
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        times = collections.defaultdict(list)
        for _ in range(rounds):                        # the columns alternate inside every round
            for key, fn in calls.items():
                if rounds == 1:                        # nothing to alternate (plain): each call is warmed up right before it is timed
                    for _ in range(warm):
                        fn()
                    torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) * 1e3 / reps)
        med = {k: sorted(t)[rounds // 2] for k, t in times.items()}
        spread = {k: (max(t) - min(t)) / med[k] for k, t in times.items()}
        if family == 'plain':
            for col in cols:
                for block in BLOCKS:
                    print(json.dumps({'shape': list(shape), 'family': col, 'block': block, 'reps': reps,
                                      'us_per_launch_with_gaps': med[(block, col)], 'bytes': algorithmic_bytes(block, *shape)}), flush=True)
        for block in BLOCKS if family != 'plain' else ():
            y, s = med[(block, cols[0])], med[(block, cols[1])]
            row = {'shape': list(shape), 'block': block, 'rounds': rounds, 'reps': reps,
                   cols[0] + '_us_per_call_with_gaps': round(y, 2), cols[1] + '_us_per_call_with_gaps': round(s, 2)}
            if family == 'large':
                nbytes = algorithmic_bytes(block, *shape)
                row.update({'ratio': round(s / y, 3), 'budget': BUDGET, 'within_budget': s <= BUDGET * y, 'algorithmic_bytes': nbytes,
                            'large_TB_per_s': round(nbytes / s * 1e-6, 3), 'plain_TB_per_s': round(nbytes / y * 1e-6, 3)})
            else:
                row.update({'fused_over_composition': round(s / y, 3), 'composition_spread': round(spread[(block, cols[0])], 3),
                            'fused_spread': round(spread[(block, cols[1])], 3)})
            print(json.dumps(row), flush=True)
        del calls
        torch.cuda.empty_cache()


def _trace_times(path, key):
    """{key(row): [kernel us]} of a rocprofv3 kernel trace, in launch order; rows whose key is None are left out."""
    by = collections.defaultdict(list)
    for row in sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp'])):
        k = key(row)
        if k is not None:
            by[k].append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) * 1e-3)
    return by


def _median(d):
    d = sorted(d[len(d) // 10:])                       # large: the first launches are warm-up
    return d[len(d) // 2] if d else float('nan')


def table_plain(path):
    def key(row):
        name = row['Kernel_Name'].split('(')[0]
        return (name, int(row['Grid_Size_X'])) if name in KERNELS else None
    by = _trace_times(path, key)

    def grid_threads(kind, N, H, W, F):
        """Total threads (rocprofv3's Grid_Size_X) of a block's launch at a shape: both families use 256-thread workgroups."""
        return N * (F // 4) * 256 if kind == 'norm' else min((N * H * W * (F // 4) + 255) // 256, 2048) * 256
    print('| shape N x H x W x F | block | family | launches | median us | MB moved | TB/s | of 6.3 TB/s | of 8 TB/s |')
    print('|---|---|---|---|---|---|---|---|---|')
    for (N, H, W, F) in C2_SHAPES:
        for block in BLOCKS:
            for name, (kind, blk) in KERNELS.items():
                d = by.get((name, grid_threads(kind, N, H, W, F)), [])
                if blk != block or not d:
                    continue
                d = sorted(d)[len(d) // 10:]               # plain: the median of all but the shortest tenth
                med, nbytes = d[len(d) // 2], algorithmic_bytes(block, N, H, W, F)
                rate = nbytes / (med * 1e-6)
                print('| %dx%dx%dx%d | %s | %s | %d | %.2f | %.2f | %.2f | %.0f %% | %.0f %% |'
                      % (N, H, W, F, block, kind, len(d), med, nbytes / 1e6, rate / 1e12, 100 * rate / HBM_ACHIEVABLE,
                         100 * rate / HBM_PEAK))


def table_large(path, shape):
    names = ['gru_plain_%s_kernel' % b for b in BLOCKS] + ['grul_%s_apply' % b for b in BLOCKS] + list(SUMS.values())
    name_re = re.compile(r'\b(' + '|'.join(re.escape(n) for n in sorted(names, key=len, reverse=True)) + r')')

    def key(row):
        m = name_re.search(row['Kernel_Name'])
        return m.group(1) if m else None
    by = _trace_times(path, key)
    N, H, W, F = shape
    print('| shape N x H x W x F | block | plain us | large sums us | large apply us | large us | ratio | budget %.1f | MB (algorithmic) | '
          'plain TB/s | large TB/s | large of 6.3 TB/s |' % BUDGET)
    print('|---|---|---|---|---|---|---|---|---|---|---|---|')
    for block in BLOCKS:
        p, s, a = (_median(by.get(n, [])) for n in ('gru_plain_%s_kernel' % block, SUMS[block], 'grul_%s_apply' % block))
        nbytes = algorithmic_bytes(block, N, H, W, F)
        print('| %dx%dx%dx%d | %s | %.2f | %.2f | %.2f | %.2f | %.2f | %s | %.1f | %.2f | %.2f | %.0f %% |'
              % (N, H, W, F, block, p, s, a, s + a, (s + a) / p, 'within' if s + a <= BUDGET * p else 'OVER', nbytes / 1e6,
                 nbytes / p * 1e-6, nbytes / (s + a) * 1e-6, 100 * nbytes / (s + a) * 1e6 / HBM_ACHIEVABLE))


def step_plain(steps, warmup):
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


def step_ln(steps, warmup):
    import torch
    from tests import gpu_model_checks as MC
    from video_prediction_amd import kernels as K
    from video_prediction_amd.models.savp_model import SAVPEngine
    c2 = MC.BENCH_CASES['c2']
    B, T, H, W, C = c2['B'], c2['T'], c2['H'], c2['W'], c2['C']
    for prec in ('bf16', 'f32'):
        for tag, over, ln_gru in (('gru_instance', dict(conv_rnn='gru'), False), ('gru_layer', dict(conv_rnn='gru', conv_rnn_norm_layer='layer'), True)):
            K.set_conv_precision(prec)
            hp = MC.make_hparams(context_frames=c2['context'], sequence_length=T, clip_length=10, nz=c2['nz'], lr=2e-4, beta1=0.5, beta2=0.999,
                                 l1_weight=100.0, l2_weight=0.0, kl_weight=c2['kl_weight'], kl_anneal='none', video_sn_vae_gan_weight=0.1,
                                 video_sn_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0, gan_feature_cdist_weight=0.0, **over)
            eng = SAVPEngine(hp, (H, W, C), B, mode='train', seed=4, device='cuda:0', ln_gru=ln_gru)
            eng.set_images(MC.synth(hp, B, H, W, C, 0).float().to('cuda:0'), time_major=True)
            rounds = []
            for i in range(warmup + 3 * steps):
                if i >= warmup and (i - warmup) % steps == 0:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                info = eng.train_step()
                if i >= warmup and (i - warmup) % steps == steps - 1:
                    torch.cuda.synchronize()
                    rounds.append((time.perf_counter() - t0) / steps * 1e3)
            print(json.dumps({'what': 'train step, c2 shape', 'model': tag, 'datapath': prec, 'B': B, 'T': T, 'frame': [H, W, C],
                              'ms_per_step_median_of_3_rounds': round(sorted(rounds)[1], 3), 'rounds_ms': [round(r_, 3) for r_ in rounds],
                              'replayed': eng.graph is not None, 'g_loss': float(info['g_loss']), 'steps_per_round': steps, 'warmup': warmup}),
                  flush=True)
            del eng
            torch.cuda.empty_cache()
    K.set_conv_precision('f32')


def forward_large(steps, warmup):
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
    ap.add_argument('--family', choices=sorted(FAMILIES), required=True)
    ap.add_argument('mode', choices=['kernels', 'table', 'step', 'forward'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--shape', type=int, help='index into the family\'s shapes (default: all)')
    ap.add_argument('--rounds', type=int)
    ap.add_argument('--reps', type=int)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int)
    args = ap.parse_args()
    shapes, _, rounds, reps, _ = FAMILIES[args.family]
    modes = {('plain', 'table'): lambda: table_plain(args.trace),
             ('large', 'table'): lambda: table_large(args.trace, shapes[args.shape]) if args.shape is not None else
             ap.error('table needs --shape: a trace holds one shape'),
             ('plain', 'step'): lambda: step_plain(args.steps, 3 if args.warmup is None else args.warmup),
             ('ln', 'step'): lambda: step_ln(args.steps, 4 if args.warmup is None else args.warmup),
             ('large', 'forward'): lambda: forward_large(args.steps, 3 if args.warmup is None else args.warmup)}
    if args.mode == 'kernels':
        run_kernels(args.family, shapes if args.shape is None else [shapes[args.shape]], args.rounds or rounds, args.reps or reps)
    elif (args.family, args.mode) in modes:
        modes[(args.family, args.mode)]()
    else:
        ap.error('--family %s has no mode %r' % (args.family, args.mode))


if __name__ == '__main__':
    main()

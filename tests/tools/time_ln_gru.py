"""Times of the fused two-pass layer-norm ConvGRU gate blocks (savp_convgru_ln_*, csrc/ln_gru.hip) beside the composition of launches they
replace -- groupnorm_act_fwd / groupnorm_act_bwd (csrc/group_norm.hip, act = 'none', a stored normalised tensor and its gradient) plus the
pointwise convgru_plain_* (csrc/gru.hip) -- at the c2 step's GRU layer shapes with N = 32 (32x32x32, 16x16x64, 8x8x128) and one large plane
(60x80x32).

    python tests/tools/time_ln_gru.py kernels [--shape 0..3] [--rounds 15] [--reps 40]
    python tests/tools/time_ln_gru.py step [--steps 10] [--warmup 4]

`kernels` alternates the two families block by block, in the manner of tests/tools/time_gru_large.py: each round times `reps` back-to-back
calls of one block with device events; printed are the median over the rounds as us per call and the run-to-run spread (max - min over the
rounds, as a fraction of the median).  A call of a fused block is two kernels; of the composition, the norm's launches plus one pointwise
kernel.  Back-to-back calls include the launch gaps, so the figures are upper bounds; both columns carry them alike.
`step` times the train step (eager warm-up, then captured-graph replays) of the opt-in model (conv_rnn = gru, conv_rnn_norm_layer = layer)
next to gru + instance at the c2 shape (B = 16, T = 30, 64 x 64 x 3) in the same run, on both datapaths."""
import argparse
import collections
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(32, 32, 32, 32), (32, 16, 16, 64), (32, 8, 8, 128), (32, 60, 80, 32)]          # N, H, W, F
NIO = 2
BLOCKS = ('gates_fwd', 'out_fwd', 'out_bwd', 'gates_bwd')


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
    g1, b1, g2, b2 = torch.ones(2 * F, device=dev), torch.ones(2 * F, device=dev), torch.ones(F, device=dev), torch.zeros(F, device=dev)
    m1, r1 = torch.empty(N, 2, device=dev), torch.empty(N, 2, device=dev)
    m2, r2 = torch.empty(N, 1, device=dev), torch.empty(N, 1, device=dev)
    acc = [torch.zeros(c, dtype=torch.float64, device=dev) for c in (2 * F, 2 * F, F, F)]
    ws = K.convgru_ln_ws(dev, N, H * W, F)
    # the composition's extra tensors: the normalised gates / candidate and their gradients
    ng, nc = torch.empty(N, H, W, 2 * F, device=dev), torch.empty(N, H, W, F, device=dev)
    dng, dnc = torch.empty(N, H, W, 2 * F, device=dev), torch.empty(N, H, W, F, device=dev)

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
    return collections.OrderedDict([
        (('gates_fwd', 'composition'), comp_gates_fwd),
        (('gates_fwd', 'fused'), lambda: K.convgru_ln_gates_fwd(pre_g, h, g1, b1, m1, r1, u, rh, ws)),
        (('out_fwd', 'composition'), comp_out_fwd),
        (('out_fwd', 'fused'), lambda: K.convgru_ln_out_fwd(pre_c, h, g2, b2, m2, r2, u, outs, ws)),
        (('out_bwd', 'composition'), comp_out_bwd),
        (('out_bwd', 'fused'), lambda: K.convgru_ln_out_bwd(pre_c, h, g2, b2, m2, r2, u, dys, dpc, du, dh_tmp, acc[2], acc[3], ws)),
        (('gates_bwd', 'composition'), comp_gates_bwd),
        (('gates_bwd', 'fused'), lambda: K.convgru_ln_gates_bwd(pre_g, h, g1, b1, m1, r1, du, drh, dpg, dh, acc[0], acc[1], ws)),
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
            med, spread = {}, {}
            for fam in ('composition', 'fused'):
                t = sorted(times[(block, fam)])
                med[fam], spread[fam] = t[rounds // 2], (t[-1] - t[0]) / t[rounds // 2]
            print(json.dumps({'shape': list(shape), 'block': block, 'rounds': rounds, 'reps': reps,
                              'composition_us_per_call_with_gaps': round(med['composition'], 2), 'fused_us_per_call_with_gaps': round(med['fused'], 2),
                              'fused_over_composition': round(med['fused'] / med['composition'], 3),
                              'composition_spread': round(spread['composition'], 3), 'fused_spread': round(spread['fused'], 3)}), flush=True)
        del calls
        torch.cuda.empty_cache()


def run_step(steps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernels', 'step'])
    ap.add_argument('--shape', type=int, choices=range(len(SHAPES)))
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=4)
    args = ap.parse_args()
    if args.mode == 'kernels':
        run_kernels(SHAPES if args.shape is None else [SHAPES[args.shape]], args.rounds, args.reps)
    else:
        run_step(args.steps, args.warmup)


if __name__ == '__main__':
    main()

"""Step time of the c2-shaped bf16 train step (BAIR 64x64x3, B = 16, T = 30, ours_savp recipe, replayed hipGraph, after warm-up) for the
default layers and for each of downsample_layer = conv2d, upsample_layer = deconv2d, activation_layer = elu alone and together, and the
per-launch times of the new down / upsample convolutions beside the 'pool' / 'up' launches they replace.

    python tests/tools/time_layer_choices.py [--steps 10] [--warmup 3] [--repeats 5] [--only conv2d] [--no-launches]

Step times: `--repeats` timed regions of `--steps` replayed steps each per configuration, the median and the spread are reported (one JSON
line per configuration).  Launch times: each ladder convolution of c2 (T x 2B = 32 samples per launch, the shapes and dtypes of the
model's buffers) built on its own, every mode (forward, data gradient, weight gradient) timed with events around 200 back-to-back launches,
median of 7 such regions after 3 warm-up regions; one JSON line per (layer, kind)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = [('default', {}), ('conv2d', dict(downsample_layer='conv2d')), ('deconv2d', dict(upsample_layer='deconv2d')),
           ('elu', dict(activation_layer='elu')),
           ('all_three', dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu'))]

# the ladder of c2 (ngf 32, tiled latent of 8 channels; engine input channels padded to 8): name, kind pair, k, hi-res plane, channels on the
# hi-res side, channels on the lo-res side
LADDER = [('h0', ('pool', 'down'), 5, 64, 16, 32), ('h1', ('pool', 'down'), 3, 32, 40, 64), ('h2', ('pool', 'down'), 3, 16, 72, 128),
          ('h3', ('up', 'deconv'), 3, 16, 64, 136), ('h4', ('up', 'deconv'), 3, 32, 32, 136), ('h5', ('up', 'deconv'), 3, 64, 32, 72)]


def time_steps(args, torch, K, name, over):
    from bench import make_hparams, synthetic_batch
    from video_prediction_amd.models.savp_model import SAVPEngine
    dev = torch.device('cuda:0')
    model = make_hparams(16, over=over)
    eng = SAVPEngine(model.hparams, (64, 64, 3), 16, mode='train', seed=4, device=str(dev))
    eng.set_images(synthetic_batch(16, 1234, dev))
    info = None
    for _ in range(args.warmup):
        info = eng.train_step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.steps):
            info = eng.train_step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    print(json.dumps({'config': name, 'ms_per_step_median': statistics.median(ms), 'ms_per_step_min': min(ms), 'ms_per_step_max': max(ms),
                      'regions': args.repeats, 'steps_per_region': args.steps, 'warmup': args.warmup, 'graph': eng.graph is not None,
                      'losses': {'d_loss': float(info['d_loss']), 'g_loss': float(info['g_loss'])}}), flush=True)
    del eng
    torch.cuda.empty_cache()


def _region(torch, fn, n=200):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per launch


def time_launches(torch, K):
    from video_prediction_amd.engine import ConvLayer, _TensorStore, same_pad_before
    dev = torch.device('cuda:0')
    N = 32
    bf = torch.bfloat16
    for name, kinds, k, hi, chi, clo in LADDER:
        for kind in kinds:
            down = kind in ('pool', 'down')
            if down:            # [k, k, Cin (hi-res side), F (lo-res side)]
                W = torch.randn(k, k, chi, clo, device=dev) * 0.05
                b = torch.zeros(clo, device=dev)
                kk = k + 1
            elif kind == 'up':   # [k, k, Cin (lo-res side), F (hi-res side)], folded to k + 3 taps
                W = torch.randn(k, k, clo, chi, device=dev) * 0.05
                b = torch.zeros(chi, device=dev)
                kk = k + 3
            else:                # deconv: [k, k, F (hi-res side), Cin (lo-res side)]
                W = torch.randn(k, k, chi, clo, device=dev) * 0.05
                b = torch.zeros(chi, device=dev)
                kk = k + 1
            st = _TensorStore({'k': W, 'b': b}, {'k': torch.zeros_like(W), 'b': torch.zeros_like(b)})
            L = ConvLayer(st, 'k', 'b', kind, (k, k), (2, 2), (same_pad_before(kk, 2, hi),) * 2)
            L.prep()
            # the model's buffers: a bf16 input behind layer 0, an fp32 pre-activation, its bf16 gradient, an fp32 input gradient
            x_hi = torch.randn(N, hi, hi, chi, device=dev).to(torch.float32 if name == 'h0' else bf)
            x_lo = torch.randn(N, hi // 2, hi // 2, clo, device=dev).to(bf if clo % 8 == 0 else torch.float32)
            if down:
                x, y = x_hi, torch.empty(N, hi // 2, hi // 2, clo, device=dev)
            else:
                x, y = x_lo, torch.empty(N, hi, hi, chi, device=dev)
            dy = torch.randn_like(y).to(bf)
            dx = torch.empty(x.shape, device=dev)
            modes = {'fwd': lambda: L.forward(x, y), 'dgrad': lambda: L.backward_data(dy, dx, beta=0),
                     'wgrad': lambda: L.backward_weights(x, dy, feeds_instance_norm=True)}
            row = {'layer': name, 'kind': kind, 'taps': L.taps, 'plane': hi, 'channels_hi': chi, 'channels_lo': clo}
            for mode, fn in modes.items():
                for _ in range(3):
                    _region(torch, fn)
                row[mode + '_us'] = round(statistics.median(_region(torch, fn) for _ in range(7)), 2)
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--only', default=None, help='one configuration: ' + ', '.join(c[0] for c in CONFIGS))
    ap.add_argument('--no-launches', action='store_true')
    ap.add_argument('--no-steps', action='store_true')
    args = ap.parse_args()
    import torch
    from video_prediction_amd import kernels as K
    K.set_conv_precision('bf16')
    table = os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json')
    if os.path.exists(table):
        K.load_tuning(table)
    if not args.no_steps:
        for name, over in CONFIGS:
            if args.only in (None, name):
                time_steps(args, torch, K, name, over)
    if not args.no_launches:
        time_launches(torch, K)


if __name__ == '__main__':
    main()

"""Step time of the c2-shaped bf16 train step (BAIR 64x64x3, B = 16, T = 30, ours_savp recipe, replayed hipGraph, after warm-up) for the
normaliser combinations: the default (instance, instance) and the three with a layer norm.  Prints one JSON line per combination.

    python tests/tools/time_layer_norm.py [--steps 10] [--warmup 3] [--only layer,layer]

Under `rocprofv3 --kernel-trace --stats -- python tests/tools/time_layer_norm.py --only layer,layer --steps 2` the kernel statistics
show the per-kernel time of the group-norm (gn_*) and ln_lstm (ll_*) kernels."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COMBOS = [('instance', 'instance'), ('layer', 'instance'), ('instance', 'layer'), ('layer', 'layer')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', default=None, help='one combination, e.g. layer,layer')
    args = ap.parse_args()
    import torch
    from bench import make_hparams, synthetic_batch
    from video_prediction_amd import kernels as K
    from video_prediction_amd.models.savp_model import SAVPEngine
    combos = [tuple(args.only.split(','))] if args.only else COMBOS
    dev = torch.device('cuda:0')
    for nl, cl in combos:
        K.set_conv_precision('bf16')
        table = os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json')
        if os.path.exists(table):
            K.load_tuning(table)
        model = make_hparams(16, over=dict(norm_layer=nl, conv_rnn_norm_layer=cl))
        eng = SAVPEngine(model.hparams, (64, 64, 3), 16, mode='train', seed=4, device=str(dev))
        eng.set_images(synthetic_batch(16, 1234, dev))
        info = None
        for _ in range(args.warmup):
            info = eng.train_step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            info = eng.train_step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({'norm_layer': nl, 'conv_rnn_norm_layer': cl, 'ms_per_step': dt / args.steps * 1e3, 'steps': args.steps,
                          'warmup': args.warmup, 'graph': eng.graph is not None,
                          'losses': {'d_loss': float(info['d_loss']), 'g_loss': float(info['g_loss'])}}), flush=True)
        del eng
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

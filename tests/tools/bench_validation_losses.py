#!/usr/bin/env python
"""Measure what scripts/train.py's validation summaries cost on the GPU (profiles/validation_losses.md):

  * one SAVPEngine.eval_losses() -- the forward-only losses of the validation batch -- against one train step of the same engine, at
    bench.py's c2 workload (BAIR 64x64x3, T = 30, B = 16, the ours_savp recipe, bf16 datapath and shipped tuning table like the bench
    default).  The step is timed the way a training job runs it (a replayed hipGraph), eval_losses the way the runner calls it (eager,
    between two replays), and the two alternate inside one loop;
  * one accumulated-evaluation update of the long model -- a mode='test' model at T = 30, B = 8 that reads the training model's variables
    (build_graph(share_with=...)), --samples prior samples per batch (100: the reference's eval_num_samples).

    python tests/tools/bench_validation_losses.py [--reps 10] [--warmup 3] [--samples 100] [--batches 2]

Times are host clocks around work that ends in a device synchronise.  Prints one JSON line.  Needs a GPU: there is no CPU path."""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--batches', type=int, default=2, help='timed validation batches of the long model (after one untimed batch)')
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_validation_losses.py needs a GPU')
    import bench
    from video_prediction_amd import kernels as K
    dev = 'cuda:0'
    cfg = bench.CONFIGS['c2']
    K.set_conv_precision('bf16')
    K.enable_autotune(True)
    table = os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json')
    if os.path.exists(table):
        K.load_tuning(table)
    B, T, shape = cfg['batch'], cfg['seq'], cfg['shape']
    model = bench.make_hparams(B, T, cfg['context'], cfg['over'])
    train = {'images': bench.synthetic_batch(B, 1234, dev, T, shape)}
    val = {'images': bench.synthetic_batch(B, 4321, dev, T, shape)}
    model.build_graph(train, device=dev)
    eng = model.engine

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def losses():
        eng.set_images(val)
        eng.eval_losses()
        eng.set_images(train)

    for _ in range(args.warmup):                    # eager step, capture, replays; every conv problem of both passes tuned
        model.train_step(train)
        losses()
    assert eng.graph is not None, 'the train step was not captured'
    t_step, t_loss = [], []
    for _ in range(args.reps):
        t_step.append(sync_time(eng.train_step))
        t_loss.append(sync_time(losses))
    med = lambda v: sorted(v)[len(v) // 2]
    out = {'workload': 'c2: %s, seq=%d, batch=%d, bf16' % (cfg['name'], T, B), 'reps': args.reps,
           'train_step_ms': {'median': med(t_step), 'min': min(t_step), 'submission': 'hipGraph replay'},
           'eval_losses_ms': {'median': med(t_loss), 'min': min(t_loss), 'submission': 'eager, staging the validation batch and back'},
           'eval_losses_over_step': med(t_loss) / med(t_step)}

    # the long model at the BAIR recipe: T = 30 on a model trained at T = 12 in the recipe; here the c2 model's variables serve (the
    # variables do not depend on the sequence length), at half the per-GPU batch
    from video_prediction_amd.models import get_model_class
    Bl = max(1, B // 2)
    hp = dict(model.hparams.values(), sequence_length=T)
    long_model = get_model_class('savp')(mode='test', hparams_dict=hp, eval_num_samples=args.samples)
    batches = [{'images': bench.synthetic_batch(Bl, 999 + i, dev, T, shape)} for i in range(args.batches + 1)]
    long_model.build_graph(batches[0], device=dev, share_with=model)
    long_model.accum_eval_reset()
    first = sync_time(lambda: long_model.accum_eval_update(batches[0]))        # eager unroll, capture: not steady state
    t_upd = [sync_time(lambda b=b: long_model.accum_eval_update(b)) for b in batches[1:]]
    vals = {k: float(v) for k, v in long_model.accum_eval_summary_fn().items()}
    out['long_model'] = {'sequence_length': T, 'batch': Bl, 'samples': args.samples, 'first_update_ms': first,
                         'update_ms': {'median': med(t_upd), 'min': min(t_upd), 'n': len(t_upd)},
                         'ms_per_sample_unroll': med(t_upd) / args.samples, 'accum_eval_psnr/avg': vals.get('accum_eval_psnr/avg')}
    step_after = sync_time(eng.train_step)          # the captured step still replays behind the long model's passes
    out['train_step_ms_after_long_eval'] = step_after
    print(json.dumps(out))


if __name__ == '__main__':
    main()

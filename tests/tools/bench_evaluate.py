"""Best-of-N evaluation time per batch (eval_outputs_and_metrics_fn, base_model.py:132-227; scripts/evaluate.py) at the reference's
evaluation protocols: num_samples prior samples drawn one unroll at a time (parallel_iterations S = 1) against S samples per unroll of the
S*B generator with the fused metric + fold kernel, captured as one hipGraph per chunk (S = 10, evaluate.py's default).  Each S gets one
untimed warm-up batch (live conv tuning of problems the tables lack, kernel loading, graph capture), then `--repeats` timed batches.
One JSON line on stdout.
usage: bench_evaluate.py [--protocol bair|kth] [--samples 100] [--S 10] [--repeats 2] [--precision bf16|f32] [--save-tuning PATH]
  --save-tuning: write the problems tuned live in this run (save_tuning's format) for merging into tuning_gfx950_<precision>.json
  bair: B = 8, 64x64x3, sequence_length 30 (evaluate_all.sh: --dataset_hparams sequence_length=30 --batch_size 8)
  kth : B = 1, 64x64x1, sequence_length 40 (--dataset_hparams sequence_length=40 --batch_size 1)"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
import bench as B
from video_prediction_amd import kernels as K, lib
from video_prediction_amd.models.savp_model import SAVPEngine

PROTOCOLS = {'bair': dict(config='c2', batch=8, seq=30), 'kth': dict(config='c4', batch=1, seq=40)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--protocol', choices=sorted(PROTOCOLS), default='bair')
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--S', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--precision', default='bf16')
    ap.add_argument('--save-tuning', default=None)
    args = ap.parse_args()
    pr = PROTOCOLS[args.protocol]
    cfg = B.CONFIGS[pr['config']]
    dev = torch.device('cuda:0')
    K.set_conv_precision(args.precision)
    K.enable_autotune(True)
    table = os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_%s.json' % args.precision)
    if os.path.exists(table):
        K.load_tuning(table)
    hp = B.make_hparams(pr['batch'], pr['seq'], cfg['context'], cfg['over']).hparams
    eng = SAVPEngine(hp, cfg['shape'], pr['batch'], mode='test', seed=4, device=str(dev))
    eng.set_images(B.synthetic_batch(pr['batch'], 1234, dev, pr['seq'], cfg['shape']))
    out = {}
    for S in (1, args.S):
        tuned0 = len(K.AUTOTUNE['log'])
        t0 = time.perf_counter()
        eng.eval_outputs_and_metrics(args.samples, parallel_iterations=S)
        torch.cuda.synchronize()
        warm = time.perf_counter() - t0
        times = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            eng.eval_outputs_and_metrics(args.samples, parallel_iterations=S)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out[S] = {'ms_per_batch': [round(t * 1e3, 2) for t in times], 'warmup_ms': round(warm * 1e3, 1),
                  'conv_problems_tuned_live': len(K.AUTOTUNE['log']) - tuned0,
                  'tuned_live': [[repr(k), list(v)] for k, v in K.AUTOTUNE['log'][tuned0:]]}
    best = {S: min(v['ms_per_batch']) for S, v in out.items()}
    if args.save_tuning:
        with open(args.save_tuning, 'w') as f:
            json.dump({k: v for S in out for k, v in out[S]['tuned_live']}, f, indent=0, sort_keys=True)
    print(json.dumps({'metric': 'best-of-%d evaluation, one batch, %s' % (args.samples, args.protocol), 'unit': 'ms',
                      'S1_ms': best[1], 'S%d_ms' % args.S: best[args.S], 'speedup': best[1] / best[args.S], 'dtype': args.precision,
                      'batch': pr['batch'], 'sequence_length': pr['seq'], 'shape': cfg['shape'], 'source_id': lib.source_id(),
                      'runs': {str(k): v for k, v in out.items()}}))


if __name__ == '__main__':
    main()

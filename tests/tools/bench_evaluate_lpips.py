"""Cost of the LPIPS metric and eval_diversity in the best-of-N evaluation (eval_outputs_and_metrics with parallel_iterations = S, one
captured hipGraph per chunk): bench_evaluate.py's protocols and timing, once without and once with LPIPS weights configured, in one
process.  The weights are seeded random ones (tests/oracle_lpips.make_weights: the time does not depend on the values).  Each engine gets
one untimed warm-up batch (live conv tuning, kernel loading, graph capture), then `--repeats` timed batches, the two engines alternating.
One JSON line on stdout; the added cost per predicted future frame is the figure of merit.
usage: bench_evaluate_lpips.py [--protocol bair|kth] [--samples 100] [--S 10] [--repeats 2] [--precision bf16|f32] [--only plain|lpips]
  --only: build and time one of the two engines (for a kernel trace)"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench as B
from tests import oracle_lpips
from tests.tools.bench_evaluate import PROTOCOLS
from video_prediction_amd import kernels as K, lib
from video_prediction_amd.models.savp_model import SAVPEngine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--protocol', choices=sorted(PROTOCOLS), default='bair')
    ap.add_argument('--samples', type=int, default=100)
    ap.add_argument('--S', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--precision', default='bf16')
    ap.add_argument('--only', choices=('plain', 'lpips'), default=None)
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
    weights = os.path.join(tempfile.mkdtemp(prefix='bench_evaluate_lpips_'), 'lpips_seeded.npz')
    np.savez(weights, **oracle_lpips.make_weights(7))
    os.environ.pop('SAVP_LPIPS_WEIGHTS', None)
    names = [args.only] if args.only else ['plain', 'lpips']
    engines, out = {}, {}
    for name in names:
        eng = SAVPEngine(hp, cfg['shape'], pr['batch'], mode='test', seed=4, device=str(dev), lpips_weights=weights if name == 'lpips' else None)
        eng.set_images(B.synthetic_batch(pr['batch'], 1234, dev, pr['seq'], cfg['shape']))
        t0 = time.perf_counter()
        eng.eval_outputs_and_metrics(args.samples, parallel_iterations=args.S)
        torch.cuda.synchronize()
        engines[name] = eng
        out[name] = {'warmup_ms': round((time.perf_counter() - t0) * 1e3, 1), 'ms_per_batch': []}
    for _ in range(args.repeats):
        for name in names:
            t0 = time.perf_counter()
            engines[name].eval_outputs_and_metrics(args.samples, parallel_iterations=args.S)
            torch.cuda.synchronize()
            out[name]['ms_per_batch'].append(round((time.perf_counter() - t0) * 1e3, 2))
    frames = args.samples * pr['batch'] * (pr['seq'] - cfg['context'])          # predicted future frames of one batch
    best = {n: min(v['ms_per_batch']) for n, v in out.items()}
    res = {'metric': 'best-of-%d evaluation, one batch, %s, S=%d' % (args.samples, args.protocol, args.S), 'unit': 'ms',
           'future_frames': frames, 'dtype': args.precision, 'batch': pr['batch'], 'sequence_length': pr['seq'], 'shape': cfg['shape'],
           'source_id': lib.source_id(), 'runs': out}
    for n in names:
        res[n + '_ms'] = best[n]
        res[n + '_us_per_future_frame'] = round(1e3 * best[n] / frames, 3)
    if len(names) == 2:
        res['lpips_added_us_per_future_frame'] = round(1e3 * (best['lpips'] - best['plain']) / frames, 3)
        res['lpips_added_fraction'] = round(best['lpips'] / best['plain'] - 1.0, 4)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

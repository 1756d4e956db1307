"""norm_layer = 'none': the launches of csrc/plain_act.hip beside their instance-norm twins on the same tensors, and the c2-shaped train
step beside the default's (profiles/norm_none.md).

    python tests/tools/time_norm_none.py [--steps 10] [--warmup 3] [--repeats 5] [--no-launches] [--no-steps]

Launches: the normalised shapes of c2's ladder at N = 32 (both unrolls of B = 16): 32x32x32, 16x16x64, 8x8x128 and the merged heads'
64x64x96.  Per shape and direction the two kernels run on the SAME tensors, their timed regions alternating (events around 200 back-to-
back launches; 3 warm-up regions each, then 7 regions each, the median and the spread reported; us per launch).  Rows: forward into one
fp32 destination; backward with an fp32 dx (the exact datapath: no column sums wanted); backward with a bf16 dx (the bf16 datapath: the
plain kernel also takes its float64 column sums, the instance norm its dgamma / dbeta).  Bytes: what each entry has to move at the least.
Step times: the method of tests/tools/time_layer_choices.py (bf16 datapath, replayed hipGraph, shipped tuning table)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(32, 32, 32, 32), (32, 16, 16, 64), (32, 8, 8, 128), (32, 64, 64, 96)]
CONFIGS = [('default', {}), ('norm_layer=none', dict(norm_layer='none'))]


def _region(torch, fn, n=200):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us per launch


def _ab(torch, a, b, warm=3, reps=7):
    """Alternating regions of the two callables: (median, min, max) of each."""
    for _ in range(warm):
        _region(torch, a)
        _region(torch, b)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_region(torch, a))
        tb.append(_region(torch, b))
    return [(round(statistics.median(t), 2), round(min(t), 2), round(max(t), 2)) for t in (ta, tb)]


def time_launches(torch, K):
    dev = torch.device('cuda:0')
    for N, H, W, C in SHAPES:
        x = torch.randn(N, H, W, C, device=dev)
        dy = torch.randn(N, H, W, C, device=dev)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        mean, rstd = torch.empty(N, C, device=dev), torch.empty(N, C, device=dev)
        y = torch.empty_like(x)
        dx32, dx16 = torch.empty_like(x), torch.empty(N, H, W, C, device=dev, dtype=torch.bfloat16)
        dg, db = (torch.zeros(C, device=dev, dtype=torch.float64) for _ in range(2))
        psum = torch.zeros(N, C, device=dev, dtype=torch.float64)
        K.instnorm_act_fwd(x, gamma, beta, [y], mean, rstd, act='relu')
        elems = N * H * W * C
        rows = [
            ('fwd', 8 * elems,
             lambda: K.plain_act_fwd(x, None, [y], act='relu'),
             lambda: K.instnorm_act_fwd(x, gamma, beta, [y], mean, rstd, act='relu')),
            ('bwd_f32_dx', 12 * elems,
             lambda: K.plain_act_bwd(x, None, [dy], dx32, act='relu'),
             lambda: K.instnorm_act_bwd(x, gamma, beta, None, mean, rstd, [dy], dx32, dg, db, act='relu')),
            ('bwd_bf16_dx_sums', 10 * elems,
             lambda: K.plain_act_bwd(x, None, [dy], dx16, act='relu', psum=psum),
             lambda: K.instnorm_act_bwd(x, gamma, beta, None, mean, rstd, [dy], dx16, dg, db, act='relu')),
        ]
        for name, nbytes, plain, inorm in rows:
            (pm, plo, phi), (im, ilo, ihi) = _ab(torch, plain, inorm)
            print(json.dumps({'shape': '%dx%dx%d' % (H, W, C), 'N': N, 'row': name, 'plain_us': pm, 'plain_min_max': [plo, phi],
                              'instnorm_us': im, 'instnorm_min_max': [ilo, ihi], 'plain_over_instnorm': round(pm / im, 3),
                              'min_bytes': nbytes, 'plain_GBps_of_min_bytes': round(nbytes / pm / 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-launches', action='store_true')
    ap.add_argument('--no-steps', action='store_true')
    args = ap.parse_args()
    import torch
    from video_prediction_amd import kernels as K
    from tests.tools.time_layer_choices import time_steps
    os.environ['SAVP_NORM_NONE'] = '1'          # the opt-in of norm_layer='none'
    K.set_conv_precision('bf16')
    table = os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json')
    if os.path.exists(table):
        K.load_tuning(table)
    if not args.no_launches:
        time_launches(torch, K)
    if not args.no_steps:
        for name, over in CONFIGS:
            time_steps(args, torch, K, name, over)


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""Measure the pixel-distribution pass on the GPU (profiles/pix_distribs.md): the one-launch recurrence (csrc/pix_distribs.hip) against the
same result composed per step from the existing kernels -- savp_select, savp_cdna_apply_fwd, savp_composite_fwd -- and torch glue (slot
copies, the per-map sum and division) in the same process, at the shapes of the C2 configuration: N = 32 (16 posterior + 16 prior rows),
T1 = 29, 64 x 64, cdna with 4 kernels, previous / first image and scratch slots (M = 7), P = 1 and 2.

    python tests/tools/bench_pix_distribs.py [--reps 20] [--warmup 3]

Times are stream-event times after a warm-up; the launch and the composition alternate inside one loop.  Prints one JSON line.  Needs a
GPU: there is no CPU path."""
from __future__ import print_function

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def time_pair(fa, fb, reps, warmup):
    import torch
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        fa()
        e[1].record()
        fb()
        e[2].record()
        torch.cuda.synchronize()
        ta.append(e[0].elapsed_time(e[1]) * 1e3)
        tb.append(e[1].elapsed_time(e[2]) * 1e3)
    med = lambda v: sorted(v)[len(v) // 2]
    return med(ta), min(ta), med(tb), min(tb)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_pix_distribs.py needs a GPU')
    from video_prediction_amd import kernels as K, lib
    dev = 'cuda:0'
    T1, N, H, W, nk, M, cf = 29, 32, 64, 64, 4, 7, 2
    slots = [(lib.PIX_SLOT_TRANSFORMED, m) for m in range(nk)] + [(lib.PIX_SLOT_CURRENT, 0), (lib.PIX_SLOT_FIXED, 0), (lib.PIX_SLOT_CURRENT, 0)]
    g = torch.Generator().manual_seed(1)
    kern = torch.rand(T1, N, 25, nk, generator=g) + 0.02
    kern = (kern / kern.sum(dim=2, keepdim=True)).to(dev)
    logits = torch.zeros(T1, N, H, W, 8)
    logits[..., :M] = 2.0 * torch.randn(T1, N, H, W, M, generator=g)
    logits = logits.to(dev)
    gt = torch.zeros(T1, N, dtype=torch.int32)
    gt[:cf] = 1
    gt = gt.to(dev)
    res = {'reps': args.reps, 'shapes': {}}
    for P in (1, 2):
        pix = torch.rand(T1 + 1, N, H, W, P, generator=g) + 0.01
        pix = (pix / pix.sum(dim=(2, 3), keepdim=True)).to(dev)
        gen = torch.empty(T1, N, H, W, P, device=dev)
        tr = torch.empty(T1, N, H, W, P, M, device=dev)
        gen_c = torch.empty(T1, N, H, W, P, device=dev)
        cur = torch.empty(N, H, W, P, device=dev)
        timgs = torch.empty(N, H, W, M * P, device=dev)

        def one_launch():
            return K.pix_distribs_fwd(pix, gt, 'cdna', kern, logits, gen, slots, 1, nk, cf, 5, 5)

        def with_transformed():
            K.pix_distribs_fwd(pix, gt, 'cdna', kern, logits, gen, slots, 1, nk, cf, 5, 5, transformed=tr)

        def composed():
            for t in range(T1):
                K.select(gt[t], pix[t], gen_c[t - 1] if t else None, [cur, timgs[..., nk * P:(nk + 1) * P], timgs[..., (nk + 2) * P:(nk + 3) * P]])
                K.cdna_apply_fwd(cur, kern[t], timgs[..., :nk * P], 5, 5, nk)
                timgs[..., (nk + 1) * P:(nk + 2) * P].copy_(pix[0])
                K.composite_fwd(logits[t], timgs, gen_c[t], M=M)
                gen_c[t].div_(gen_c[t].sum(dim=(1, 2), keepdim=True))
        resident = one_launch()
        composed()
        torch.cuda.synchronize()
        diff = float((gen.double() - gen_c.double()).abs().max() / gen_c.double().abs().max())
        k_med, k_min, c_med, c_min = time_pair(one_launch, composed, args.reps, args.warmup)
        t_med, t_min, _, _ = time_pair(with_transformed, lambda: None, args.reps, args.warmup)
        res['shapes']['P%d' % P] = dict(N=N, T1=T1, H=H, W=W, P=P, M=M, lds_resident=bool(resident), workgroups=N * P,
                                        max_rel_diff_to_composed=diff, one_launch_us_median=round(k_med, 1), one_launch_us_min=round(k_min, 1),
                                        with_transformed_us_median=round(t_med, 1), with_transformed_us_min=round(t_min, 1),
                                        composed_us_median=round(c_med, 1), composed_us_min=round(c_min, 1),
                                        composed_launches_per_pass=T1 * 6)
    print(json.dumps(res))


if __name__ == '__main__':
    main()

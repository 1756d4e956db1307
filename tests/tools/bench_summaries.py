#!/usr/bin/env python
"""Measure the summary path on the GPU (profiles/summaries.md): the board kernel (csrc/summary.hip) against the same board composed from
torch ops in the same process, at the shapes of the C2 configuration (64x64x3, batch 16 = 8 posterior + 8 prior rows, 29 steps, 7 masks),
and the wall time of one full image summary split into GPU work, device -> host copy and GIF encoding.

    python tests/tools/bench_summaries.py [--reps 50] [--warmup 5] [--no-model]

Times are stream-event times of back-to-back launches after a warm-up; kernel and torch composition alternate inside one loop.  Prints one
JSON line.  Needs a GPU: there is no CPU path."""
from __future__ import print_function

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def torch_board(view):
    """The board from torch ops: slice (the caller's view), permute / mul / clamp / to(uint8) / cat."""
    import torch
    x = view.mul(255.5).clamp(0, 255).to(torch.uint8)
    if x.dim() == 6:
        x = torch.cat(x.unbind(-1), dim=2)              # [T, n, M * H, W, C]
    return torch.cat(x.unbind(1), dim=2)                # [T, M * H, n * W, C]


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
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-model', action='store_true')
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_summaries.py needs a GPU')
    from video_prediction_amd import kernels as K, summaries as S
    dev = 'cuda:0'
    T1, N, H, W, C, M, ngf = 29, 16, 64, 64, 3, 7, 32
    lo, n = 8, 8
    rowc = (ngf + M * C + 7) // 8 * 8
    g = torch.Generator().manual_seed(1)
    maskin = (torch.rand(T1, N, H, W, rowc, generator=g) * 1.5 - 0.25).to(dev)
    masks = torch.rand(T1, N, H, W, M, generator=g).to(dev)
    gen = (torch.rand(T1, N, H, W, C, generator=g) * 1.5 - 0.25).to(dev)
    views = {
        'transformed_images': maskin[..., ngf:ngf + M * C].unflatten(-1, (M, C)).transpose(-1, -2)[:, lo:lo + n],
        'masks': masks.reshape(T1, N, H, W, 1, M)[:, lo:lo + n],
        'gen_images': gen[:, lo:lo + n],
    }
    res = {'shapes': {}, 'reps': args.reps}
    for name, v in views.items():
        out = torch.empty(T1, (v.shape[5] if v.dim() == 6 else 1) * H, n * W, v.shape[4], dtype=torch.uint8, device=dev)
        same = bool(torch.equal(K.summary_board_u8(v, out), torch_board(v)))
        k_med, k_min, t_med, t_min = time_pair(lambda: K.summary_board_u8(v, out), lambda: torch_board(v), args.reps, args.warmup)
        nbytes = out.numel() * 5                                        # 4 bytes read + 1 written per output byte
        res['shapes'][name] = dict(shape=list(v.shape), board_bytes=out.numel(), equal_to_torch=same, kernel_us_median=round(k_med, 1),
                                   kernel_us_min=round(k_min, 1), torch_us_median=round(t_med, 1), torch_us_min=round(t_min, 1),
                                   kernel_GBps=round(nbytes / k_med / 1e3, 1))
    if not args.no_model:
        from video_prediction_amd.models import get_model_class
        B, T = 8, 30
        m = get_model_class('savp')(mode='test', hparams_dict=dict(context_frames=2, sequence_length=T))
        images = torch.rand(B, T, H, W, C, generator=g).to(dev)
        m.build_graph({'images': images})
        xfer = S.BoardTransfer()
        parts = []
        for _ in range(3):                                               # the first pass tunes / loads kernels: report the last
            torch.cuda.synchronize()
            t0 = time.time()
            boards = m.image_summary_fn({'images': images})
            torch.cuda.synchronize()
            t1 = time.time()
            host = xfer.to_host(boards)
            t2 = time.time()
            gifs = {k: S.encode_gif(b, S.GIF_FPS) for k, b in host.items()}
            t3 = time.time()
            parts.append((t1 - t0, t2 - t1, t3 - t2))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        eng = m.engine
        e0.record()
        K.summary_board_u8(eng.images_tm[:, :B])
        for k, v in eng.output_views().items():
            K.summary_board_u8(v[:, :B])
        e1.record()
        torch.cuda.synchronize()
        res['image_summary'] = dict(batch=B, frames=T, boards=len(boards), board_bytes=sum(int(b.size) for b in host.values()),
                                    gif_bytes=sum(len(x) for x in gifs.values()), gpu_forward_and_boards_ms=round(parts[-1][0] * 1e3, 2),
                                    boards_only_ms=round(e0.elapsed_time(e1), 3), d2h_ms=round(parts[-1][1] * 1e3, 2),
                                    gif_encode_ms=round(parts[-1][2] * 1e3, 1))
    print(json.dumps(res))


if __name__ == '__main__':
    main()

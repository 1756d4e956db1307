"""The LPIPS stem kernel (savp_lpips_stem: affine + 11x11/4 conv + bias + ReLU) against the generic implicit-GEMM kernel of savp_conv on
the same convolution, frames = 28 x 8 x 10 (the future frames of one BAIR evaluation chunk), at 64x64 and 128x128.  The generic path gets
its input already scaled (the affine pass it would need is NOT in its time) and its tile / split-K from the live tuner.  The two are timed
alternately with device events, `--reps` launches per window, `--rounds` windows each; results agree to float32 rounding (checked).
One JSON line per shape on stdout.  Achieved FLOP/s = 2 * pixels * 363 * 64 over the kernel's time, against the 157.3 TF fp32 MFMA peak.
usage: bench_lpips_stem.py [--frames 2240] [--reps 20] [--rounds 5]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from tests import oracle_lpips as OL
from video_prediction_amd import kernels as K, lib
from video_prediction_amd.lpips import Lpips

PEAK_F32 = 157.3e12


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=28 * 8 * 10)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    dev = 'cuda:0'
    w = OL.make_weights(7)
    net = Lpips(w, dev)
    K.enable_autotune(True)
    N = args.frames
    for H in (64, 128):
        Ho = (H + 4 - 11) // 4 + 1
        g = torch.Generator().manual_seed(H)
        frames = torch.rand(1, N, H, H, 3, generator=g).to(dev)
        scaled = torch.as_tensor(OL.preprocess(frames[0].cpu().numpy()).astype(np.float32)).to(dev)
        src = torch.as_tensor(w['conv1_w']).to(dev)
        wt = torch.empty(src.numel(), device=dev)
        K.pack_weights(src, wt=wt)
        y_stem, y_gen = torch.empty(N, Ho, Ho, 64, device=dev), torch.empty(N, Ho, Ho, 64, device=dev)
        geom = K.ConvGeom((11, 11), (4, 4), (2, 2))
        stem = lambda: K.lpips_stem(frames, net.stem_w, net.bias[0], y_stem)
        generic = lambda: K.conv(lib.CONV_FPROP, geom, scaled, y_gen, wt, bias=net.bias[0], act=lib.ACT_LRELU, alpha=0.0, precision=0)
        stem(); generic(); stem(); generic()                                 # code objects, the tuner's choice
        torch.cuda.synchronize()
        diff = float((y_stem - y_gen).abs().max() / y_gen.abs().max())
        ts, tg = [], []
        for _ in range(args.rounds):
            ts.append(window(stem, args.reps))
            tg.append(window(generic, args.reps))
        flop = 2.0 * N * Ho * Ho * 363 * 64
        best_s, best_g = min(ts), min(tg)
        cfg = [list(v) for k, v in K.AUTOTUNE['log'] if k[4] == H and k[5] == H and k[11] == (1, 11, 11)]
        print(json.dumps({'shape': [H, H, 3], 'frames': N, 'stem_us': [round(t, 1) for t in ts], 'generic_us': [round(t, 1) for t in tg],
                          'stem_best_us': round(best_s, 1), 'generic_best_us': round(best_g, 1), 'speedup': round(best_g / best_s, 2),
                          'stem_tflops': round(flop / best_s / 1e6, 2), 'generic_tflops': round(flop / best_g / 1e6, 2),
                          'stem_share_of_fp32_peak': round(flop / (best_s * 1e-6) / PEAK_F32, 3), 'generic_tile_splitk': cfg,
                          'max_rel_diff': diff, 'source_id': lib.source_id()}), flush=True)


if __name__ == '__main__':
    main()

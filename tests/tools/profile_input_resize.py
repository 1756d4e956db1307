"""Launch sequence for the kernel-time comparison in profiles/input_resize.md: in ONE process and alternating, warm,

  (a) u8_frames_kernel          uint8 [16, 30, 128, 128, 3] -> float32 [30, 16, 128, 128, 3]   (the plain conversion: the yardstick)
  (b) u8_frames_resize_kernel   uint8 [16, 30,  64,  64, 3] -> float32 [30, 16, 128, 128, 3]   (bilinear, scale_size=128)
  (c) u8_frames_resize_kernel   uint8 [16, 30, 128, 128, 3] -> float32 [30, 16,  64,  64, 3]   (area, scale_size=64)

Run it under the profiler, in a run of its own, and read the per-kernel averages from the stats file:

    rocprofv3 --kernel-trace --stats -d <dir> -o input_resize --output-format csv -- python tests/tools/profile_input_resize.py --launches 60

Without the profiler it prints one JSON line: the bytes each kernel moves (computed from the shapes) and device-event times per launch
(launch gaps included, so an upper bound of the kernel time)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    import torch
    from video_prediction_amd import kernels as K
    if not torch.cuda.is_available():
        raise SystemExit('profile_input_resize.py needs an MI355X')
    B, T, C = 16, 30, 3
    g = torch.Generator().manual_seed(0)
    u128 = torch.randint(0, 256, (B, T, 128, 128, C), dtype=torch.uint8, generator=g).cuda()
    u64 = torch.randint(0, 256, (B, T, 64, 64, C), dtype=torch.uint8, generator=g).cuda()
    o128 = torch.empty(T, B, 128, 128, C, device='cuda')
    o64 = torch.empty(T, B, 64, 64, C, device='cuda')
    cases = (('a_plain_128', lambda: K.u8_frames_to_f32(u128, o128), u128, o128),
             ('b_bilinear_64_to_128', lambda: K.u8_frames_resize_f32(u64, o128, 64), u64, o128),
             ('c_area_128_to_64', lambda: K.u8_frames_resize_f32(u128, o64, 128), u128, o64))
    for _ in range(args.warmup):
        for _, fn, _, _ in cases:
            fn()
    torch.cuda.synchronize()
    ev = {name: [] for name, _, _, _ in cases}
    for _ in range(args.launches):
        for name, fn, _, _ in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for name, _, src, dst in cases:
        us = sorted(1e3 * a.elapsed_time(b) for a, b in ev[name])
        out[name] = dict(bytes_read=src.numel(), bytes_written=4 * dst.numel(), event_us_median=round(us[len(us) // 2], 2),
                         event_us_min=round(us[0], 2))
    print(json.dumps(dict(launches=args.launches, cases=out)))


if __name__ == '__main__':
    main()

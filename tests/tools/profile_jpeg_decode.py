"""Measurements behind profiles/jpeg_decode.md: 240 frames (B = 16, T = 15) of 512 x 640, 4:2:0, photograph-like content, quality 90, encoded
here with Pillow and written as google_robot records into a temporary directory.

  --mode kernel   entropy-decode the batch once on the host, then launch savp_jpeg_decode_u8 --launches times.  Run it under the profiler,
                  in a run of its own, and read the per-kernel averages from the stats file:
                      rocprofv3 --kernel-trace --stats -d <dir> -o jpeg_decode --output-format csv -- \\
                          python tests/tools/profile_jpeg_decode.py --mode kernel --launches 40
                  Without the profiler it prints device-event times per call (both kernels + launch gap: an upper bound).
  --mode host     no GPU: frames/s of the host entropy decoder inside the pipeline (savp_pipeline_next_jpeg) with 1, 4 and 16 worker threads,
                  and of Pillow's full decode (libjpeg-turbo; Image.load releases the GIL) on a pool of as many threads.
  --mode pipeline the GoogleRobotVideoDataset iterator end to end (records -> float32 [16, 15, 64, 64, 3] on the device, crop_size=512,
                  scale_size=64) with SAVP_DECODE_THREADS = 1, 4, 16: frames/s.
Every mode prints one JSON line with the byte counts computed from the shapes."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, H, W = 16, 15, 512, 640
FMT = 'move/%d/image/encoded'


def photo(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6, 3)
    img = np.stack([127 + 90 * np.sin(0.013 * xx * (k + 1) + ph[k]) * np.cos(0.011 * yy + k) + 50 * (((xx + 2 * yy) // 37 + k) % 3 == 0)
                    for k in range(3)], -1)
    return np.clip(np.rint(img + rng.normal(0, 5, img.shape)), 0, 255).astype(np.uint8)


def make_records(d, distinct=24):
    """16 examples of 15 frames from `distinct` different images (encoding 240 different ones changes nothing for any figure here)."""
    from PIL import Image
    from oracle import tfrecord as R
    rng = np.random.default_rng(0)
    streams = []
    for _ in range(distinct):
        buf = io.BytesIO()
        Image.fromarray(photo(rng, H, W)).save(buf, 'JPEG', quality=90, subsampling=2)
        streams.append(buf.getvalue())
    os.makedirs(d)
    exs = [R.encode_example({FMT % t: streams[(7 * i + t) % distinct] for t in range(T)}) for i in range(B)]
    path = os.path.join(d, 'push_train.tfrecord-00000-of-00001')
    R.write_records(path, exs)
    return [path], streams


def mode_host(paths, streams, batches):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from video_prediction_amd import io as sio
    out = {'jpeg_bytes_per_frame': int(np.mean([len(s) for s in streams]))}

    def pil(s):
        im = Image.open(io.BytesIO(s))
        im.load()
        return im.size

    for n in (1, 4, 16):
        pipe = sio.VideoPipeline(paths, FMT, T, (H, W, 3), T, B, jpeg=True, decode_threads=n, num_epochs=batches + 1)
        coef, qtab = np.empty(pipe.coef_shape, np.int16), np.empty(pipe.qtab_shape, np.uint16)
        pipe.next_jpeg(coef, qtab)
        t0 = time.perf_counter()
        for _ in range(batches):
            assert pipe.next_jpeg(coef, qtab) is not None
        out['entropy_decode_fps_%d_threads' % n] = round(batches * B * T / (time.perf_counter() - t0), 1)
        pipe.close()
        work = [streams[k % len(streams)] for k in range(B * T)]
        with ThreadPoolExecutor(n) as ex:
            list(ex.map(pil, work[:n * 2]))
            t0 = time.perf_counter()
            for _ in range(batches):
                list(ex.map(pil, work))
            out['pillow_full_decode_fps_%d_threads' % n] = round(batches * B * T / (time.perf_counter() - t0), 1)
    return out


def mode_kernel(paths, launches):
    import torch
    from video_prediction_amd import io as sio, kernels as K
    pipe = sio.VideoPipeline(paths, FMT, T, (H, W, 3), T, B, jpeg=True, decode_threads=16)
    coef, qtab, _, _ = pipe.next_jpeg()
    info = pipe.jpeg_info
    pipe.close()
    dc = torch.from_numpy(coef).cuda()
    dq = torch.from_numpy(qtab.view(np.int16)).cuda()
    out = torch.empty((B, T, H, W, 3), dtype=torch.uint8, device='cuda')
    ws = torch.empty(K.jpeg_workspace_bytes(info, B * T), dtype=torch.uint8, device='cuda')
    for _ in range(3):
        K.jpeg_decode_u8(dc, dq, info, out, ws)
    torch.cuda.synchronize()
    ev = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        K.jpeg_decode_u8(dc, dq, info, out, ws)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    return dict(launches=launches, frames=B * T, coef_bytes=dc.numel() * 2, qtab_bytes=dq.numel() * 2, plane_bytes=ws.numel(), out_bytes=out.numel(),
                nonzero_coef_fraction=round(float((coef != 0).mean()), 4), event_us_median=round(us[len(us) // 2], 1), event_us_min=round(us[0], 1))


def mode_pipeline(d, batches):
    import torch
    from video_prediction_amd.datasets import get_dataset_class
    out = {}
    for n in (1, 4, 16):
        os.environ['SAVP_DECODE_THREADS'] = str(n)
        ds = get_dataset_class('google_robot')(d, mode='test', num_epochs=batches + 2, hparams='crop_size=512,scale_size=64')
        it = ds.make_batch(B)
        for _ in range(2):
            x = next(it)['images']
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            x = next(it)['images']
        torch.cuda.synchronize()
        out['pipeline_fps_%d_threads' % n] = round(batches * B * T / (time.perf_counter() - t0), 1)
        assert tuple(x.shape) == (B, T, 64, 64, 3)
        it.pipe.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('kernel', 'host', 'pipeline'), required=True)
    ap.add_argument('--launches', type=int, default=40)
    ap.add_argument('--batches', type=int, default=6)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, 'push_train')
        paths, streams = make_records(d)
        if args.mode == 'host':
            res = mode_host(paths, streams, args.batches)
        elif args.mode == 'kernel':
            res = mode_kernel(paths, args.launches)
        else:
            res = mode_pipeline(d, args.batches)
    print(json.dumps(dict(mode=args.mode, **res)))


if __name__ == '__main__':
    main()

"""SSIM kernel times at 64x64 (the plane in LDS whole) and 128x128 (strips of whole rows), and the SSIM launch's share of one parallel
evaluation chunk of the 128x128 workload (bench.py's c5).  Made to run under a kernel trace (profiles/ssim_large.md):

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT1 -- python tests/tools/bench_ssim_large.py kernels
  rocprofv3 --kernel-trace --output-format csv -d OUT2 -- python tests/tools/bench_ssim_large.py chunk
  python tests/tools/bench_ssim_large.py report OUT1/.../kernel_trace.csv OUT2/.../kernel_trace.csv

kernels: savp_eval_fold_samples at F = 28, S = 4, B = 8 and savp_frame_ssim at T = 28, B = 8, C = 3, each size `--repeats` times.
chunk  : eval_outputs_and_metrics(parallel_iterations = 4) of the c5 engine (B = 8, sequence 30, context 2, bf16 convolutions as
         tests/tools/bench_evaluate.py): one untimed warm-up (tuning, the eager chunk, graph capture), then `--repeats` chunks replayed.
report : per-window-position time of the four SSIM kernels from the first trace; from the second, the kernel time of the last replayed
         chunks (the dispatches from one fold_mse_kernel to the next) and the SSIM launch's share of it."""
import argparse, csv, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

F, S, NB, C = 28, 4, 8, 3


def kernels(repeats):
    import torch
    from video_prediction_amd import kernels as K
    dev = 'cuda:0'
    for HW in (64, 128):
        g = torch.Generator().manual_seed(HW)
        target = torch.rand(F, NB, HW, HW, C, generator=g).to(dev)
        pred = (target.repeat(1, S, 1, 1, 1) + 0.05 * torch.randn(F, S * NB, HW, HW, C, generator=g).to(dev)).clamp(0, 1)
        st = {k: dict(min=torch.full((F, NB), float('inf'), device=dev), sum=torch.zeros(F, NB, device=dev),
                      max=torch.full((F, NB), float('-inf'), device=dev), gmin=torch.zeros(F, NB, HW, HW, C, device=dev),
                      gsum=torch.zeros(F, NB, HW, HW, C, device=dev), gmax=torch.zeros(F, NB, HW, HW, C, device=dev)) for k in K.EVAL_FOLD_KEYS}
        ws = K.eval_fold_ws(F, S, NB, C, dev)
        nv = torch.tensor([S], dtype=torch.int32, device=dev)
        out = torch.empty(F, NB, device=dev)
        for _ in range(repeats + 1):
            K.eval_fold_samples(target, pred, nv, st, ws)
            K.frame_ssim(target, pred[:, :NB], out)
            torch.cuda.synchronize()
        print('%dx%d: ssim of the first frame %.6f' % (HW, HW, float(out[0, 0])))


def chunk(repeats):
    import torch
    import bench as B
    from video_prediction_amd import kernels as K
    from video_prediction_amd.models.savp_model import SAVPEngine
    cfg = B.CONFIGS['c5']
    dev = torch.device('cuda:0')
    K.set_conv_precision('bf16')
    K.enable_autotune(True)
    table = os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json')
    if os.path.exists(table):
        K.load_tuning(table)
    hp = B.make_hparams(cfg['batch'], cfg['seq'], cfg['context'], cfg['over']).hparams
    eng = SAVPEngine(hp, cfg['shape'], cfg['batch'], mode='test', seed=4, device=str(dev))
    eng.set_images(B.synthetic_batch(cfg['batch'], 1234, dev, cfg['seq'], cfg['shape']))
    eng.eval_outputs_and_metrics(2 * S, parallel_iterations=S)
    torch.cuda.synchronize()
    eng.eval_outputs_and_metrics(repeats * S, parallel_iterations=S)
    torch.cuda.synchronize()


def _rows(path):
    rows = [(r['Kernel_Name'].split('(')[0], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(open(path))]
    return sorted(rows, key=lambda r: r[1])


def report(kernel_csv, chunk_csv):
    out = {}
    per = {}
    for name, t0, t1 in _rows(kernel_csv):
        if 'ssim' in name:
            per.setdefault(name, []).append((t1 - t0) * 1e-3)
    for name, us in sorted(per.items()):
        us = sorted(us[1:])                                 # the first launch loads the code object
        med = us[len(us) // 2]
        HW = 128 if 'strip' in name else 64
        planes = F * NB * C * (S if name.startswith('fold') else 1)
        windows = planes * (HW - 10) ** 2
        out[name] = {'launches': len(us), 'median_us': round(med, 1), 'min_us': round(us[0], 1), 'max_us': round(us[-1], 1),
                     'planes': planes, 'ps_per_window': round(med * 1e6 / windows, 2)}
    if chunk_csv:
        rows = _rows(chunk_csv)
        starts = [i for i, r in enumerate(rows) if r[0] == 'fold_mse_kernel']
        chunks = []
        for i0, i1 in zip(starts[:-1], starts[1:]):         # fold .. next unroll .. up to the next fold: one chunk's worth of kernels
            seg = rows[i0:i1]
            tot = sum(t1 - t0 for _, t0, t1 in seg) * 1e-3
            ssim = sum(t1 - t0 for n, t0, t1 in seg if n.startswith('fold_ssim')) * 1e-3
            chunks.append((tot, ssim, len(seg), (rows[i1][1] - rows[i0][1]) * 1e-3))
        chunks = chunks[2:]                                 # the warm-up call's chunks: tuning and the eager chunk
        chunks.sort()
        tot, ssim, n, wall = chunks[len(chunks) // 2]
        out['chunk'] = {'chunks': len(chunks), 'kernels': n, 'kernel_time_us': round(tot, 1), 'fold_to_fold_us': round(wall, 1),
                        'ssim_us': round(ssim, 1), 'ssim_share_of_kernel_time': round(ssim / tot, 4)}
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=('kernels', 'chunk', 'report'))
    ap.add_argument('traces', nargs='*')
    ap.add_argument('--repeats', type=int, default=6)
    a = ap.parse_args()
    if a.what == 'report':
        report(a.traces[0], a.traces[1] if len(a.traces) > 1 else None)
    else:
        {'kernels': kernels, 'chunk': chunk}[a.what](a.repeats)

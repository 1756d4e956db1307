"""SSIM for frames of more than 8192 pixels (pytest -m gpu): metrics.hip walks such planes in strips of whole rows.  The single-sample kernel
and the fold against the fp64 oracle and against each other on the inputs of tests/ssim_large_cases.py, the fold against the sequential
foldl, the engine's metrics and evaluation at 128x128, scripts/train.py and scripts/evaluate.py at that size, and the refused geometries."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ssim_large_cases as SC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = 'cuda:0'


def _ssim(a, b):
    from video_prediction_amd import kernels as K
    out = torch.empty(a.shape[0], a.shape[1], device=DEV)
    K.frame_ssim(a, b, out)
    torch.cuda.synchronize()
    return out.cpu()


# 1 -- the single-sample kernel against the fp64 oracle (tolerances of tests/gpu_checks.py check_metrics: 2e-5 relative, identity 1e-5)
@pytest.mark.parametrize('shape', SC.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_frame_ssim_equals_the_oracle(shape):
    for profile in SC.PROFILES:
        a, b = SC.frames(*shape, profile)
        ref = SC.reference(*shape, profile)
        ad = a.float().to(DEV)
        got = _ssim(ad, b.float().to(DEV))
        err = float(((got.double() - ref).abs() / ref.abs()).max())
        print('%s %s: ssim %s, relative error %.3g' % (shape, profile, ref.flatten().tolist(), err))
        assert err <= SC.SSIM_RTOL, (profile, err)
        ident = float((_ssim(ad, ad) - 1).abs().max())
        assert ident <= 1e-5, (profile, ident)


def test_frame_ssim_at_the_widest_row():
    """W = 744: strips of one window row, the widest the library takes."""
    from oracle import metrics as OM
    g = torch.Generator().manual_seed(744)
    a = torch.rand(1, 2, 13, 744, 1, generator=g, dtype=torch.float64)
    b = (a + 0.1 * torch.randn(a.shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    ref = OM.ssim(a, b)
    got = _ssim(a.float().to(DEV), b.float().to(DEV))
    err = float(((got.double() - ref).abs() / ref.abs()).max())
    assert err <= SC.SSIM_RTOL, err


# 2 -- the fold's per-frame metrics against the single-sample kernels (as test_fold_per_frame_metrics_equal_the_single_sample_kernels)
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('HW', [91, 128])
def test_fold_per_frame_metrics_equal_the_single_sample_kernels(HW, C):
    from oracle import metrics as OM
    from tests.test_gpu_evaluate import _fresh_states
    from video_prediction_amd import kernels as K
    F, T1, S, B, H, W = 2, 3, 3, 2, HW, HW
    g = torch.Generator().manual_seed(50 + HW + C)
    target = torch.rand(F, B, H, W, C, generator=g)
    pred = torch.rand(T1, S * B, H, W, C, generator=g)
    # predictions near the targets (ssim ~0.9: a relative error means something there)
    pred[T1 - F:] = (target.repeat(1, S, 1, 1, 1) + 0.05 * torch.randn(F, S * B, H, W, C, generator=g)).clamp(0, 1)
    tg, pr = target.to(DEV), pred.to(DEV)
    ws = K.eval_fold_ws(F, S, B, C, DEV)
    K.eval_fold_samples(tg, pr, torch.tensor([S], dtype=torch.int32, device=DEV), _fresh_states(F, B, T1, H, W, C), ws)
    met = ws[:3 * F * S * B].view(3, F, S, B).cpu()
    for s in range(S):
        p = pr[T1 - F:, s * B:(s + 1) * B]
        mse, psnr, ssim = (torch.empty(F, B, device=DEV) for _ in range(3))
        K.frame_mse_psnr(tg, p, mse=mse, psnr=psnr)
        K.frame_ssim(tg, p, ssim)
        torch.cuda.synchronize()
        assert torch.equal(met[0, :, s], psnr.cpu()) and torch.equal(met[1, :, s], mse.cpu()), s
        if C == 1:
            assert torch.equal(met[2, :, s], ssim.cpu()), s
        else:                                              # atomics in arrival order against c = 0, 1, 2: a rounding apart
            assert torch.allclose(met[2, :, s], ssim.cpu(), rtol=4e-7, atol=0), s
        a, b = target.double(), pred[T1 - F:, s * B:(s + 1) * B].double()
        for k, fn in ((0, OM.psnr), (1, OM.mse), (2, OM.ssim)):
            r = fn(a, b)
            err = float(((met[k, :, s].double() - r).abs() / r.abs()).max())
            assert err <= 1e-5, (s, k, err)


# 3 -- the fold against the sequential foldl, exactly (as test_fold_kernel_matches_the_sequential_foldl_exactly)
def test_fold_kernel_matches_the_sequential_foldl_exactly():
    from tests.test_gpu_evaluate import _fresh_states, _np_fold, _np_states
    from video_prediction_amd import kernels as K
    F, T1, S, B, H, W, C = 3, 5, 4, 3, 96, 96, 3
    g = torch.Generator().manual_seed(13)
    target = torch.rand(F, B, H, W, C, generator=g)
    pred = torch.rand(T1, S * B, H, W, C, generator=g)
    pred[:, 2 * B + 1] = pred[:, 0 * B + 1]               # planted ties: sample 2 repeats sample 0 (b = 1) ...
    pred[:, 1 * B + 2] = pred[:, 0 * B + 2]               # ... and sample 1 repeats sample 0 (b = 2)
    pred[T1 - F:, 1 * B + 0] = target[:, 0]               # a perfect prediction: mse 0, psnr inf, ssim 1
    st = _fresh_states(F, B, T1, H, W, C)
    ref = _np_states(st)
    ws = K.eval_fold_ws(F, S, B, C, DEV)
    tg, pr = target.to(DEV), pred.to(DEV)
    for chunk, nv in enumerate((S, 3, 0)):                 # a full chunk, a padded one (n_valid < S), an empty one
        p = pr.clone()
        if chunk:
            p = torch.roll(p, shifts=B * chunk, dims=1)    # other samples in the later chunks
            p[:, nv * B:] = float('nan')                   # padding rows are never read
        n_valid = torch.tensor([nv], dtype=torch.int32, device=DEV)
        K.eval_fold_samples(tg, p, n_valid, st, ws)
        torch.cuda.synchronize()
        met = ws[:3 * F * S * B].view(3, F, S * B).cpu().numpy()
        pn = p.cpu().numpy()
        for k, name in enumerate(K.EVAL_FOLD_KEYS):
            _np_fold(ref[name], met[k], pn, nv, B)
        got = _np_states(st)
        for name in K.EVAL_FOLD_KEYS:
            for key in ('min', 'sum', 'max', 'gmin', 'gsum', 'gmax'):
                assert np.array_equal(got[name][key], ref[name][key]), (chunk, name, key)
    assert np.isinf(ref['psnr']['max']).any() and (ref['mse']['min'] == 0).any()     # the perfect sample won
    assert (ref['ssim']['max'] == 1).any()


# 4 -- two launches on the same input
@pytest.mark.parametrize('C', [1, 3])
def test_two_launches_give_the_same_bits(C):
    from tests.test_gpu_evaluate import _fresh_states, _np_states
    from video_prediction_amd import kernels as K
    F, T1, S, B, H, W = 2, 3, 3, 2, 128, 128
    a, b = SC.frames(H, W, C, 'bump')
    g = torch.Generator().manual_seed(60 + C)
    target = a.float().expand(F, B, H, W, C).contiguous()
    pred = (target.repeat(T1 // F + 1, S, 1, 1, 1)[:T1] + 0.1 * torch.randn(T1, S * B, H, W, C, generator=g)).clamp(0, 1)
    tg, pr = target.to(DEV), pred.to(DEV)
    runs = []
    for _ in range(2):
        st = _fresh_states(F, B, T1, H, W, C)
        ws = K.eval_fold_ws(F, S, B, C, DEV)
        K.eval_fold_samples(tg, pr, torch.tensor([S], dtype=torch.int32, device=DEV), st, ws)
        torch.cuda.synchronize()
        runs.append((ws[:3 * F * S * B].cpu().numpy().copy(), _np_states(st)))
    assert np.array_equal(runs[0][0], runs[1][0])
    for name in K.EVAL_FOLD_KEYS:
        for key, v in runs[0][1][name].items():
            assert np.array_equal(v, runs[1][1][name][key]), (name, key)
    if C == 1:                                             # one share per frame: nothing for the atomics to reorder
        p = pr[T1 - F:, :B]
        assert torch.equal(_ssim(tg, p), _ssim(tg, p))


# 5 -- the engine at 128x128
def test_engine_metrics_and_evaluation_at_128():
    from oracle import metrics as OM
    from tests.test_gpu_evaluate import _compare, _engine, _per_sample_means
    eng, noises = _engine(False, B=2, T=6, H=128, W=128, C=1)
    noises = noises[:5]
    F = eng.T - eng.hp.context_frames
    gen = eng.generate(noises[0])
    got = float(eng.metrics(gen)['ssim'])
    torch.cuda.synchronize()
    ref = float(OM.ssim(eng.images_tm[eng.T - F:].double().cpu(), gen[eng.T1 - F:, eng.B:].double().cpu()).mean())
    assert abs(got - ref) / abs(ref) <= 2e-5, (got, ref)
    seq = eng.eval_outputs_and_metrics(5, noises)
    seq = ({k: v.clone() for k, v in seq[0].items()}, {k: v.clone() for k, v in seq[1].items()})
    runs = []
    for _ in range(3):                                     # eager first chunk + capture, then replays only
        o, m = eng.eval_outputs_and_metrics(5, noises, parallel_iterations=2)        # chunks of 2, 2, 1 (padded)
        runs.append(({k: v.clone() for k, v in o.items()}, {k: v.clone() for k, v in m.items()}))
    torch.cuda.synchronize()
    # at least half of the 12 selections (metric x sequence x min / max) must be decided by more than the gap, as in that file's f32 test
    _compare(seq, runs[0], _per_sample_means(eng, noises), eng, 1e-5, 1e-4, eng.B * len(eng.METRICS))
    ev = next(iter(eng._par_eval.values()))
    assert ev.graph is not None and ev.graph.segments == 1              # one hipGraph per chunk
    for half in (0, 1):
        for k in runs[0][half]:
            assert torch.equal(runs[0][half][k], runs[1][half][k]) and torch.equal(runs[1][half][k], runs[2][half][k]), k


# 6 -- the scripts at 128x128x1
def test_train_script_writes_ssim_summaries_at_128(tmp_path):
    """The run that the 128x128 recipe dies in at its first --summary_freq step without the strip kernels."""
    from tests import oracle_summaries as OS
    out = str(tmp_path / 'run')
    cmd = ['timeout', '-k', '10', '600', sys.executable, os.path.join(ROOT, 'scripts', 'train.py'), '--input_dir', 'none', '--dataset',
           'synthetic', '--synthetic_shape', '128,128,1', '--model', 'savp', '--output_dir', out, '--progress_freq', '0', '--save_freq', '0',
           '--seed', '3', '--dataset_hparams', 'sequence_length=4', '--model_hparams', 'batch_size=2,max_steps=2,nz=4,clip_length=3',
           '--summary_freq', '1', '--image_summary_freq', '0', '--eval_summary_freq', '2', '--accum_eval_summary_freq', '0']
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    rows = [json.loads(l) for l in open(os.path.join(out, 'summaries.jsonl'))]
    ev_rows = [row for row in rows if row['tag'] == 'eval_summary_1']
    assert ev_rows
    for row in ev_rows:
        for sfx in ('min', 'avg', 'max'):
            v = row['eval_ssim/' + sfx]
            assert math.isfinite(v) and -1 <= v <= 1, (sfx, v)
    ev_files = [f for f in os.listdir(out) if f.startswith('events.out.tfevents.')]
    assert len(ev_files) == 1
    scalars = {}
    for e in OS.read_events(os.path.join(out, ev_files[0]))[1:]:
        for v in e.summary.value:
            if not v.HasField('image'):
                scalars.setdefault(v.tag, []).append(v.simple_value)
    for tag in ('ssim/ssim', 'ssim_1/ssim', 'eval_ssim/eval_ssim/min', 'eval_ssim/eval_ssim/avg', 'eval_ssim/eval_ssim/max',
                'eval_ssim_1/eval_ssim/min', 'eval_ssim_1/eval_ssim/avg', 'eval_ssim_1/eval_ssim/max'):
        assert tag in scalars, (tag, sorted(scalars))
        assert all(math.isfinite(v) and -1 <= v <= 1 for v in scalars[tag]), (tag, scalars[tag])


def test_evaluate_script_at_128(tmp_path):
    """scripts/evaluate.py on a 128x128x1 checkpoint: its ssim tables equal eval_outputs_and_metrics_fn in this process (as
    test_evaluate_script_end_to_end)."""
    from scripts.train import get_dataset_class
    from tests.test_gpu_evaluate import _load_csv
    from video_prediction_amd.models import get_model_class
    T, B, shape = 6, 2, '128,128,1'
    hparams = dict(nz=8)
    ckdir = tmp_path / 'ckpt' / 'savp_128'
    ckdir.mkdir(parents=True)
    Dataset = get_dataset_class('synthetic', shape)
    ds = Dataset('unused', mode='test', seed=7, hparams='sequence_length=%d' % T)
    hpd = dict(hparams, context_frames=ds.hparams.context_frames, sequence_length=T, repeat=ds.hparams.time_shift)
    Model = get_model_class('savp')
    src = Model(mode='test', hparams_dict=hpd)
    src.build_graph(next(ds.make_batch(B, device=DEV)), seed=11)
    src.engine.step = 5
    src.save(str(ckdir / 'model-5'))
    (ckdir / 'options.json').write_text(json.dumps({'dataset': 'synthetic', 'model': 'savp'}))
    (ckdir / 'model_hparams.json').write_text(json.dumps(hparams))
    res = tmp_path / 'res'
    cmd = ['timeout', '-k', '10', '600', sys.executable, os.path.join(ROOT, 'scripts', 'evaluate.py'), '--input_dir', 'unused',
           '--checkpoint', str(ckdir / 'model-5'), '--results_dir', str(res), '--mode', 'test', '--batch_size', str(B), '--num_samples', '2',
           '--num_stochastic_samples', '3', '--eval_parallel_iterations', '2', '--dataset_hparams', 'sequence_length=%d' % T,
           '--synthetic_shape', shape]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    F = T - ds.hparams.context_frames
    model = Model(mode='test', hparams_dict=hpd, eval_num_samples=3, eval_parallel_iterations=2)
    batch = next(Dataset('unused', mode='test', seed=7, hparams='sequence_length=%d' % T).make_batch(B, device=DEV))
    model.build_graph(batch)
    model.restore(str(ckdir / 'model-5'))
    _, m = model.eval_outputs_and_metrics_fn(batch)
    for sub in ('min', 'avg', 'max'):
        rows = _load_csv(str(res / 'savp_128' / ('prediction_eval_ssim_%s' % sub) / 'metrics' / 'ssim.csv'))
        assert rows[0] == ['sample_ind'] + [str(t) for t in range(F)] + ['mean']
        assert len(rows) == 1 + 2 and all(len(row) == F + 2 for row in rows)
        got = np.array(rows)[1:, 1:-1].astype(np.float32)
        ref = m['eval_ssim/' + sub].transpose(0, 1).cpu().numpy()
        # a fresh process tunes its convolutions anew: same draws, the same kernels up to the tuner's choice
        assert np.isfinite(got).all() and np.allclose(got, ref, rtol=1e-5, atol=0), (sub, np.abs(got - ref).max())


# 7 -- refused geometries
@pytest.mark.parametrize('H,W', [(11, 800), (10, 128), (11, 745)])
def test_refused_geometries_name_the_sizes(H, W):
    from tests.test_gpu_evaluate import _fresh_states
    from video_prediction_amd import kernels as K
    from video_prediction_amd import lib
    F, T1, S, B, C = 1, 1, 1, 1, 1
    x = torch.zeros(F, B, H, W, C, device=DEV)
    out = torch.full((F, B), 7.0, device=DEV)
    with pytest.raises(ValueError) as e:
        K.frame_ssim(x, x, out)
    assert 'H=%d' % H in str(e.value) and 'W=%d' % W in str(e.value) and ('744' if H >= 11 else '11') in str(e.value)
    ws = K.eval_fold_ws(F, S, B, C, DEV)
    st = _fresh_states(F, B, T1, H, W, C)
    nv = torch.ones(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError) as e:
        K.eval_fold_samples(x, x, nv, st, ws)
    assert 'H=%d' % H in str(e.value) and 'W=%d' % W in str(e.value) and ('744' if H >= 11 else '11') in str(e.value)
    L = lib.get()
    assert L.savp_frame_ssim(None, x.data_ptr(), x.stride(0), x.stride(1), x.data_ptr(), x.stride(0), x.stride(1), F, B, H, W, C,
                             out.data_ptr()) != 0
    arr = (lib.SavpEvalFoldState * 3)()
    for k, name in enumerate(K.EVAL_FOLD_KEYS):
        a = st[name]
        arr[k] = lib.SavpEvalFoldState(*(a[key].data_ptr() for key in ('min', 'sum', 'max', 'gmin', 'gsum', 'gmax')))
    assert L.savp_eval_fold_samples(None, x.data_ptr(), x.stride(0), x.stride(1), x.data_ptr(), x.stride(0), x.stride(1), F, T1, S, B, H, W, C,
                                    nv.data_ptr(), arr, ws.data_ptr(), ws.numel()) != 0
    torch.cuda.synchronize()
    assert float(out[0, 0]) == 7.0                          # refused before anything was launched

"""Best-of-N evaluation with parallel prior sampling (pytest -m gpu): the fused metric + fold kernel (savp_eval_fold_samples) against a
numpy restatement of the reference's foldl (base_model.py:176-201) and against the single-sample kernels, the S*B prior unroll
(eval_outputs_and_metrics(parallel_iterations=S)) against the sequential path, and scripts/evaluate.py end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = 'cuda:0'


def _fresh_states(F, B, T1, H, W, C):
    shape = (T1, B, H, W, C)
    return {k: dict(min=torch.full((F, B), float('inf'), device=DEV), sum=torch.zeros(F, B, device=DEV),
                    max=torch.full((F, B), float('-inf'), device=DEV), gmin=torch.zeros(shape, device=DEV),
                    gsum=torch.zeros(shape, device=DEV), gmax=torch.zeros(shape, device=DEV)) for k in ('psnr', 'mse', 'ssim')}


def _np_states(st):
    return {k: {n: v.cpu().numpy().copy() for n, v in a.items()} for k, a in st.items()}


def _np_fold(state, met, pred, nv, B):
    """base_model.py:176-201 in float32, sample after sample: met [F, S*B] per-frame metric, pred [T1, S*B, ...] (numpy)."""
    F = met.shape[0]
    f32 = np.float32
    for s in range(nv):
        for b in range(B):
            n = s * B + b
            sm = smin = smax = f32(0)
            for t in range(F):
                sm = f32(sm + met[t, n])
                smin = f32(smin + state['min'][t, b])
                smax = f32(smax + state['max'][t, b])
            lo = f32(sm / f32(F)) < f32(smin / f32(F))
            hi = f32(sm / f32(F)) > f32(smax / f32(F))
            for t in range(F):
                if lo:
                    state['min'][t, b] = met[t, n]
                if hi:
                    state['max'][t, b] = met[t, n]
                state['sum'][t, b] = f32(state['sum'][t, b] + met[t, n])
            if lo:
                state['gmin'][:, b] = pred[:, n]
            if hi:
                state['gmax'][:, b] = pred[:, n]
            state['gsum'][:, b] = (state['gsum'][:, b] + pred[:, n]).astype(np.float32)


def _case(C, seed):
    F, T1, S, B, H, W = 3, 5, 4, 3, 16, 16
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(F, B, H, W, C, generator=g)
    pred = torch.rand(T1, S * B, H, W, C, generator=g)
    pred[:, 2 * B + 1] = pred[:, 0 * B + 1]               # planted ties: sample 2 repeats sample 0 (b = 1) ...
    pred[:, 1 * B + 2] = pred[:, 0 * B + 2]               # ... and sample 1 repeats sample 0 (b = 2)
    pred[T1 - F:, 1 * B + 0] = target[:, 0]               # a perfect prediction: mse 0, psnr inf, ssim 1
    return F, T1, S, B, H, W, target, pred


@pytest.mark.parametrize('C', [3, 1])
def test_fold_kernel_matches_the_sequential_foldl_exactly(C):
    from video_prediction_amd import kernels as K
    F, T1, S, B, H, W, target, pred = _case(C, seed=10 + C)
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


def test_fold_kernel_rejects_bad_arguments():
    from video_prediction_amd import lib
    L = lib.get()
    ws = torch.zeros(1 << 16, device=DEV)
    x = torch.zeros(4, 2, 16, 16, 3, device=DEV)
    nv = torch.ones(1, dtype=torch.int32, device=DEV)
    arr = (lib.SavpEvalFoldState * 3)()
    for k in range(3):
        arr[k] = lib.SavpEvalFoldState(*([ws.data_ptr()] * 6))
    ok = (None, x.data_ptr(), x.stride(0), x.stride(1), x.data_ptr(), x.stride(0), x.stride(1), 2, 4, 1, 2, 16, 16, 3, nv.data_ptr(), arr,
          ws.data_ptr(), ws.numel())
    for i, bad in ((1, None), (7, 0), (8, 1), (9, 0), (10, 0), (11, 10), (13, 0), (14, None), (15, None), (16, None), (17, 3)):
        args = list(ok)
        args[i] = bad
        assert L.savp_eval_fold_samples(*args) != 0, i
    arr[1] = lib.SavpEvalFoldState(ws.data_ptr(), None, ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), ws.data_ptr())
    assert L.savp_eval_fold_samples(*ok) != 0


@pytest.mark.parametrize('C', [3, 1])
def test_fold_per_frame_metrics_equal_the_single_sample_kernels(C):
    from oracle import metrics as OM
    from video_prediction_amd import kernels as K
    F, T1, S, B, H, W, target, pred = _case(C, seed=20 + C)
    # predictions near the targets (ssim ~0.9: a relative error means something there), no perfect one (psnr inf)
    g = torch.Generator().manual_seed(30 + C)
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
        else:
            # savp_frame_ssim adds the C channel shares with atomics in arrival order; the fold adds them c = 0, 1, 2: a rounding apart
            assert torch.allclose(met[2, :, s], ssim.cpu(), rtol=4e-7, atol=0), s
        a, b = target.double(), pred[T1 - F:, s * B:(s + 1) * B].double()
        for k, fn in ((0, OM.psnr), (1, OM.mse), (2, OM.ssim)):
            r = fn(a, b)
            err = float(((met[k, :, s].double() - r).abs() / r.abs()).max())
            assert err <= 1e-5, (s, k, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# parallel against sequential evaluation of one model
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine(learn_prior, B=2, T=6, H=32, W=32, C=3):
    from tests.gpu_model_checks import make_hparams, make_noise, synth
    from video_prediction_amd import variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = make_hparams(context_frames=2, sequence_length=T, nz=8, schedule_sampling='none', learn_prior=learn_prior)
    specs = V.variable_specs(hp, (H, W, C), mode='test')
    vals = V.init_variables(specs, seed=4)
    rng = np.random.default_rng(5)
    for k in vals:                                         # make the latent matter at init scale
        if 'rnn_z' in k or k.endswith('gamma'):
            vals[k] = (vals[k] + 0.3 * rng.standard_normal(vals[k].shape)).astype(np.float32)
    eng = SAVPEngine(hp, (H, W, C), B, mode='test', values=vals, device=DEV)
    eng.set_images(synth(hp, B, H, W, C, 3).float().to(DEV), time_major=True)
    noises = [make_noise(hp, B, seed=40 + i, sampling=False) for i in range(10)]
    return eng, noises


def _per_sample_means(eng, noises):
    """Time-means [samples, metric, B] of every sample's metrics, from the sequential unrolls."""
    F = eng.T - eng.hp.context_frames
    out = []
    for n in noises:
        buf = {k: torch.empty(F, eng.B, device=DEV) for k in eng.METRICS}
        eng._frame_metrics(eng.generate(n)[:, eng.B:], buf)
        out.append([buf[k].mean(0).cpu().numpy() for k in eng.METRICS])
    return np.asarray(out)


def _compare(seq, par, means, eng, tol, gap, min_checked):
    (so, sm), (po, pm) = seq, par
    for key in sm:
        err = float(((pm[key].double() - sm[key].double()).abs() / sm[key].double().abs().clamp_min(1e-30)).max())
        assert err <= tol, (key, err)
    for key in so:
        if key.endswith('/avg'):                          # the mean sequence: every sample contributes
            err = float((po[key].double() - so[key].double()).abs().max())
            assert err <= max(tol * 10, 1e-4), (key, err)
    # the chosen sample agrees wherever the best and the second-best time-means are further apart than `gap`
    checked = 0
    for mi, k in enumerate(eng.METRICS):
        for b in range(eng.B):
            v = np.sort(means[:, mi, b])
            for sfx, pair in (('min', v[:2]), ('max', v[-2:])):
                if abs(float(pair[1] - pair[0])) <= gap * max(1.0, abs(float(pair[0]))):
                    continue
                key = 'eval_gen_images_%s/%s' % (k, sfx)
                err = float((po[key][:, b].double() - so[key][:, b].double()).abs().max())
                assert err <= max(tol * 10, 1e-4), (key, b, err)
                checked += 1
    assert checked >= min_checked


@pytest.mark.parametrize('learn_prior', [False, True])
def test_parallel_matches_sequential_f32(learn_prior):
    """f32 datapath: min / avg / max metrics within 1e-5 relative; the S*B unroll differs from the 2B one only in summation order."""
    eng, noises = _engine(learn_prior)
    seq = eng.eval_outputs_and_metrics(10, noises)
    seq = ({k: v.clone() for k, v in seq[0].items()}, {k: v.clone() for k, v in seq[1].items()})
    par = eng.eval_outputs_and_metrics(10, noises, parallel_iterations=4)       # chunks of 4, 4, 2 (padded)
    torch.cuda.synchronize()
    _compare(seq, par, _per_sample_means(eng, noises), eng, 1e-5, 1e-4, eng.B * len(eng.METRICS))


@pytest.mark.parametrize('learn_prior', [False, True])
def test_parallel_matches_sequential_bf16(learn_prior):
    """bf16 datapath: the unroll's operands are rounded to bf16 and the S*B problems may tile differently from the 2B ones, so both paths
    sit within the bf16 unroll's own tolerance of each other: 5e-2 relative (the generator's bf16-vs-fp64 gate, check_model_bf16);
    selections are compared where the two best time-means are more than 5e-2 apart."""
    from video_prediction_amd import kernels as K
    K.set_conv_precision('bf16')
    try:
        eng, noises = _engine(learn_prior)
        seq = eng.eval_outputs_and_metrics(10, noises)
        seq = ({k: v.clone() for k, v in seq[0].items()}, {k: v.clone() for k, v in seq[1].items()})
        par = eng.eval_outputs_and_metrics(10, noises, parallel_iterations=4)
        torch.cuda.synchronize()
        _compare(seq, par, _per_sample_means(eng, noises), eng, 5e-2, 5e-2, 0)
    finally:
        K.set_conv_precision('f32')


def test_parallel_evaluation_is_deterministic():
    eng, noises = _engine(False)
    runs = []
    for _ in range(3):                                     # eager first chunk + capture, then replays only
        o, m = eng.eval_outputs_and_metrics(10, noises, parallel_iterations=4)
        runs.append({k: v.clone() for k, v in list(o.items()) + list(m.items())})
    torch.cuda.synchronize()
    ev = next(iter(eng._par_eval.values()))
    assert ev.graph is not None and ev.graph.segments == 1              # one hipGraph per chunk
    for k in runs[0]:
        assert torch.equal(runs[1][k], runs[2][k]), k
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_model_fn_reads_eval_parallel_iterations():
    """eval_outputs_and_metrics_fn(parallel_iterations=...) and the model's eval_parallel_iterations reach the engine."""
    from video_prediction_amd.models import get_model_class
    Model = get_model_class('savp')
    images = torch.rand(2, 5, 32, 32, 3).cuda()
    m = Model(mode='test', hparams_dict=dict(context_frames=2, sequence_length=5, nz=8), eval_num_samples=3, eval_parallel_iterations=2)
    m.build_graph({'images': images})
    m.eval_outputs_and_metrics_fn({'images': images})
    assert (2, 0) in m.engine._par_eval
    m.eval_outputs_and_metrics_fn({'images': images}, parallel_iterations=3)
    assert (3, 0) in m.engine._par_eval


# ---------------------------------------------------------------------------------------------------------------------------------
# scripts/evaluate.py end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def _load_csv(path):
    import csv
    with open(path, newline='') as f:
        rows = list(csv.reader(f, delimiter='\t', quotechar='|'))
    return rows


def test_evaluate_script_end_to_end(tmp_path):
    from scripts.evaluate import to_uint8
    from scripts.train import get_dataset_class
    from tests.test_evaluate_script import _read_png
    from video_prediction_amd.models import get_model_class
    T, B, shape = 6, 2, '32,32,3'
    hparams = dict(nz=8)
    ckdir = tmp_path / 'ckpt' / 'tiny_savp'
    ckdir.mkdir(parents=True)
    Dataset = get_dataset_class('synthetic', shape)
    ds = Dataset('unused', mode='test', seed=7, hparams='sequence_length=%d' % T)
    hpd = dict(hparams, context_frames=ds.hparams.context_frames, sequence_length=T, repeat=ds.hparams.time_shift)
    Model = get_model_class('savp')
    batches = ds.make_batch(B, device=DEV)
    first = next(batches)
    src = Model(mode='test', hparams_dict=hpd)
    src.build_graph(first, seed=11)
    src.engine.step = 5
    src.save(str(ckdir / 'model-5'))
    (ckdir / 'options.json').write_text(json.dumps({'dataset': 'synthetic', 'model': 'savp'}))
    (ckdir / 'model_hparams.json').write_text(json.dumps(hparams))
    res = tmp_path / 'res'
    cmd = ['timeout', '-k', '10', '900', sys.executable, os.path.join(ROOT, 'scripts', 'evaluate.py'), '--input_dir', 'unused',
           '--checkpoint', str(ckdir / 'model-5'), '--results_dir', str(res), '--mode', 'test', '--batch_size', str(B), '--num_samples', '4',
           '--num_stochastic_samples', '5', '--eval_parallel_iterations', '2', '--dataset_hparams', 'sequence_length=%d' % T,
           '--synthetic_shape', shape]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'prediction_eval_psnr_max psnr' in r.stdout and 'prediction_eval_ssim_max ssim' in r.stdout
    assert 'lpips and eval_diversity are not computed' in r.stdout
    out = res / 'tiny_savp'
    for f in ('options.json', 'dataset_hparams.json', 'model_hparams.json'):
        assert (out / f).exists(), f
    F = T - ds.hparams.context_frames
    # the same model, batches and draws in this process
    model = Model(mode='test', hparams_dict=hpd, eval_num_samples=5, eval_parallel_iterations=2)
    ds2 = Dataset('unused', mode='test', seed=7, hparams='sequence_length=%d' % T)
    it = ds2.make_batch(B, device=DEV)
    batch0 = next(it)
    model.build_graph(batch0)
    model.restore(str(ckdir / 'model-5'))
    want = {}
    for i, batch in enumerate((batch0, next(it))):
        o, m = model.eval_outputs_and_metrics_fn(batch)
        for k, v in list(o.items()) + list(m.items()):
            if k != 'eval_images':
                want.setdefault(k, []).append(v.transpose(0, 1).cpu().numpy())
        want.setdefault('images', []).append(batch['images'].cpu().numpy())
    want = {k: np.concatenate(v) for k, v in want.items()}
    for metric in ('psnr', 'mse', 'ssim'):
        for sub in ('max', 'avg', 'min'):
            d = out / ('prediction_eval_%s_%s' % (metric, sub))
            rows = _load_csv(str(d / 'metrics' / (metric + '.csv')))
            assert rows[0] == ['sample_ind'] + [str(t) for t in range(F)] + ['mean']
            assert len(rows) == 1 + 4 and all(len(row) == F + 2 for row in rows)
            got = np.array(rows)[1:, 1:-1].astype(np.float32)
            ref = want['eval_%s/%s' % (metric, sub)]
            # a fresh process tunes its convolutions anew: same draws, the same kernels up to the tuner's choice
            assert np.allclose(got, ref, rtol=1e-5, atol=0), (metric, sub, np.abs(got - ref).max())
            gen = want['eval_gen_images_%s/%s' % (metric, sub)]
            for i in range(4):
                for t in range(F):
                    img = _read_png(str(d / 'outputs' / ('gen_image_%05d_%02d.png' % (i, t))))
                    exp = to_uint8(gen[i, -F + t])
                    diff = np.abs(img.astype(int) - exp.astype(int))
                    assert diff.max() <= 1 and (diff == 0).mean() >= 0.999, (metric, sub, i, t)
                for t in range(ds.hparams.context_frames):
                    img = _read_png(str(d / 'inputs' / ('context_image_%05d_%02d.png' % (i, t))))
                    assert np.array_equal(img, to_uint8(want['images'][i, t]))

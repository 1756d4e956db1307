"""The training guard at model level on the GPU (pytest -m gpu): SAVPEngine(guard=True) / SAVP_GUARD=1.  A guarded step equals a plain
one while the gradients are finite; the reported norms are the norms of the gradients; a generator step whose gradient is non-finite
leaves the generator group untouched while the discriminator goes on training, where the unguarded engine ends with NaN weights; the
guarded step is captured and replayed with fresh health scalars; scripts/train.py reports, stops and leaves a finite checkpoint.

Engine: that of tests/test_gpu_layer_norm.py::_engine with the normalisers back at 'instance' -- B = 2, 64 x 64 x 3, sequence_length 12,
nz = 8, both video discriminators, cdna."""
import contextlib
import functools
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import gpu_model_checks as MC
from tests import oracle_summaries as OS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(monkeypatch, graph, guard, seed=4, **over):
    from video_prediction_amd.models.savp_model import SAVPEngine
    monkeypatch.setenv('SAVP_GRAPH', '1' if graph else '0')
    monkeypatch.delenv('SAVP_GUARD', raising=False)
    kw = dict(context_frames=2, sequence_length=12, nz=8, lr=1e-3, beta1=0.5, l1_weight=100.0, kl_weight=1.0, video_sn_gan_weight=0.1,
              video_sn_vae_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0, norm_layer='instance', conv_rnn_norm_layer='instance')
    kw.update(over)
    hp = MC.make_hparams(**kw)
    assert hp.transformation == 'cdna'
    eng = SAVPEngine(hp, (64, 64, 3), 2, mode='train', seed=seed, guard=guard)
    g = torch.Generator().manual_seed(3)
    eng.set_images(torch.rand(12, 2, 64, 64, 3, generator=g).cuda(), time_major=True)
    return eng


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _state(eng):
    return {'%s.%s' % (g, k): getattr(eng.store.groups[g], k).clone() for g in ('d', 'g') for k in ('p', 'm', 'v')}


def _health(info):
    return {k: (float(v) if k.startswith('grad_norm') else int(v)) for k, v in info['health'].items()}


def test_guard_on_equals_guard_off_while_the_gradients_are_finite(monkeypatch):
    out = {}
    for guard in (False, True):
        eng = _engine(monkeypatch, False, guard)
        assert eng.guard is guard
        assert (eng.store.groups['g'].health_state is not None) is guard and (eng.store.groups['d'].health_state is not None) is guard
        infos = [eng.train_step() for _ in range(2)]
        torch.cuda.synchronize()
        out[guard] = ([(float(i['d_loss']), float(i['g_loss'])) for i in infos], _state(eng), infos)
        del eng
    assert all('health' not in i for i in out[False][2])                 # guard off: nothing is returned
    print('losses off', out[False][0], 'on', out[True][0], 'health', [_health(i) for i in out[True][2]])
    assert out[False][0] == out[True][0]
    for k, v in out[False][1].items():
        assert torch.equal(_bits(v), _bits(out[True][1][k])) and torch.equal(v, out[True][1][k]), k
    for i in out[True][2]:
        h = _health(i)
        assert h['skipped_d'] == h['skipped_g'] == h['consecutive_d'] == h['consecutive_g'] == h['nonfinite_d'] == h['nonfinite_g'] == 0
        assert np.isfinite(h['grad_norm_d']) and np.isfinite(h['grad_norm_g']) and h['grad_norm_d'] > 0 and h['grad_norm_g'] > 0


def test_reported_norms_are_the_norms_of_the_gradients(monkeypatch):
    """return_grads=True hands out the gradients of the very step whose health entry is returned (clones taken before Adam)."""
    eng = _engine(monkeypatch, False, True)
    info = eng.train_step(return_grads=True)
    torch.cuda.synchronize()
    h = _health(info)
    for grp in ('d', 'g'):
        want = float(np.sqrt(sum(float((g.double() ** 2).sum()) for g in info[grp + '_grads'].values())))
        print(grp, 'grad norm', h['grad_norm_' + grp], 'float64 norm of the returned gradients', want)
        assert abs(h['grad_norm_' + grp] - want) <= 1e-6 * want, (grp, h, want)
    # the per-variable table: every variable that has a gradient (groups d and g; the spectral-norm u vectors of 'aux' are not trained
    # and have none) exactly once, with the norm of its gradient
    report = eng.health_report()
    names = [n for n, _, _ in report]
    store = eng.store
    assert sorted(names) == sorted(n for n in store.names() if store.group_of[n] != 'aux') and len(set(names)) == len(names)
    grads = dict(info['d_grads'], **info['g_grads'])
    for n, norm, bad in report:
        want = float(grads[n].double().norm())
        assert bad == 0 and abs(norm - want) <= 1e-6 * max(want, 1e-30), (n, norm, want)
    assert [n for n, _, _ in eng.health_report('g')] == store.groups['g'].arena.names()


def test_a_non_finite_generator_gradient_is_skipped_and_the_discriminator_trains_on(monkeypatch):
    """l1_weight = inf: the forward pass is finite, the L1 term's gradient is not.  Guarded, the generator group keeps its bits and the
    discriminator group trains; unguarded, the generator's variables are NaN after two steps."""
    eng = _engine(monkeypatch, False, True, l1_weight=float('inf'))
    s0 = _state(eng)
    for _ in range(2):
        info = eng.train_step()
    torch.cuda.synchronize()
    s2, h = _state(eng), _health(info)
    print(h)
    for k in ('g.p', 'g.m', 'g.v'):
        assert torch.equal(_bits(s2[k]), _bits(s0[k])), k
    assert h['skipped_g'] == h['consecutive_g'] == 2 and h['nonfinite_g'] > 0
    assert h['skipped_d'] == 0 and h['consecutive_d'] == 0 and h['nonfinite_d'] == 0 and np.isfinite(h['grad_norm_d'])
    assert not torch.equal(s2['d.p'], s0['d.p'])
    for k in ('d.p', 'd.m', 'd.v'):
        assert bool(torch.isfinite(s2[k]).all()), k
    assert eng.store.groups['g'].t == 2                                   # attempted steps: the host count advances
    bad = [r for r in eng.health_report('g') if r[2]]
    assert bad and int(eng.store.groups['g'].health_state[4]) == [n for n, _, _ in eng.health_report('g')].index(bad[0][0])
    del eng
    off = _engine(monkeypatch, False, False, l1_weight=float('inf'))
    for _ in range(2):
        off.train_step()
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(off.store.groups['g'].p).all())         # the contrast the guard exists for


def test_guarded_step_is_captured_and_replayed_with_fresh_health_scalars(monkeypatch):
    def run(eng, steps):
        out = []
        for _ in range(steps):
            info = eng.train_step()
            out.append((float(info['d_loss']), float(info['g_loss']), _health(info)))
        torch.cuda.synchronize()
        return out

    le = run(_engine(monkeypatch, False, True), 3)
    eg = _engine(monkeypatch, True, True)
    lg = run(eg, 3)
    assert eg.graph is not None
    spread = [max(abs(a[0] - b[0]) / max(1.0, abs(a[0])), abs(a[1] - b[1]) / max(1.0, abs(a[1]))) for a, b in zip(le, lg)]
    print('spread', spread, 'eager', le, 'replayed', lg)
    assert spread[0] <= 1e-5 and max(spread[1:]) <= 1e-4, (spread, le, lg)
    assert all(h['skipped_d'] == h['skipped_g'] == 0 for _, _, h in lg)
    # fresh: a further replay over health buffers filled with garbage writes every one of them again, and the gradient norm it reports
    # is that of the step's own gradient arena (still in place behind the step), not an earlier step's
    for grp in ('d', 'g'):
        G_ = eg.store.groups[grp]
        for t in (G_.health_sumsq, G_.health_nonfinite, G_.health_total, G_.health_ws):
            t.view(torch.uint8).fill_(0xFF)
        G_.health_state[0:2].fill_(77)
        G_.health_state[4:5].fill_(77)
    info = eg.train_step()
    torch.cuda.synchronize()
    h = _health(info)
    for grp in ('d', 'g'):
        G_ = eg.store.groups[grp]
        want = float(G_.g.double().norm())
        assert abs(h['grad_norm_' + grp] - want) <= 1e-6 * want, (grp, h, want)
        assert h['grad_norm_' + grp] != lg[-1][2]['grad_norm_' + grp]
        assert G_.health_state.cpu().tolist() == [0, 1, 0, 0, -1]
        assert bool(torch.isfinite(G_.health_sumsq).all())


def _run_train(out, monkeypatch, hparams, max_steps, summary_freq):
    """scripts/train.py in this process on the synthetic dataset at 32 x 32, batch 2, sequence 4, with two image discriminators (a second
    optimiser group at a frame size the video discriminators' pyramid does not reach).  Returns (exit status, what it printed)."""
    sys.path.insert(0, ROOT)
    from scripts import train as TR
    from video_prediction_amd import models
    orig = models.get_model_class
    monkeypatch.setattr(models, 'get_model_class', lambda name: functools.partial(orig(name), eval_num_samples=2))
    monkeypatch.setattr(TR.SyntheticVideoDataset, 'num_examples_per_epoch', lambda self: 8)
    buf, code = io.StringIO(), 0
    with contextlib.redirect_stdout(buf):
        try:
            TR.main(['--input_dir', 'none', '--dataset', 'synthetic', '--synthetic_shape', '32,32,3', '--model', 'savp', '--output_dir', out,
                     '--progress_freq', '1', '--seed', '3', '--dataset_hparams', 'sequence_length=4',
                     '--model_hparams', 'batch_size=2,max_steps=%d,nz=4,clip_length=3,image_sn_gan_weight=0.1,images_sn_vae_gan_weight=0.1%s' % (
                         max_steps, hparams),
                     '--summary_freq', str(summary_freq), '--image_summary_freq', '0', '--eval_summary_freq', '0',
                     '--accum_eval_summary_freq', '0', '--save_freq', '0'])
        except SystemExit as e:
            code = e.code
    torch.cuda.synchronize()
    return code, buf.getvalue()


def _rows(run_dir):
    with open(os.path.join(run_dir, 'summaries.jsonl')) as f:
        return [json.loads(ln) for ln in f if ln.strip()]


GUARD_SCALARS = ('grad_norm_d', 'grad_norm_g', 'skipped_steps_d', 'skipped_steps_g')


def test_runner_stops_on_repeated_skips_with_a_finite_checkpoint(tmp_path, monkeypatch):
    from video_prediction_amd.checkpoint import read_checkpoint
    monkeypatch.setenv('SAVP_GUARD', '1')
    monkeypatch.setenv('SAVP_GUARD_MAX_SKIPS', '2')
    out = str(tmp_path / 'bad')
    code, printed = _run_train(out, monkeypatch, ',l1_weight=inf', 6, 0)
    print(printed[-3000:], code)
    assert code not in (0, None)                                          # a non-zero exit status ...
    assert 'generator' in str(code) and '\n' not in str(code)             # ... with a one-line reason that names the group
    assert 'gradient report of the generator group' in printed and 'grad_norm' in printed
    assert os.path.exists(os.path.join(out, 'model-2.index'))             # tripped at the second step's progress check
    values = read_checkpoint(out)
    gen = [k for k in values if k.startswith('generator/')]
    assert len(gen) > 20 and any(k.endswith('/Adam') for k in gen)
    for k in gen:
        assert np.isfinite(np.asarray(values[k])).all(), k


def test_runner_reports_the_four_scalars_with_the_guard_and_none_without(tmp_path, monkeypatch):
    monkeypatch.setenv('SAVP_GUARD', '1')
    monkeypatch.delenv('SAVP_GUARD_MAX_SKIPS', raising=False)
    on = str(tmp_path / 'on')
    code, printed = _run_train(on, monkeypatch, '', 3, 1)
    assert code == 0 and 'grad_norm' in printed
    rows = [r for r in _rows(on) if r['tag'] == 'summary']
    assert len(rows) == 3
    for r in rows:
        assert all(k in r for k in GUARD_SCALARS), r
        assert r['skipped_steps_d'] == r['skipped_steps_g'] == 0 and r['grad_norm_g'] > 0 and r['grad_norm_d'] > 0
    ev = [f for f in os.listdir(on) if f.startswith('events.out.tfevents.')]
    tags = {v.tag.split('/')[0] for e in OS.read_events(os.path.join(on, ev[0]))[1:] for v in e.summary.value}
    assert set(GUARD_SCALARS) <= tags, tags
    monkeypatch.delenv('SAVP_GUARD')
    off = str(tmp_path / 'off')
    code, printed = _run_train(off, monkeypatch, '', 3, 1)
    assert code == 0 and 'grad_norm' not in printed
    assert not any(k in r for r in _rows(off) for k in GUARD_SCALARS)
    ev = [f for f in os.listdir(off) if f.startswith('events.out.tfevents.')]
    tags = {v.tag.split('/')[0] for e in OS.read_events(os.path.join(off, ev[0]))[1:] for v in e.summary.value}
    assert not (set(GUARD_SCALARS) & tags)

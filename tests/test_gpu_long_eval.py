"""The long_sequence_length model of scripts/train.py on the GPU (pytest -m gpu): a test-mode model that reads the training model's variables
(build_graph(share_with=...), the reference's reuse_variables()), and the runner that writes its accumulated evaluation under the suffix _2
next to the validation losses under _1."""
import contextlib
import functools
import io
import os
import struct
import sys

import numpy as np
import pytest
import torch

from tests import oracle_summaries as OS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = 'cuda:0'
B, T, T_LONG, H, W = 2, 4, 6, 32, 32
HP = dict(context_frames=2, sequence_length=T, nz=4, clip_length=3, batch_size=B)


def _model(mode, **over):
    from video_prediction_amd.models import get_model_class
    return get_model_class('savp')(mode=mode, hparams_dict=dict(HP, **over), eval_num_samples=2)


def _batches():
    g = torch.Generator().manual_seed(21)
    return ({'images': torch.rand(B, T, H, W, 3, generator=g).to(DEV)}, {'images': torch.rand(1, T_LONG, H, W, 3, generator=g).to(DEV)})


def test_long_model_reads_the_training_models_variables():
    train, long_inputs = _batches()
    m = _model('train')
    m.build_graph(train)
    allocated = torch.cuda.memory_allocated()
    long = _model('test', sequence_length=T_LONG)
    long.build_graph(long_inputs, share_with=m)
    own = torch.cuda.memory_allocated() - allocated
    store = m.engine.store
    assert long.engine.store is store
    # no variable tensor of its own: every variable the long model's networks hold is a view into the training model's arenas ...
    for name in long.saveable_variables:
        assert long.engine.net_store[name].data_ptr() == store[name].data_ptr(), name
    # ... and a model of the same shapes that creates its variables allocates that much more
    apart = _model('test', sequence_length=T_LONG)
    allocated = torch.cuda.memory_allocated()
    apart.build_graph(long_inputs)
    assert torch.cuda.memory_allocated() - allocated >= own + 4 * sum(int(np.prod(store[n].shape)) for n in apart.engine.store.names())
    del apart
    before = {k: g.p.clone() for k, g in store.groups.items()}
    m.train_step(train)
    after_step = {k: g.p.clone() for k, g in store.groups.items()}
    assert not torch.equal(before['g'], after_step['g'])
    noise = long.engine.default_noise()
    got = {k: v.clone() for k, v in long.generate(long_inputs, noise).items()}
    torch.cuda.synchronize()
    assert long.global_step == m.global_step == 1                  # the sharing model follows the step of the model that trains
    for k, g in store.groups.items():                              # it never writes the store
        assert torch.equal(g.p.view(torch.int32), after_step[k].view(torch.int32)), k
    fresh = _model('test', sequence_length=T_LONG)
    fresh.build_graph(long_inputs, values=store.to_numpy())
    want = fresh.generate(long_inputs, noise)
    torch.cuda.synchronize()
    assert set(got) == set(want) == {'gen_images', 'gen_images_enc'}
    for k in got:
        assert tuple(got[k].shape) == (1, T_LONG - 1, H, W, 3)
        assert torch.equal(got[k].contiguous().view(torch.int32), want[k].contiguous().view(torch.int32)), k


def test_a_missing_or_mis_shaped_shared_variable_is_named():
    train, long_inputs = _batches()
    m = _model('train')
    m.build_graph(train)
    with pytest.raises(KeyError, match='generator/prior/'):         # the learned prior's network is not in the training model
        _model('test', sequence_length=T_LONG, learn_prior=True).build_graph(long_inputs, share_with=m)
    with pytest.raises(ValueError, match=r"'generator/[^']+' has shape"):
        _model('test', sequence_length=T_LONG, ngf=16).build_graph(long_inputs, share_with=m)
    with pytest.raises(ValueError, match='build_graph'):
        _model('test', sequence_length=T_LONG).build_graph(long_inputs, share_with=_model('train'))


def _run_train(out, dataset_hparams, monkeypatch):
    sys.path.insert(0, ROOT)
    from scripts import train as TR
    from video_prediction_amd import models
    orig = models.get_model_class
    monkeypatch.setattr(models, 'get_model_class', lambda name: functools.partial(orig(name), eval_num_samples=2))
    monkeypatch.setattr(TR.SyntheticVideoDataset, 'num_examples_per_epoch', lambda self: 8)
    TR.main(['--input_dir', 'none', '--dataset', 'synthetic', '--synthetic_shape', '32,32,3', '--model', 'savp', '--output_dir', out,
             '--progress_freq', '0', '--seed', '3', '--dataset_hparams', dataset_hparams,
             '--model_hparams', 'batch_size=2,max_steps=3,nz=4,clip_length=3',
             '--summary_freq', '1', '--image_summary_freq', '0', '--eval_summary_freq', '0', '--accum_eval_summary_freq', '3'])
    torch.cuda.synchronize()


LONG_HPARAMS = 'sequence_length=4,long_sequence_length=6'


@pytest.fixture(scope='module')
def train_runs(tmp_path_factory):
    """scripts/train.py twice, in this process: three steps on the synthetic dataset at 32x32, batch 2, sequence 4, two evaluation samples, eight
    validation examples, frequencies 1 / 0 / 0 / 3; run `long` with an explicit long_sequence_length=6, run `short` without one."""
    root = tmp_path_factory.mktemp('long_eval_train')
    out = {}
    for name, dataset_hparams in (('long', LONG_HPARAMS), ('short', 'sequence_length=4')):
        buf = io.StringIO()
        with pytest.MonkeyPatch.context() as mp, contextlib.redirect_stdout(buf):
            _run_train(str(root / name), dataset_hparams, mp)
        out[name] = (str(root / name), buf.getvalue())
    return out


def _scalars(run_dir):
    ev_files = [f for f in os.listdir(run_dir) if f.startswith('events.out.tfevents.')]
    assert len(ev_files) == 1
    out = {}
    for e in OS.read_events(os.path.join(run_dir, ev_files[0]))[1:]:
        for v in e.summary.value:
            if not v.HasField('image'):
                out[(e.step, v.tag)] = v.simple_value
    return out


LOSS_TAGS = ('g_loss_1/g_loss', 'gen_l1_loss_1/gen_l1_loss', 'd_loss_1/d_loss', 'loss_1/loss')


def test_runner_writes_validation_losses_and_the_long_models_evaluation(train_runs):
    long_dir, printed = train_runs['long']
    short_dir, short_printed = train_runs['short']
    s_long, s_short = _scalars(long_dir), _scalars(short_dir)
    tags_long, tags_short = {t for _, t in s_long}, {t for _, t in s_short}
    for t in LOSS_TAGS + ('accum_eval_psnr_1/accum_eval_psnr/min', 'accum_eval_psnr_2/accum_eval_psnr/min', 'accum_eval_ssim_2/accum_eval_ssim/avg',
                          'accum_eval_mse_2/accum_eval_mse/max'):
        assert t in tags_long, (t, sorted(tags_long))
    for t in LOSS_TAGS + ('accum_eval_psnr_1/accum_eval_psnr/min',):
        assert t in tags_short, (t, sorted(tags_short))
    assert not [t for t in tags_short if t.split('/')[0].endswith('_2')]
    assert {t for t in tags_long if not t.split('/')[0].endswith('_2')} == tags_short
    # the validation losses are written at every summary step, the training losses next to them
    assert {s for s, t in s_long if t == 'g_loss_1/g_loss'} == {s for s, t in s_long if t == 'g_loss/g_loss'} != set()
    # eight examples: four updates of the main model at batch 2, eight of the long model at batch max(1, 2 // 2) = 1
    assert 'evaluating 4 / 4' in printed and 'evaluating 8 / 8' in printed and 'evaluating 8 / 8' not in short_printed
    # what the main model writes does not depend on the long model being there
    for key, v in s_short.items():
        if 'ssim' in key[1]:                         # fp32 atomics in arrival order: tests/test_gpu_evaluate.py bounds the effect by rtol 4e-7
            assert abs(s_long[key] - v) <= 4e-7 * abs(v), key
        else:
            assert struct.pack('<f', s_long[key]) == struct.pack('<f', v), key


def test_long_model_changes_neither_the_checkpoint_nor_the_jsonl(train_runs):
    from video_prediction_amd import checkpoint as CK
    long_dir, short_dir = train_runs['long'][0], train_runs['short'][0]
    va, vb = CK.read_checkpoint(os.path.join(long_dir, 'model-3')), CK.read_checkpoint(os.path.join(short_dir, 'model-3'))
    assert set(va) == set(vb) and any('Adam' in k for k in va)
    diff = [k for k in va if np.asarray(va[k]).tobytes() != np.asarray(vb[k]).tobytes()]
    assert not diff, (len(diff), diff[:3])
    rows = open(os.path.join(long_dir, 'summaries.jsonl'), 'rb').read()
    assert rows == open(os.path.join(short_dir, 'summaries.jsonl'), 'rb').read() and len(rows.splitlines()) == 3
    assert b'_1' not in rows and b'_2' not in rows                  # the rows stay as they are: training scalars only


def test_the_long_models_tags_equal_a_direct_accumulated_evaluation(train_runs):
    """The _2 values against accum_eval_* computed here with a model of its own, built from the run's final checkpoint (the accumulated
    evaluation ran behind the last step), on the same batches -- the head of the long validation set at batch 1 -- at the same step."""
    sys.path.insert(0, ROOT)
    from scripts import train as TR
    from video_prediction_amd import checkpoint as CK
    long_dir = train_runs['long'][0]
    scalars = {t: v for (s, t), v in _scalars(long_dir).items() if s == 2 and t.split('/')[0].endswith('_2')}
    ds = TR.SyntheticVideoDataset('none', mode='val', seed=3, hparams=LONG_HPARAMS, shape=(H, W, 3))
    ds.set_sequence_length(TR.long_eval_length(ds, True))
    it = iter(ds.make_batch(TR.long_eval_batch(B), device=DEV))
    batches = [next(it) for _ in range(8)]
    assert tuple(batches[0]['images'].shape) == (1, T_LONG, H, W, 3)
    m = _model('test', sequence_length=T_LONG)
    m.build_graph(batches[0], values=CK.read_checkpoint(os.path.join(long_dir, 'model-3')))
    m.engine.step = 3
    m.accum_eval_reset()
    for b in batches:
        m.accum_eval_update(b)
    want = {k: float(v) for k, v in m.accum_eval_summary_fn().items()}
    assert len(want) == 9 and set(scalars) == {k.split('/')[0] + '_2/' + k for k in want}
    for k, v in want.items():
        got = scalars[k.split('/')[0] + '_2/' + k]
        if 'ssim' in k:
            assert abs(got - v) <= 4e-7 * abs(v), (k, got, v)
        else:
            assert struct.pack('<f', got) == struct.pack('<f', v), (k, got, v)

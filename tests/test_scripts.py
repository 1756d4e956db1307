"""Host logic of scripts/train.py / scripts/generate.py against the reference's command line (flags, defaults, directory naming,
step-frequency rules, side files) -- CPU only; the GPU smoke of the runners is tests/test_gpu_model.py::test_train_and_generate_scripts."""
import json
import os
import struct
import zlib

import numpy as np
import pytest

from scripts import generate as G
from scripts import train as T

# the flags the reference's scripts/train.py and scripts/generate.py declare (tests/golden/make_reference_fixtures.py)
REF_FLAGS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'reference_script_flags.json')


def _ref_flags(name):
    with open(REF_FLAGS) as fh:
        return set(json.load(fh)[name])


def test_flags_match_the_reference_scripts():
    ours = {a.option_strings[0] for a in T.build_parser()._actions if a.option_strings and a.option_strings[0] != '-h'}
    assert _ref_flags('train.py') <= ours, _ref_flags('train.py') - ours
    assert ours - _ref_flags('train.py') == {'--synthetic_shape'}
    ours = {a.option_strings[0] for a in G.build_parser()._actions if a.option_strings and a.option_strings[0] != '-h'}
    assert _ref_flags('generate.py') <= ours
    assert ours - _ref_flags('generate.py') == {'--synthetic_shape'}


def test_flag_defaults():
    a = T.build_parser().parse_args(['--input_dir', 'x'])
    assert (a.logs_dir, a.summary_freq, a.image_summary_freq, a.eval_summary_freq, a.accum_eval_summary_freq, a.progress_freq,
            a.save_freq, a.aggregate_nccl, a.gpu_mem_frac, a.seed) == ('logs', 1000, 5000, 25000, 100000, 100, 5000, 0, 0, None)
    g = G.build_parser().parse_args(['--input_dir', 'x'])
    assert (g.results_dir, g.mode, g.batch_size, g.num_epochs, g.num_stochastic_samples, g.fps, g.seed) == ('results', 'val', 8, 1, 5, 4, 7)


def test_output_dir_naming_like_train_py_68_83():
    assert T.model_fname_from('savp', 'lr=0.001,schedule_sampling_steps=[0,100]') == 'model.savp.lr.0.001.schedule_sampling_steps.0..100'
    assert T.model_fname_from('savp', None) == 'model.savp.None'
    a = T.build_parser().parse_args(['--input_dir', 'x', '--model', 'savp', '--model_hparams', 'nz=8', '--output_dir_postfix', '_run1'])
    T.resolve_options(a)
    assert a.output_dir == os.path.join('logs', 'model.savp.nz.8') + '_run1'


def test_resume_reads_options_and_hparams_back(tmp_path):
    d = tmp_path / 'run'
    d.mkdir()
    (d / 'options.json').write_text(json.dumps({'dataset': 'bair', 'model': 'savp'}))
    (d / 'model_hparams.json').write_text(json.dumps({'nz': 8, 'lr': 0.0002}))
    (d / 'dataset_hparams.json').write_text(json.dumps({'sequence_length': 12}))
    a = T.build_parser().parse_args(['--input_dir', 'x', '--output_dir', str(d), '--resume'])
    ds, mh = T.resolve_options(a)
    assert (a.checkpoint, a.dataset, a.model) == (str(d), 'bair', 'savp') and mh == {'nz': 8, 'lr': 0.0002} and ds == {'sequence_length': 12}
    with pytest.raises(ValueError):
        T.resolve_options(T.build_parser().parse_args(['--input_dir', 'x', '--output_dir', str(d), '--resume', '--checkpoint', str(d)]))
    # a checkpoint PREFIX names its directory (train.py:98-101); generate.py derives the result directories from it (:77-79)
    g = G.build_parser().parse_args(['--input_dir', 'x', '--checkpoint', str(d / 'model-100')])
    ds, mh = G.resolve_options(g)
    assert (g.dataset, g.model, mh['nz']) == ('bair', 'savp', 8)
    assert g.output_png_dir == os.path.join('results', 'run') and g.output_gif_dir == os.path.join('results', 'run')
    with pytest.raises(ValueError):
        G.resolve_options(G.build_parser().parse_args(['--input_dir', 'x']))


def test_should_rule_like_train_py_232_236():
    max_steps, start = 1000, 0
    assert T.should(-1, 100, max_steps, start)                      # step -1: log everything before training
    assert T.should(99, 100, max_steps, start) and not T.should(100, 100, max_steps, start)
    assert T.should(999, 7, max_steps, start)                       # the last step always
    assert not T.should(5, 0, max_steps, start)                     # 0 disables
    assert T.should(999, None, max_steps, start) and not T.should(99, None, max_steps, start)


def test_checkpoint_pruning_keeps_two(tmp_path):
    for step in (5, 10, 15):
        for ext in ('.index', '.data-00000-of-00001'):
            (tmp_path / ('model-%d%s' % (step, ext))).write_bytes(b'x')
    T.prune_checkpoints(str(tmp_path), keep=2)
    left = sorted(os.listdir(str(tmp_path)))
    assert left == ['model-10.data-00000-of-00001', 'model-10.index', 'model-15.data-00000-of-00001', 'model-15.index']


def test_png_writer_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    for c in (1, 3):
        img = rng.integers(0, 256, (5, 7, c), dtype=np.uint8)
        p = str(tmp_path / ('a%d.png' % c))
        G.write_png(p, img)
        raw = open(p, 'rb').read()
        assert raw[:8] == b'\x89PNG\r\n\x1a\n'
        pos, chunks = 8, {}
        while pos < len(raw):
            n, tag = struct.unpack('>I4s', raw[pos:pos + 8])
            data = raw[pos + 8:pos + 8 + n]
            assert struct.unpack('>I', raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xffffffff
            chunks[tag] = data
            pos += 12 + n
        w, h, depth, ctype = struct.unpack('>IIBB', chunks[b'IHDR'][:10])
        assert (w, h, depth, ctype) == (7, 5, 8, 0 if c == 1 else 2)
        rows = zlib.decompress(chunks[b'IDAT'])
        got = np.frombuffer(rows, dtype=np.uint8).reshape(5, 1 + 7 * c)[:, 1:].reshape(5, 7, c)
        assert np.array_equal(got, img)


def test_generate_main_loop_file_names_and_side_files(tmp_path, monkeypatch):
    """scripts/generate.py main() with a stand-in dataset / model on CPU: two batches x two draws, only the future frames written, names
    gen_image_<sample>_<draw>_<t>.png (generate.py:154-189), the three side JSONs in both output directories (:140-148)."""
    import types
    import torch
    from scripts import train as T_
    from video_prediction_amd import models as M

    class HP(object):
        def __init__(self, **kw):
            self.__dict__.update(kw)

        def values(self):
            return dict(self.__dict__)

    class FakeDataset(object):
        def __init__(self, input_dir, mode, num_epochs, seed, hparams_dict, hparams):
            self.hparams = HP(context_frames=2, sequence_length=5, time_shift=0)

        def num_examples_per_epoch(self):
            return 4

        def make_batch(self, batch_size, device=None):
            for k in range(2):
                yield {'images': torch.full((batch_size, 5, 4, 6, 3), 0.1 * (k + 1))}

    calls = []

    class FakeModel(object):
        def __init__(self, mode, hparams_dict, hparams):
            assert mode == 'test' and hparams_dict['sequence_length'] == 5 and hparams_dict['context_frames'] == 2
            self.hparams = HP(**hparams_dict)

        def build_graph(self, inputs, device=None):
            calls.append('build')

        def generate(self, inputs):
            calls.append('generate')
            x = inputs['images']
            ramp = torch.arange(4, dtype=torch.float32).view(1, 4, 1, 1, 1) / 255.0
            return {'gen_images': x[:, 1:] * 0 + ramp}                      # frame t of the unroll = t / 255

    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(T_, 'get_dataset_class', lambda name, shape: FakeDataset)
    monkeypatch.setattr(M, 'get_model_class', lambda name: FakeModel)
    out = tmp_path / 'res'
    G.main(['--input_dir', 'none', '--dataset', 'synthetic', '--model', 'savp', '--batch_size', '2', '--num_stochastic_samples', '2',
            '--results_dir', str(out)])
    d = out / 'model.savp'
    names = sorted(p for p in os.listdir(str(d)) if p.endswith('.png'))
    assert len(names) == 4 * 2 * 3                                            # samples x draws x future frames (5 - 2)
    assert names[0] == 'gen_image_00000_00_00.png' and names[-1] == 'gen_image_00003_01_02.png'
    assert calls == ['build'] + ['generate'] * 4
    for fname in ('options.json', 'dataset_hparams.json', 'model_hparams.json'):
        assert json.load(open(str(d / fname)))
    assert json.load(open(str(d / 'options.json')))['num_stochastic_samples'] == 2
    # the LAST three frames of the unroll are the future ones: pixel value = 1 + t
    raw = open(str(d / 'gen_image_00002_01_01.png'), 'rb').read()
    pos = raw.index(b'IDAT')
    n = struct.unpack('>I', raw[pos - 4:pos])[0]
    rows = np.frombuffer(zlib.decompress(raw[pos + 4:pos + 4 + n]), dtype=np.uint8).reshape(4, 1 + 6 * 3)
    assert set(rows[:, 1:].ravel().tolist()) == {2}
    with pytest.raises(ValueError):
        G.main(['--input_dir', 'none', '--dataset', 'synthetic', '--model', 'savp', '--batch_size', '3', '--results_dir', str(out)])

"""scripts/evaluate.py on the host: the reference's command line (tests/golden/reference_evaluate_flags.json, read out of the reference's
evaluate.py by tests/golden/make_evaluate_flags.py), output-directory naming and the prediction_eval_* tree that the reference's
combine_results.py / plot_results.py read (CSV bytes, appends, PNG names and pixels).  No GPU."""
import argparse
import csv
import json
import os
import struct
import types
import zlib

import numpy as np
import pytest

from scripts import evaluate as E

HERE = os.path.dirname(os.path.abspath(__file__))


def _reference_flags():
    with open(os.path.join(HERE, 'golden', 'reference_evaluate_flags.json')) as f:
        return json.load(f)['evaluate.py']


def _reference_load_metrics(prefix_fname):
    """Restatement of the reference's load_metrics (evaluate.py:61-67 / combine_results.py:17-24)."""
    with open('%s.csv' % prefix_fname, newline='') as csvfile:
        reader = csv.reader(csvfile, delimiter='\t', quotechar='|')
        rows = list(reader)
        metrics = np.array(rows)[1:, 1:-1].astype(np.float32)
    return metrics


def _read_png(path):
    """8-bit RGB / grayscale PNG with filter type 0 on every scanline (what scripts.generate.write_png writes) -> uint8 [H, W, C]."""
    data = open(path, 'rb').read()
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, hdr = 8, b'', None
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    w, h, depth, ctype = hdr[0], hdr[1], hdr[2], hdr[3]
    assert depth == 8
    c = 3 if ctype == 2 else 1
    raw = zlib.decompress(idat)
    rows = []
    for y in range(h):
        line = raw[y * (w * c + 1):(y + 1) * (w * c + 1)]
        assert line[0] == 0
        rows.append(np.frombuffer(line[1:], dtype=np.uint8).reshape(w, c))
    return np.stack(rows)


def test_flags_names_order_and_defaults_match_the_reference():
    ref = _reference_flags()
    actions = [a for a in E.build_parser()._actions if a.option_strings and a.dest != 'help']
    ours = [a.option_strings[0] for a in actions]
    assert ours[:len(ref)] == [e['flag'] for e in ref]
    assert ours[len(ref):] == ['--synthetic_shape']                # this repository's only addition, last
    for a, e in zip(actions, ref):
        if e.get('action') == 'store_true':
            assert isinstance(a, argparse._StoreTrueAction) and a.default is False, e['flag']
            continue
        assert a.default == e.get('default'), e['flag']
        assert (a.type.__name__ if a.type else None) == e.get('type'), e['flag']
        assert a.nargs == e.get('nargs'), e['flag']
        assert (list(a.choices) if a.choices else None) == e.get('choices'), e['flag']
        assert bool(a.required) == bool(e.get('required')), e['flag']
    assert E.build_parser().parse_args(['--input_dir', 'x']).eval_substasks == ['max', 'avg', 'min']
    help_text = E.build_parser().format_help()
    for flag in ('--gpu_mem_frac', '--gt_inputs_dir', '--gt_outputs_dir'):
        block = help_text[help_text.rindex(flag):]
        assert 'no effect' in ' '.join(block[:400].split()), flag


def test_output_dir_naming(tmp_path):
    ckpt = tmp_path / 'logs' / 'bair' / 'ours_savp'
    ckpt.mkdir(parents=True)
    (ckpt / 'options.json').write_text(json.dumps({'dataset': 'bair', 'model': 'savp'}))
    (ckpt / 'model_hparams.json').write_text(json.dumps({'nz': 8}))
    p = E.build_parser()
    for checkpoint in (str(ckpt), str(ckpt / 'model-200000')):      # a directory, or a checkpoint prefix inside it
        args = p.parse_args(['--input_dir', 'x', '--checkpoint', checkpoint, '--results_dir', 'res'])
        ds, mh, leaf = E.read_checkpoint_options(args)
        assert (args.dataset, args.model, ds, mh) == ('bair', 'savp', {}, {'nz': 8})
        assert E.output_dir_of(args, leaf) == os.path.join('res', 'ours_savp')
    args = p.parse_args(['--input_dir', 'x', '--dataset', 'kth', '--model', 'savp'])
    assert E.output_dir_of(args, E.read_checkpoint_options(args)[2]) == os.path.join('results', 'model.savp')
    args = p.parse_args(['--input_dir', 'x', '--dataset', 'kth', '--model', 'savp', '--output_dir', 'here'])
    assert E.output_dir_of(args, E.read_checkpoint_options(args)[2]) == 'here'
    with pytest.raises(ValueError):
        E.read_checkpoint_options(p.parse_args(['--input_dir', 'x', '--model', 'savp']))


def test_csv_bytes_append_and_reference_load_metrics(tmp_path):
    prefix = str(tmp_path / 'metrics' / 'psnr')
    first = np.array([[1.5, 2.25, 3.0], [0.1, 0.2, 0.3]], dtype=np.float32)
    second = np.array([[4.0, 5.0, 6.5]], dtype=np.float32)
    E.save_metrics(prefix, first, sample_start_ind=0)
    E.save_metrics(prefix, second, sample_start_ind=2)
    want = ('sample_ind\t0\t1\t2\tmean\r\n'
            '0\t1.5\t2.25\t3.0\t%s\r\n' % str(np.mean(first[0])) +
            '1\t0.1\t0.2\t0.3\t%s\r\n' % str(np.mean(first[1])) +
            '2\t4.0\t5.0\t6.5\t%s\r\n' % str(np.mean(second[0])))
    assert open(prefix + '.csv', 'rb').read().decode() == want
    back = _reference_load_metrics(prefix)
    assert back.dtype == np.float32 and np.array_equal(back, np.concatenate([first, second]))
    assert np.array_equal(E.load_metrics(prefix), back)
    E.save_metrics(prefix, second, sample_start_ind=0)               # a first batch truncates
    assert np.array_equal(_reference_load_metrics(prefix), second)


def test_png_names_truncation_and_grayscale_tiling(tmp_path):
    rgb = np.full((2, 4, 5, 3), 0.999, dtype=np.float32)
    rgb[0, 0, 0] = (0.0, 0.5, 1.0)
    E.save_image_sequences(str(tmp_path / 'inputs' / 'context_image'), rgb[None], sample_start_ind=7)
    names = sorted(os.listdir(tmp_path / 'inputs'))
    assert names == ['context_image_00007_00.png', 'context_image_00007_01.png']
    img = _read_png(str(tmp_path / 'inputs' / names[0]))
    assert img.shape == (4, 5, 3)
    assert tuple(img[0, 0]) == (0, 127, 255)                        # 0.5 * 255 = 127.5 -> 127: truncation, not rounding
    assert int(img[1, 1, 0]) == int(np.float32(0.999) * np.float32(255.0)) == 254
    gray = np.linspace(0, 1, 4 * 5, dtype=np.float32).reshape(1, 4, 5, 1)
    E.save_image_sequence(str(tmp_path / 'g'), gray, time_start_ind=3)
    img = _read_png(str(tmp_path / 'g_03.png'))
    assert img.shape == (4, 5, 3)
    want = (gray[0] * 255.0).astype(np.uint8)[..., 0]
    for c in range(3):
        assert np.array_equal(img[..., c], want)


def _hand_results(B, T, F, H=12, W=12, C=3, seed=0):
    rng = np.random.default_rng(seed)
    res = {'images': rng.random((B, T, H, W, C), dtype=np.float32)}
    for m in ('psnr', 'mse', 'ssim'):
        for sub in ('min', 'avg', 'max'):
            res['eval_%s/%s' % (m, sub)] = rng.random((B, F), dtype=np.float32)
            res['eval_gen_images_%s/%s' % (m, sub)] = rng.random((B, T - 1, H, W, C), dtype=np.float32)
    return res


def test_prediction_eval_tree_from_a_hand_made_results_dict(tmp_path):
    hp = types.SimpleNamespace(sequence_length=6, context_frames=2)
    F = hp.sequence_length - hp.context_frames
    task = str(tmp_path / 'prediction_eval')
    r0, r1 = _hand_results(2, 6, F, seed=1), _hand_results(2, 6, F, seed=2)
    E.save_prediction_eval_results(task, r0, hp, 0, False, ['max', 'avg', 'min'])
    E.save_prediction_eval_results(task, r1, hp, 2, False, ['max', 'avg', 'min'])
    dirs = sorted(os.listdir(tmp_path))
    assert dirs == sorted('prediction_eval_%s_%s' % (m, s) for m in ('psnr', 'mse', 'ssim') for s in ('max', 'avg', 'min'))
    for m in ('psnr', 'mse', 'ssim'):
        for s in ('max', 'avg', 'min'):
            d = tmp_path / ('prediction_eval_%s_%s' % (m, s))
            assert sorted(os.listdir(d)) == ['inputs', 'metrics', 'outputs']
            assert os.listdir(d / 'metrics') == [m + '.csv']
            met = _reference_load_metrics(str(d / 'metrics' / m))
            assert met.shape == (4, F)
            assert np.array_equal(met, np.concatenate([r0['eval_%s/%s' % (m, s)], r1['eval_%s/%s' % (m, s)]]))
            ins = sorted(os.listdir(d / 'inputs'))
            outs = sorted(os.listdir(d / 'outputs'))
            assert ins == ['context_image_%05d_%02d.png' % (i, t) for i in range(4) for t in range(hp.context_frames)]
            assert outs == ['gen_image_%05d_%02d.png' % (i, t) for i in range(4) for t in range(F)]
            gen = r1['eval_gen_images_%s/%s' % (m, s)]
            got = _read_png(str(d / 'outputs' / 'gen_image_00003_01.png'))
            assert np.array_equal(got, (gen[1, -F + 1] * 255.0).astype(np.uint8))      # future frame 1 of the batch's 2nd sequence
            got = _read_png(str(d / 'inputs' / 'context_image_00002_01.png'))
            assert np.array_equal(got, (r1['images'][0, 1] * 255.0).astype(np.uint8))


def test_only_metrics_skips_images_and_a_deterministic_model_shares_its_frames(tmp_path):
    hp = types.SimpleNamespace(sequence_length=5, context_frames=2)
    rng = np.random.default_rng(3)
    res = {'images': rng.random((1, 5, 12, 12, 1), dtype=np.float32),
           'eval_gen_images': rng.random((1, 4, 12, 12, 1), dtype=np.float32)}
    for sub in ('min', 'avg', 'max'):
        res['eval_psnr/%s' % sub] = rng.random((1, 3), dtype=np.float32)
    E.save_prediction_eval_results(str(tmp_path / 'a' / 'prediction_eval'), res, hp, 0, True, ['max'])
    assert sorted(os.listdir(tmp_path / 'a')) == ['prediction_eval_psnr_max']
    assert os.listdir(tmp_path / 'a' / 'prediction_eval_psnr_max') == ['metrics']
    E.save_prediction_eval_results(str(tmp_path / 'b' / 'prediction_eval'), res, hp, 0, False, ['avg'])
    img = _read_png(str(tmp_path / 'b' / 'prediction_eval_psnr_avg' / 'outputs' / 'gen_image_00000_02.png'))
    assert img.shape == (12, 12, 3)
    assert np.array_equal(img[..., 2], (res['eval_gen_images'][0, 3, ..., 0] * 255.0).astype(np.uint8))


def test_closing_table_prints_the_max_tables_that_exist(tmp_path, capsys):
    E.save_metrics(str(tmp_path / 'prediction_eval_psnr_max' / 'metrics' / 'psnr'), np.array([[20.0, 22.0], [24.0, 26.0]], np.float32))
    E.save_metrics(str(tmp_path / 'prediction_eval_ssim_avg' / 'metrics' / 'ssim'), np.array([[0.5, 0.6]], np.float32))
    E.print_metric_tables(str(tmp_path))
    out = capsys.readouterr().out
    assert 'prediction_eval_psnr_max psnr' in out and 'ssim' not in out and 'lpips' not in out
    assert '{:>10} {:>10.4f} ({:>7.4f})'.format('mean (std)', 23.0, np.std([20.0, 22.0, 24.0, 26.0])) in out
    assert '{:>10} {:>10.4f} ({:>7.4f})'.format(1, 24.0, 2.0) in out

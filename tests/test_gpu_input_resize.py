"""Dataset hyper-parameters crop_size / scale_size on the device (pytest -m gpu): savp_u8_frames_resize_f32 (csrc/input_resize.hip) against the
float64 restatement tests/oracle_resize.py, its exact cases, the three datasets end to end on records written here, and scripts/train.py +
scripts/generate.py on 32-pixel records enlarged to 64.

Error bound of the parity cases, derived, not tuned: outputs lie in [0, 1] and an output pixel is a weighted fp32 sum of n source values
(n = 4 for bilinear, (ceil(crop / S) + 1)^2 for area, 1 for a copy), so |got - want| <= (n + 4) * 2^-23 absolute -- about twice the worst
case of one rounding per term plus the weight and the final scaling.  (The kernel sums in integers and rounds only in the final division
and scaling, which is well inside it.)  Every element is compared."""
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import oracle_resize as OR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = 'cuda:0'

# name: (Hs, Ws, C, crop_size, scale_size, B, T)
CASES = {
    'bilinear 64->128 dyadic': (64, 64, 3, 0, 128, 2, 3),
    'bilinear 32->64 dyadic, 1 channel': (32, 32, 1, 0, 64, 3, 5),
    'bilinear 48x64 -> crop 48 -> 64 non-dyadic': (48, 64, 3, 0, 64, 3, 5),
    'bilinear 5->7 odd, scalar stores': (5, 5, 1, 0, 7, 3, 5),
    'area 128->64 integer': (128, 128, 3, 0, 64, 2, 3),
    'area 64->48 fractional': (64, 64, 3, 0, 48, 3, 5),
    'area 7->3 odd, 1 channel': (7, 7, 1, 0, 3, 3, 5),
    'area 9x7 -> crop 7 -> 3 odd, 3 channels': (9, 7, 3, 0, 3, 1, 7),
    'area 64->47 fractional, 1 channel': (64, 64, 1, 0, 47, 1, 3),
    'crop only 64->48': (64, 64, 3, 48, 0, 3, 5),
    'crop only 65->64 (odd pixel dropped at the far end)': (65, 65, 1, 64, 0, 3, 5),
    'pad only 47x64 -> 64': (47, 64, 3, 64, 0, 3, 5),
    'pad then bilinear 47x64 -> 64 -> 96': (47, 64, 3, 64, 96, 1, 3),
    'pad then area 47x50 -> 64 -> 40, 1 channel': (47, 50, 1, 64, 40, 3, 5),
    'crop one axis, pad the other, 10x6 -> 8 -> 12, 2 channels': (10, 6, 2, 8, 12, 3, 5),
}


def bound(crop, S):
    return (OR.taps(crop, S) + 4) * 2.0 ** -23


def _frames(name, shape):
    rng = np.random.default_rng(sum(name.encode()))
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _resize(frames, crop, S):
    """frames uint8 [B, T, Hs, Ws, C] (numpy) -> the kernel's [T, B, S, S, C] as numpy."""
    from video_prediction_amd import kernels as K
    B, T, _, _, C = frames.shape
    out = torch.empty(T, B, S, S, C, device=DEV)
    K.u8_frames_resize_f32(torch.from_numpy(frames).to(DEV), out, crop)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('name', sorted(CASES))
def test_kernel_matches_the_float64_restatement(name):
    Hs, Ws, C, crop_size, scale_size, B, T = CASES[name]
    frames = _frames(name, (B, T, Hs, Ws, C))
    crop, S = OR.resolve((Hs, Ws, C), crop_size, scale_size)
    got = _resize(frames, crop, S)
    want = OR.preprocess(frames, crop_size, scale_size).transpose(1, 0, 2, 3, 4)
    assert got.shape == want.shape == (T, B, S, S, C) and got.dtype == np.float32
    err = float(np.abs(got.astype(np.float64) - want).max())                      # NaN (an element nobody wrote) fails the comparison
    print('%s: max abs err %.3e, bound %.3e' % (name, err, bound(crop, S)))
    assert err <= bound(crop, S), (name, err, bound(crop, S))


@pytest.mark.parametrize('name', ['crop only 64->48', 'crop only 65->64 (odd pixel dropped at the far end)', 'pad only 47x64 -> 64'])
def test_crop_only_and_pad_only_are_bit_exact(name):
    """The contract of test_input_pipeline_to_device (tests/test_gpu_ops.py): uint8 * float32(1/255) of the window; padding is exactly 0.0."""
    Hs, Ws, C, crop, _, B, T = CASES[name]
    frames = _frames(name, (B, T, Hs, Ws, C))
    frames[frames == 0] = 1                                                        # zeros then mark the padding alone
    got = _resize(frames, crop, crop)
    window = OR.crop_or_pad(frames, crop)
    want = (window.astype(np.float32) * np.float32(1.0 / 255.0)).transpose(1, 0, 2, 3, 4)
    assert np.array_equal(got, want)
    pad = (window == 0).transpose(1, 0, 2, 3, 4)
    (sy, py), (sx, px) = OR.crop_or_pad_offsets(Hs, crop), OR.crop_or_pad_offsets(Ws, crop)
    assert pad.sum() == T * B * C * (crop * crop - min(Hs, crop) * min(Ws, crop))
    assert (got[pad] == 0.0).all() and not np.signbit(got[pad]).any()
    if py:
        assert not got[:, :, :py].any() and not got[:, :, py + Hs:].any() and got[:, :, py:py + Hs].all()


@pytest.mark.parametrize('side,C', [(32, 3), (24, 1)])
def test_bilinear_2x_reproduces_the_source_pixels_at_even_indices(side, C):
    frames = _frames('even %d' % side, (2, 3, side, side, C))
    got = _resize(frames, side, 2 * side)
    want = (frames.astype(np.float32) * np.float32(1.0 / 255.0)).transpose(1, 0, 2, 3, 4)
    assert np.array_equal(got[:, :, ::2, ::2], want)
    # and the last odd row / column repeats the last source row / column (bottom index clamped)
    assert np.array_equal(got[:, :, -1, ::2], want[:, :, -1]) and np.array_equal(got[:, :, ::2, -1], want[:, :, :, -1])


def test_invalid_arguments_are_refused():
    from video_prediction_amd import kernels as K, lib
    L = lib.get()
    u8 = torch.zeros(2, 3, 8, 8, 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros(3, 2, 16, 16, 3, device=DEV)
    ok = [None, u8.data_ptr(), out.data_ptr(), 2, 3, 8, 8, 3, 8, 16]
    assert L.savp_u8_frames_resize_f32(*ok) == 0
    for i, bad in ((1, None), (2, None), (2, out.data_ptr() + 2), (3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (8, 4097), (9, 4097),
                   (3, 70000), (4, 70000)):
        args = list(ok)
        args[i] = bad
        assert L.savp_u8_frames_resize_f32(*args) != 0, (i, bad)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        K.u8_frames_resize_f32(u8, torch.zeros(3, 2, 16, 12, 3, device=DEV), 8)     # not square
    with pytest.raises(ValueError):
        K.u8_frames_resize_f32(u8, torch.zeros(2, 3, 16, 16, 3, device=DEV), 8)     # batch-major output
    with pytest.raises(RuntimeError):
        K.u8_frames_resize_f32(u8.float(), out, 8)


# ---- the datasets end to end -----------------------------------------------------------------------------------------------------
def _check_batches(it, frames, crop_size, scale_size, B, floats=None):
    """Every batch of the unshuffled iterator against the oracle on the frames written; StopIteration after the last full batch."""
    n, T, Hs, Ws, C = frames.shape
    crop, S = OR.resolve((Hs, Ws, C), crop_size, scale_size)
    for k in range(n // B):
        batch = next(it)
        got = batch['images']
        assert tuple(got.shape) == (B, T, S, S, C) and got.dtype == torch.float32
        want = OR.preprocess(frames[k * B:(k + 1) * B], crop_size, scale_size)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        assert err <= bound(crop, S), (k, err, bound(crop, S))
        if floats is not None:
            states, actions = floats
            assert np.array_equal(batch['states'].cpu().numpy(), states[k * B:(k + 1) * B])
            assert np.array_equal(batch['actions'].cpu().numpy(), actions[k * B:(k + 1) * B])
        else:
            assert set(batch) == {'images'}
    with pytest.raises(StopIteration):
        next(it)


def test_bair_records_of_64_pixels_enlarged_to_128(tmp_path):
    from tests.test_oracle_resize import _write_bair
    from video_prediction_amd.datasets import get_dataset_class
    frames = _frames('bair', (5, 12, 64, 64, 3))
    _write_bair(tmp_path / 'test', frames)
    ds = get_dataset_class('bair')(str(tmp_path), mode='test', num_epochs=1, hparams='sequence_length=12,scale_size=128')
    assert ds.image_shape == (64, 64, 3) and ds.output_image_shape == (128, 128, 3)
    _check_batches(ds.make_batch(2), frames, 0, 128, 2)                                  # 5 examples, batch 2, drop_remainder


def test_kth_records_with_crop_size(tmp_path):
    from tests.test_oracle_resize import _write_kth
    from video_prediction_amd.datasets import get_dataset_class
    frames = _frames('kth', (4, 10, 60, 80, 1))                                          # non-square, one channel
    _write_kth(tmp_path / 'test', frames)
    DS = get_dataset_class('kth')
    ds = DS(str(tmp_path), mode='test', num_epochs=1, hparams='sequence_length=10,crop_size=48')
    assert ds.output_image_shape == (48, 48, 1)
    it = ds.make_batch(2)
    first = next(it)['images'].cpu().numpy()
    assert np.array_equal(first, frames[:2, :, 6:54, 16:64].astype(np.float32) * np.float32(1.0 / 255.0))       # crop only: bit-exact
    ds = DS(str(tmp_path), mode='test', num_epochs=1, hparams='sequence_length=10,crop_size=48,scale_size=32')
    _check_batches(ds.make_batch(2), frames, 48, 32, 2)
    ds = DS(str(tmp_path), mode='test', num_epochs=1, hparams='sequence_length=10,scale_size=64')     # crop = the shorter side (60)
    _check_batches(ds.make_batch(3), frames, 0, 64, 3)


def test_cartgripper_records_enlarged_to_64_with_states_and_actions(tmp_path):
    from tests.test_oracle_resize import _write_cartgripper
    from video_prediction_amd.datasets import get_dataset_class
    rng = np.random.default_rng(9)
    frames = _frames('cartgripper', (4, 15, 48, 64, 3))
    states = rng.standard_normal((4, 15, 6)).astype(np.float32)
    actions = rng.standard_normal((4, 14, 3)).astype(np.float32)
    _write_cartgripper(tmp_path / 'test', frames, states, actions)
    DS = get_dataset_class('cartgripper')
    ds = DS(str(tmp_path), mode='test', num_epochs=1, hparams='scale_size=64')
    assert ds.crop_and_scale == (48, 64) and ds.output_image_shape == (64, 64, 3)
    _check_batches(ds.make_batch(2), frames, 0, 64, 2, floats=(states, actions))
    ds = DS(str(tmp_path), mode='test', num_epochs=1)                                     # as recorded: 48 x 64, the plain conversion kernel
    batch = next(ds.make_batch(2))
    assert np.array_equal(batch['images'].cpu().numpy(), frames[:2].astype(np.float32) * np.float32(1.0 / 255.0))


# ---- the scripts -----------------------------------------------------------------------------------------------------------------
def _png_size(path):
    with open(path, 'rb') as f:
        head = f.read(24)
    assert head[:8] == b'\x89PNG\r\n\x1a\n' and head[12:16] == b'IHDR'
    return struct.unpack('>II', head[16:24])


def test_train_and_generate_scripts_on_enlarged_records(tmp_path):
    """Two train steps of a small SAVP (B = 2, sequence_length = 6) on 32-pixel records with --dataset_hparams scale_size=64, then
    scripts/generate.py on the checkpoint it saved: the model is sized from what the iterator delivers (64 x 64).  Each child process runs
    under a limit of its own.  Rehearsed on an MI355X at exactly this size: 2.4 s for each command on a warm machine; the first import of
    torch on a fresh machine can add a minute or more, hence 180 s."""
    import json
    from tests.test_oracle_resize import _write_bair
    data = tmp_path / 'data'
    for mode in ('train', 'val'):
        _write_bair(data / mode, _frames('script ' + mode, (4, 8, 32, 32, 3)))
    out, res = str(tmp_path / 'run'), str(tmp_path / 'results')
    hp = 'sequence_length=6,scale_size=64'
    cmd = ['timeout', '-k', '10', '180', sys.executable, os.path.join(ROOT, 'scripts', 'train.py'), '--input_dir', str(data), '--dataset', 'bair',
           '--model', 'savp', '--output_dir', out, '--progress_freq', '1', '--summary_freq', '1', '--eval_summary_freq', '0', '--save_freq', '2',
           '--dataset_hparams', hp, '--model_hparams', 'batch_size=2,max_steps=2,nz=8']
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print('scripts/train.py: %.1f s' % (time.time() - t0))
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'progress  global step 2' in r.stdout and os.path.exists(os.path.join(out, 'model-2.index'))
    rows = [json.loads(l) for l in open(os.path.join(out, 'summaries.jsonl'))]
    rows = [row for row in rows if row.get('tag') == 'summary']
    assert len(rows) >= 2
    for row in rows:
        assert all(np.isfinite(v) for v in row.values() if isinstance(v, float)), row
        assert np.isfinite(row['g_loss']) and np.isfinite(row['d_loss'])
    assert json.load(open(os.path.join(out, 'dataset_hparams.json')))['scale_size'] == 64
    cmd = ['timeout', '-k', '10', '180', sys.executable, os.path.join(ROOT, 'scripts', 'generate.py'), '--input_dir', str(data), '--dataset', 'bair',
           '--mode', 'val', '--checkpoint', out, '--results_dir', res, '--batch_size', '2', '--num_samples', '2', '--num_stochastic_samples', '1',
           '--dataset_hparams', hp]
    t0 = time.time()
    g = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print('scripts/generate.py: %.1f s' % (time.time() - t0))
    assert g.returncode == 0, g.stdout[-4000:]
    pngs = sorted(f for f in os.listdir(os.path.join(res, 'run')) if f.endswith('.png'))
    assert len(pngs) == 2 * 1 * 4                                                         # 2 sequences x 1 sample x 4 future frames
    for f in pngs:
        assert _png_size(os.path.join(res, 'run', f)) == (64, 64)

"""JPEG-encoded datasets on the device (pytest -m gpu): savp_jpeg_decode_u8 (csrc/jpeg_decode.hip), fed by the host entropy decoder of
libsavp_io.so, against pixels recorded from Pillow / libjpeg-turbo (tests/golden/jpeg_fixtures.npz); the three datasets end to end on
records written here; scripts/train.py + scripts/generate.py on sv2p-layout records.

The kernel restates libjpeg's integer arithmetic, so every comparison with decoded pixels is == on uint8 over every element: no tolerance,
no fixture left out.  Only the google_robot case goes on through the area resize, and is held to that kernel's own derived bound
(tests/test_gpu_input_resize.py: bound)."""
import io
import os
import struct
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import tfrecord as R
from tests import oracle_resize as OR
from video_prediction_amd import io as sio

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = 'cuda:0'
FIX = np.load(os.path.join(HERE, 'golden', 'jpeg_fixtures.npz'))
NAMES = [str(n) for n in FIX['names']]


def _jpeg(i):
    return FIX['jpeg_%d' % i].tobytes()


def _decode(streams, window=None, out_hw=None):
    """Host entropy decode of every stream (one geometry), then the kernel: uint8 [N, out_h, out_w, C] as numpy."""
    from video_prediction_amd import kernels as K
    info = sio.jpeg_info(streams[0])
    parts = [sio.jpeg_entropy_decode(s, info)[1:] for s in streams]
    coef = torch.from_numpy(np.stack([p[0] for p in parts])).to(DEV)
    qtab = torch.from_numpy(np.stack([p[1] for p in parts]).view(np.int16)).to(DEV)
    h, w = out_hw or (info.height, info.width)
    out = torch.empty((len(streams), h, w, info.components), dtype=torch.uint8, device=DEV)
    ws = torch.empty(K.jpeg_workspace_bytes(info, len(streams)), dtype=torch.uint8, device=DEV)
    win = None if window is None else torch.tensor(window, dtype=torch.int32, device=DEV).reshape(len(streams), 2)
    K.jpeg_decode_u8(coef, qtab, info, out, ws, window=win)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('i', range(len(NAMES)), ids=NAMES)
def test_single_frames_equal_the_recorded_pixels(i):
    got, want = _decode([_jpeg(i)])[0], FIX['pixels_%d' % i]
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), (NAMES[i], int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


def _groups():
    by = {}
    for i, n in enumerate(NAMES):
        by.setdefault(tuple(n.split()[1:3]), []).append(i)                      # (size, sampling)
    return {' '.join(k): v for k, v in by.items() if len(v) > 1}


@pytest.mark.parametrize('key', sorted(_groups()))
def test_mixed_quality_batches_equal_the_recorded_pixels(key):
    """Fixtures of one geometry stacked: every frame brings its own quantisation tables."""
    idx = _groups()[key]
    idx = idx + idx[::-1]                                                      # the same frames at other batch positions
    got = _decode([_jpeg(i) for i in idx])
    for k, i in enumerate(idx):
        assert np.array_equal(got[k], FIX['pixels_%d' % i]), (key, k, NAMES[i])


@pytest.mark.parametrize('name,size,windows', [
    ('photo 96x80 420', (40, 32), [(0, 0), (56, 48), (13, 7), (1, 47)]),        # dword stores; odd origins cut chroma pairs and rows
    ('photo 96x80 420', (33, 27), [(63, 53), (0, 1), (31, 30), (62, 0)]),       # byte stores
    ('photo 48x80 422', (48, 80), [(0, 0)] * 2),                               # the whole image through the window path
    ('photo 48x80 422', (5, 12), [(43, 68), (0, 3)]),
    ('photo 70x50 444', (9, 10), [(61, 40), (8, 8)]),
    ('photo 70x50 grey', (16, 8), [(54, 42), (3, 1)]),
    ('photo 70x50 grey', (7, 7), [(63, 43), (0, 0)]),
    ('photo 5x3 420', (2, 2), [(3, 1), (0, 0)]),
])
def test_window_output_is_the_slice_of_the_full_decode(name, size, windows):
    i = next(k for k, n in enumerate(NAMES) if n.startswith(name))
    full = FIX['pixels_%d' % i]
    got = _decode([_jpeg(i)] * len(windows), window=windows, out_hw=size)
    for k, (y0, x0) in enumerate(windows):
        assert np.array_equal(got[k], full[y0:y0 + size[0], x0:x0 + size[1]]), (name, size, (y0, x0))


def test_a_window_outside_the_image_is_clamped_into_it():
    """Windows live in device memory, so the launcher cannot check them: the kernel clamps, it never reads outside the planes."""
    i = next(k for k, n in enumerate(NAMES) if n.startswith('photo 96x80 420'))
    full = FIX['pixels_%d' % i]
    got = _decode([_jpeg(i)] * 3, window=[(-5, 1000), (90, -3), (2 ** 31 - 1, -2 ** 31)], out_hw=(40, 32))
    for k, (y0, x0) in enumerate([(0, 48), (56, 0), (56, 0)]):
        assert np.array_equal(got[k], full[y0:y0 + 40, x0:x0 + 32])


def test_bad_arguments_return_a_negative_code():
    import ctypes
    from video_prediction_amd import kernels as K, lib
    L = lib.get()
    i = next(k for k, n in enumerate(NAMES) if n.startswith('photo 70x50 420'))
    info, coef, qtab = sio.jpeg_entropy_decode(_jpeg(i))
    coef = torch.from_numpy(coef).to(DEV)
    qtab = torch.from_numpy(qtab.view(np.int16)).to(DEV)
    out = torch.empty((1, 70, 50, 3), dtype=torch.uint8, device=DEV)
    ws = torch.empty(K.jpeg_workspace_bytes(info, 1) + 16, dtype=torch.uint8, device=DEV)
    win = torch.zeros((1, 2), dtype=torch.int32, device=DEV)

    def args(**over):
        a = K.jpeg_args(info, 1)
        a.coef, a.qtab, a.out, a.ws, a.ws_bytes = coef.data_ptr(), qtab.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()
        for k, v in over.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a

    assert L.savp_jpeg_decode_u8(lib.stream(), ctypes.byref(args())) == 0
    bad = [dict(N=0), dict(width=0), dict(height=-1), dict(width=70000), dict(components=2), dict(components=4), dict(h=(0, 1)), dict(h=(0, 4)),
           dict(v=(0, 1)), dict(h=(1, 2)), dict(v=(2, 2)), dict(blocks_w=(0, 9)), dict(blocks_h=(1, 4)), dict(block_offset=(1, 1)),
           dict(total_blocks=info.total_blocks + 1), dict(out_h=69), dict(out_w=51), dict(coef=None), dict(qtab=None), dict(out=None),
           dict(ws=None), dict(ws_bytes=info.total_blocks * 64 - 1), dict(coef=coef.data_ptr() + 2), dict(qtab=qtab.data_ptr() + 8),
           dict(ws=ws.data_ptr() + 4), dict(window=win.data_ptr(), out_h=71), dict(window=win.data_ptr(), out_w=0),
           dict(window=win.data_ptr() + 2, out_h=8, out_w=8)]
    for over in bad:
        assert L.savp_jpeg_decode_u8(lib.stream(), ctypes.byref(args(**over))) < 0, over
    assert L.savp_jpeg_workspace_bytes(ctypes.byref(args(components=4))) < 0
    assert L.savp_jpeg_decode_u8(lib.stream(), None) < 0
    torch.cuda.synchronize()
    assert L.savp_jpeg_decode_u8(lib.stream(), ctypes.byref(args(window=win.data_ptr(), out_h=8, out_w=8))) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        K.jpeg_decode_u8(coef, qtab, info, torch.empty((1, 70, 50, 1), dtype=torch.uint8, device=DEV), ws)
    with pytest.raises(RuntimeError):
        K.jpeg_decode_u8(coef.float(), qtab, info, out, ws)


# ---- the datasets end to end, on streams encoded here ------------------------------------------------------------------------------
def _pillow():
    PIL = pytest.importorskip('PIL')
    from PIL import Image, features
    if not features.check('libjpeg_turbo'):
        pytest.skip('the reference pixels of these cases are libjpeg-turbo decodes')
    return Image


def _photo(rng, h, w):
    """Photograph-like content: smooth shading, hard edges, a little noise."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6, 3)
    img = np.stack([127 + 90 * np.sin(0.013 * xx * (k + 1) + ph[k]) * np.cos(0.011 * yy + k) + 50 * (((xx + 2 * yy) // 37 + k) % 3 == 0)
                    for k in range(3)], -1)
    return np.clip(np.rint(img + rng.normal(0, 5, img.shape)), 0, 255).astype(np.uint8)


def _encode_all(Image, rng, n, T, h, w, subsampling, quality):
    """(streams [n][T], Pillow's decode of them uint8 [n, T, h, w, 3])."""
    streams, pixels = [], np.empty((n, T, h, w, 3), np.uint8)
    for i in range(n):
        row = []
        for t in range(T):
            buf = io.BytesIO()
            Image.fromarray(_photo(rng, h, w)).save(buf, 'JPEG', quality=quality[(i + t) % len(quality)], subsampling=subsampling)
            row.append(buf.getvalue())
            pixels[i, t] = np.asarray(Image.open(io.BytesIO(row[-1])))
        streams.append(row)
    return streams, pixels


def test_google_robot_at_its_real_geometry_cropped_and_resized(tmp_path):
    from tests.test_gpu_input_resize import bound
    from video_prediction_amd.datasets import get_dataset_class
    Image = _pillow()
    rng = np.random.default_rng(21)
    n, T, B = 2, 4, 2
    streams, pixels = _encode_all(Image, rng, n, T, 512, 640, 2, (90, 75))
    states = rng.standard_normal((n, T, 5)).astype(np.float32)
    actions = rng.standard_normal((n, T - 1, 5)).astype(np.float32)
    d = tmp_path / 'push_testseen'
    d.mkdir()
    exs = []
    for i in range(n):
        feats = {'move/%d/image/encoded' % t: streams[i][t] for t in range(T)}
        feats.update({'move/%d/endeffector/vec_pitch_yaw' % t: [float(v) for v in states[i, t]] for t in range(T)})
        feats.update({'move/%d/commanded_pose/vec_pitch_yaw' % t: [float(v) for v in actions[i, t]] for t in range(T - 1)})
        exs.append(R.encode_example(feats))
    R.write_records(str(d / 'push_testseen.tfrecord-00000-of-00001'), exs)
    ds = get_dataset_class('google_robot')(str(d), mode='test', num_epochs=1, hparams='sequence_length=4,crop_size=512,scale_size=64,use_state=true')
    assert ds.image_shape == (512, 640, 3) and ds.output_image_shape == (64, 64, 3) and ds.num_examples_per_epoch() == 1038
    it = ds.make_batch(B)
    batch = next(it)
    got = batch['images']
    assert tuple(got.shape) == (B, T, 64, 64, 3) and got.dtype == torch.float32
    want = OR.preprocess(pixels, 512, 64)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print('google_robot 512x640 -> crop 512 -> 64: max abs err %.3e, bound %.3e' % (err, bound(512, 64)))
    assert err <= bound(512, 64), (err, bound(512, 64))
    assert np.array_equal(batch['states'].cpu().numpy(), states) and np.array_equal(batch['actions'].cpu().numpy(), actions)
    assert np.array_equal(it.dev_u8.cpu().numpy(), pixels)                      # and the decoded frames themselves: exact
    with pytest.raises(StopIteration):
        next(it)


def test_sv2p_without_resizing_is_exact(tmp_path):
    from video_prediction_amd.datasets import get_dataset_class
    Image = _pillow()
    rng = np.random.default_rng(22)
    n, T, B = 5, 7, 2
    streams, pixels = _encode_all(Image, rng, n, T, 64, 64, 2, (95, 60, 80))
    d = tmp_path / 'shape' / 'val'
    d.mkdir(parents=True)
    R.write_records(str(d / 'val.tfrecords'), [R.encode_example({'image_%d' % t: streams[i][t] for t in range(T)}) for i in range(n)])
    ds = get_dataset_class('sv2p')(str(tmp_path / 'shape'), mode='val', num_epochs=1)
    assert ds.hparams.sequence_length == 6 and ds.output_image_shape == (64, 64, 3)
    it = ds.make_batch(B)
    for k in range(n // B):
        got = next(it)
        assert set(got) == {'images'}
        want = pixels[k * B:(k + 1) * B, :6].astype(np.float32) * np.float32(1.0 / 255.0)
        assert np.array_equal(got['images'].cpu().numpy(), want)
    with pytest.raises(StopIteration):
        next(it)


def test_ucf101_with_random_crop(tmp_path):
    from video_prediction_amd.datasets import get_dataset_class
    Image = _pillow()
    rng = np.random.default_rng(23)
    lengths = [9, 5, 8, 10, 8]
    n, B = len(lengths), 2
    streams, pixels = _encode_all(Image, rng, n, max(lengths), 240, 320, 2, (85, 92))
    d = tmp_path / 'train'
    d.mkdir()
    R.write_records(str(d / 'sequence_0_to_4.tfrecords'),
                    [R.encode_example({'sequence_length': ('int64', [lengths[i]]), 'images/encoded': streams[i][:lengths[i]]}) for i in range(n)])
    DS = get_dataset_class('ucf101')
    ds = DS(str(d), mode='test', num_epochs=1, seed=3, hparams='random_crop_size=128')            # test mode: file order, time_shift 0
    assert ds.image_shape == (240, 320, 3) and ds.output_image_shape == (128, 128, 3) and ds.num_examples_per_epoch() == 5

    def run():
        out, wins = [], []
        it = DS(str(d), mode='test', num_epochs=1, seed=3, hparams='random_crop_size=128').make_batch(B)
        for batch in it:
            out.append(batch['images'].cpu().numpy())
            wins.append(it.seq_windows.copy())
        return np.concatenate(out), np.concatenate(wins)

    got, wins = run()
    kept = [i for i in range(n) if lengths[i] >= 8]
    assert got.shape == (4, 8, 128, 128, 3) and wins.shape == (4, 2)
    assert (wins >= 0).all() and (wins[:, 0] < 240 - 128).all() and (wins[:, 1] < 320 - 128).all() and len(set(map(tuple, wins))) > 1
    for k, i in enumerate(kept):
        y0, x0 = wins[k]
        want = pixels[i, :8, y0:y0 + 128, x0:x0 + 128].astype(np.float32) * np.float32(1.0 / 255.0)       # test mode: time_shift 0
        assert np.array_equal(got[k], want), (k, i, (y0, x0))
    again, wins2 = run()
    assert np.array_equal(wins, wins2) and np.array_equal(got, again)           # the windows come from the seed
    it = DS(str(d), mode='test', num_epochs=1).make_batch(B)                    # no random crop: whole frames
    assert np.array_equal(next(it)['images'].cpu().numpy(), pixels[[0, 2], :8].astype(np.float32) * np.float32(1.0 / 255.0))


# ---- the scripts -------------------------------------------------------------------------------------------------------------------
def _png_size(path):
    with open(path, 'rb') as f:
        head = f.read(24)
    assert head[:8] == b'\x89PNG\r\n\x1a\n' and head[12:16] == b'IHDR'
    return struct.unpack('>II', head[16:24])


def test_train_and_generate_scripts_on_sv2p_records(tmp_path):
    """Three train steps of a small SAVP (B = 2; sequence_length 6, context_frames 1: the sv2p 'shape' defaults) on JPEG records built from the
    committed 64 x 64 streams, then scripts/generate.py on the checkpoint it saved.  Each child process runs under a limit of its own, the
    one tests/test_gpu_input_resize.py uses for the same pair of commands."""
    import json
    same = [i for i, n in enumerate(NAMES) if ' 64x64 420 ' in n]
    data = tmp_path / 'shape'
    for mode in ('train', 'val'):
        (data / mode).mkdir(parents=True)
        exs = [R.encode_example({'image_%d' % t: _jpeg(same[(3 * i + t) % len(same)]) for t in range(8)}) for i in range(4)]
        R.write_records(str(data / mode / ('%s.tfrecords' % mode)), exs)
    out, res = str(tmp_path / 'run'), str(tmp_path / 'results')
    cmd = ['timeout', '-k', '10', '180', sys.executable, os.path.join(ROOT, 'scripts', 'train.py'), '--input_dir', str(data), '--dataset', 'sv2p',
           '--model', 'savp', '--output_dir', out, '--progress_freq', '1', '--summary_freq', '1', '--eval_summary_freq', '0', '--save_freq', '3',
           '--model_hparams', 'batch_size=2,max_steps=3,nz=8']
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print('scripts/train.py: %.1f s' % (time.time() - t0))
    assert r.returncode == 0, r.stdout[-4000:]
    assert 'progress  global step 3' in r.stdout and os.path.exists(os.path.join(out, 'model-3.index'))
    rows = [json.loads(l) for l in open(os.path.join(out, 'summaries.jsonl'))]
    rows = [row for row in rows if row.get('tag') == 'summary']
    assert len(rows) >= 3
    for row in rows:
        assert all(np.isfinite(v) for v in row.values() if isinstance(v, float)), row
        assert np.isfinite(row['g_loss']) and np.isfinite(row['d_loss'])
    assert json.load(open(os.path.join(out, 'dataset_hparams.json')))['sequence_length'] == 6
    cmd = ['timeout', '-k', '10', '180', sys.executable, os.path.join(ROOT, 'scripts', 'generate.py'), '--input_dir', str(data), '--dataset', 'sv2p',
           '--mode', 'val', '--checkpoint', out, '--results_dir', res, '--batch_size', '2', '--num_samples', '2', '--num_stochastic_samples', '1']
    t0 = time.time()
    g = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print('scripts/generate.py: %.1f s' % (time.time() - t0))
    assert g.returncode == 0, g.stdout[-4000:]
    pngs = sorted(f for f in os.listdir(os.path.join(res, 'run')) if f.endswith('.png'))
    assert len(pngs) == 2 * 1 * 5                                                         # 2 sequences x 1 sample x 5 future frames
    for f in pngs:
        assert _png_size(os.path.join(res, 'run', f)) == (64, 64)

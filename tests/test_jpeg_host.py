"""JPEG-encoded datasets, host side (CPU only): the NumPy yardstick tests/oracle_jpeg.py against pixels recorded from Pillow / libjpeg-turbo
(tests/golden/jpeg_fixtures.npz), the host entropy decoder of libsavp_io.so against the yardstick, its refusals and its behaviour on
truncated streams, the JPEG mode of the batched pipeline on records written here, and the class surfaces of the three datasets."""
import os

import numpy as np
import pytest

from oracle import tfrecord as R
from tests import oracle_jpeg as OJ
from video_prediction_amd import io as sio

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = np.load(os.path.join(HERE, 'golden', 'jpeg_fixtures.npz'))
NAMES = [str(n) for n in FIX['names']]
SAME = [i for i, n in enumerate(NAMES) if ' 64x64 420 ' in n]                 # one geometry, five quality / table / restart settings


def _jpeg(i):
    return FIX['jpeg_%d' % i].tobytes()


def test_fixture_file_covers_what_it_should():
    assert len(NAMES) >= 40 and len(SAME) >= 4
    for word in ('grey', '444', '422', '420', 'opt', 'rst', 'checker', 'primaries', 'noise', 'q100', 'q50'):
        assert any(word in n for n in NAMES), word
    shapes = [FIX['pixels_%d' % i].shape for i in range(len(NAMES))]
    assert any(h < 8 for h, w, c in shapes) and any(w < 8 for h, w, c in shapes) and any(w % 16 and ((w + 1) // 2) % 2 for h, w, c in shapes)
    assert os.path.getsize(os.path.join(HERE, 'golden', 'jpeg_fixtures.npz')) < 1 << 20
    assert 'libjpeg-turbo' in str(FIX['versions'][1])


@pytest.mark.parametrize('i', range(len(NAMES)), ids=NAMES)
def test_oracle_equals_pillow(i):
    """The yardstick itself: every sample equal to what libjpeg-turbo decoded."""
    assert np.array_equal(OJ.decode(_jpeg(i)), FIX['pixels_%d' % i])


@pytest.mark.parametrize('i', range(len(NAMES)), ids=NAMES)
def test_host_decoder_equals_oracle(i):
    data = _jpeg(i)
    p, coef, qtab = OJ.entropy_decode(data)
    assert sio.jpeg_info(data).as_dict() == OJ.info(data)
    info, got_coef, got_qtab = sio.jpeg_entropy_decode(data)
    assert got_coef.dtype == np.int16 and got_qtab.dtype == np.uint16
    assert np.array_equal(got_coef, coef) and np.array_equal(got_qtab, qtab)
    assert info.total_blocks == p['total_blocks'] == coef.shape[0]


def _with_segment(data, marker, payload, before=0xDA):
    """data with one more marker segment in front of the first `before` marker."""
    i = 2
    while data[i + 1] != before:
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    seg = bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, 'big') + payload
    return data[:i] + seg + data[i:]


def _patched_sof(data, marker=None, precision=None, sampling=None):
    i = 2
    while data[i + 1] not in (0xC0, 0xC1):
        i += 2 + ((data[i + 2] << 8) | data[i + 3])
    d = bytearray(data)
    if marker is not None:
        d[i + 1] = marker
    if precision is not None:
        d[i + 4] = precision
    if sampling is not None:
        d[i + 11] = sampling                                                   # first component's H << 4 | V
    return bytes(d)


def test_refusals_name_their_reason():
    base = _jpeg(SAME[0])
    cases = [(FIX['refuse_progressive'].tobytes(), 'progressive'), (FIX['refuse_cmyk'].tobytes(), '4 components'),
             (_patched_sof(base, marker=0xC9), 'arithmetic'), (_patched_sof(base, marker=0xC3), 'lossless'),
             (_patched_sof(base, precision=12), '12-bit'), (_patched_sof(base, sampling=0x12), 'sampling'),
             (_patched_sof(base, sampling=0x41), 'sampling'),
             (_with_segment(base, 0xDB, bytes([0x12]) + bytes(128)), '16-bit DQT'),
             (_with_segment(base, 0xEE, b'Adobe' + bytes([0, 100, 0, 0, 0, 0, 0])), 'Adobe')]
    for data, word in cases:
        for fn in (sio.jpeg_info, sio.jpeg_entropy_decode):
            with pytest.raises(sio.JpegError, match=word) as e:
                fn(data)
            assert e.value.code == sio.EUNSUPPORTED == -6, word
        with pytest.raises(OJ.Unsupported):
            OJ.parse(data)
    # harmless extras are skipped: COM, APPn, fill bytes in front of a marker, an Adobe marker that says YCbCr
    extra = _with_segment(_with_segment(base, 0xFE, b'a comment'), 0xE5, bytes(40))
    extra = _with_segment(extra, 0xEE, b'Adobe' + bytes([0, 100, 0, 0, 0, 0, 1]))
    i = extra.index(b'\xff\xda')
    extra = extra[:i] + b'\xff\xff\xff' + extra[i:]
    assert np.array_equal(sio.jpeg_entropy_decode(extra)[1], sio.jpeg_entropy_decode(base)[1])
    assert np.array_equal(OJ.decode(extra), OJ.decode(base))


def test_geometry_that_differs_from_the_expected_one_is_corrupt():
    expect = sio.jpeg_info(_jpeg(SAME[0]))
    other = next(i for i, n in enumerate(NAMES) if ' 64x64 444 ' in n)
    with pytest.raises(sio.JpegError, match='geometry') as e:
        sio.jpeg_entropy_decode(_jpeg(other), expect)
    assert e.value.code == sio.ECORRUPT


@pytest.mark.parametrize('i', [SAME[4], next(k for k, n in enumerate(NAMES) if n.startswith('noise 48x80 422'))], ids=['420 rst', '422 opt rst'])
def test_every_proper_prefix_is_an_error(i):
    """A truncated stream never decodes and never crashes; the bytes are handed over in a buffer of exactly their length
    (tests/tools/jpeg_sanitize.sh runs the same loop under AddressSanitizer / UBSan)."""
    data = _jpeg(i)
    full = sio.jpeg_info(data)
    for n in range(len(data)):
        with pytest.raises(sio.JpegError) as e:
            sio.jpeg_entropy_decode(data[:n], full)
        assert e.value.code == sio.ECORRUPT, n
        with pytest.raises(OJ.Corrupt):
            OJ.entropy_decode(data[:n])
    # and bytes flipped inside the scan either decode to something or fail cleanly
    rng = np.random.default_rng(i)
    for _ in range(200):
        d = bytearray(data)
        for k in rng.integers(2, len(d), 3):
            d[k] = int(rng.integers(0, 256))
        try:
            sio.jpeg_entropy_decode(bytes(d))
        except sio.JpegError as e:
            assert e.code in (sio.ECORRUPT, sio.EUNSUPPORTED)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
FRAMES = 9


def _fixture_of(idx, t):
    return SAME[(idx * 7 + t * 3) % len(SAME)]


def _write(d, fmt, n=6, floats=False, per_file=3):
    d.mkdir(parents=True)
    paths = []
    for f in range(n // per_file):
        exs = []
        for idx in range(f * per_file, (f + 1) * per_file):
            feats = {}
            for t in range(FRAMES):
                feats[fmt % t] = _jpeg(_fixture_of(idx, t))
                if floats:
                    feats['state_%d' % t] = [float(idx), float(t)]
                    if t < FRAMES - 1:
                        feats['action_%d' % t] = [float(idx), float(t) + 0.5]
            exs.append(R.encode_example(feats))
        paths.append(str(d / ('traj_%d_to_%d.tfrecords' % (f * per_file, (f + 1) * per_file - 1))))
        R.write_records(paths[-1], exs)
    return paths


COEF = {}


def _coef(fixture):
    if fixture not in COEF:
        COEF[fixture] = sio.jpeg_entropy_decode(_jpeg(fixture))[1:]
    return COEF[fixture]


@pytest.mark.parametrize('fmt', ['move/%d/image/encoded', 'image_%d'])
def test_pipeline_in_order_with_frame_skip(tmp_path, fmt):
    paths = _write(tmp_path / 'test', fmt, floats=True)
    pipe = sio.VideoPipeline(paths, fmt, FRAMES, (64, 64, 3), 4, 2, frame_skip=1, jpeg=True, decode_threads=3,
                             float_keys=[('state_%d', 2, 0), ('action_%d', 2, 1)])
    assert pipe.jpeg_info.as_dict() == OJ.info(_jpeg(SAME[0]))
    state_t, action_t = R.slice_times(FRAMES, 4, 1, 0)
    for k in range(3):
        coef, qtab, windows, (states, actions) = pipe.next_jpeg()
        assert windows is None and coef.shape == (2, 4, pipe.jpeg_info.total_blocks, 64) and qtab.shape == (2, 4, 3, 64)
        for b in range(2):
            idx = 2 * k + b
            for j, t in enumerate(state_t):
                want_coef, want_qtab = _coef(_fixture_of(idx, t))
                assert np.array_equal(coef[b, j], want_coef) and np.array_equal(qtab[b, j], want_qtab)
                assert list(states[b, j]) == [idx, t]
            assert np.array_equal(actions[b].reshape(-1, 2), [[idx, t + 0.5] for t in action_t])
    assert pipe.next_jpeg() is None
    with pytest.raises(RuntimeError):
        pipe.next()                                                            # the raw call on a jpeg pipeline
    pipe.close()


def test_pipeline_shuffle_and_time_shift_decode_the_frames_the_slicing_selects(tmp_path):
    paths = _write(tmp_path / 'train', 'image_%d', floats=True)
    pipe = sio.VideoPipeline(paths, 'image_%d', FRAMES, (64, 64, 3), 3, 2, frame_skip=1, time_shift=2, shuffle=True, num_epochs=3, seed=11,
                             jpeg=True, float_keys=[('state_%d', 2, 0)])
    seen, starts = [], set()
    while True:
        got = pipe.next_jpeg()
        if got is None:
            break
        coef, qtab, _, (states,) = got
        for b in range(2):
            idx, t0 = int(states[b, 0, 0]), int(states[b, 0, 1])
            times, _ = R.slice_times(FRAMES, 3, 1, t0)
            assert t0 % 2 == 0 and [int(t) for t in states[b, :, 1]] == times
            for j, t in enumerate(times):
                want_coef, want_qtab = _coef(_fixture_of(idx, t))
                assert np.array_equal(coef[b, j], want_coef) and np.array_equal(qtab[b, j], want_qtab)
            seen.append(idx)
            starts.add(t0)
    # the shuffle buffer spans the epochs (shuffle_and_repeat): every example three times in all, not in file order
    assert sorted(seen) == sorted(list(range(6)) * 3) and seen != sorted(seen)
    assert starts == {0, 2, 4}
    pipe.close()


def _write_varlen(d, lengths):
    d.mkdir(parents=True)
    exs = [R.encode_example({'sequence_length': ('int64', [n]), 'images/encoded': [_jpeg(_fixture_of(idx, t)) for t in range(n)]})
           for idx, n in enumerate(lengths)]
    path = str(d / ('sequence_0_to_%d.tfrecords' % (len(lengths) - 1)))
    R.write_records(path, exs)
    return [path]


def test_pipeline_varlen_layout_filters_short_sequences_and_draws_windows(tmp_path):
    lengths = [7, 2, 9, 5, 8, 6]
    paths = _write_varlen(tmp_path / 'test', lengths)
    kw = dict(var_len=True, jpeg=True, frame_skip=1, num_epochs=1)
    pipe = sio.VideoPipeline(paths, 'images/encoded', 0, (64, 64, 3), 3, 2, **kw)
    kept = [i for i, n in enumerate(lengths) if n >= 3]                        # the filter compares with sequence_length, as the reference does
    assert kept == [0, 2, 3, 4, 5]
    for k in range(len(kept) // 2):
        coef, qtab, windows, _ = pipe.next_jpeg()
        for b in range(2):
            idx = kept[2 * k + b]
            for j, t in enumerate(R.slice_times(lengths[idx], 3, 1, 0)[0]):
                assert np.array_equal(coef[b, j], _coef(_fixture_of(idx, t))[0])
    assert pipe.next_jpeg() is None                                            # the incomplete last batch is dropped
    pipe.close()
    # windows: in range, one per sequence, reproducible from the seed, different for another seed
    lengths = [6] * 40
    paths = _write_varlen(tmp_path / 'win', lengths)

    def windows_of(seed, crop):
        p = sio.VideoPipeline(paths, 'images/encoded', 0, (64, 64, 3), 3, 4, seed=seed, random_crop=crop, **kw)
        out = []
        while True:
            got = p.next_jpeg()
            if got is None:
                break
            assert got[2].shape == (4, 2) and got[2].dtype == np.int32
            out.append(got[2].copy())
        p.close()
        return np.concatenate(out)

    a, b, c = windows_of(5, 40), windows_of(5, 40), windows_of(6, 40)
    assert a.shape == (40, 2) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert a.min() >= 0 and a.max() < 24 and len(set(map(tuple, a))) > 20          # [0, 64 - 40): the upper bound is excluded
    assert not windows_of(5, 64).any()                                         # a window as large as the frame can only sit at the origin
    with pytest.raises(sio.JpegError, match='random_crop'):
        sio.VideoPipeline(paths, 'images/encoded', 0, (64, 64, 3), 3, 4, random_crop=65, **kw)


def test_pipeline_names_the_file_of_a_frame_with_another_geometry(tmp_path):
    d = tmp_path / 'test'
    d.mkdir()
    other = next(i for i, n in enumerate(NAMES) if ' 64x64 444 ' in n)
    good = R.encode_example({'image_%d' % t: _jpeg(SAME[t % len(SAME)]) for t in range(4)})
    bad = R.encode_example({'image_%d' % t: _jpeg(other if t == 2 else SAME[0]) for t in range(4)})
    truncated = R.encode_example({'image_%d' % t: _jpeg(SAME[0])[:-40 if t == 3 else None] for t in range(4)})
    paths = []
    for name, exs in (('a', [good, good]), ('b', [good, bad]), ('c', [truncated, good])):
        paths.append(str(d / ('%s.tfrecords' % name)))
        R.write_records(paths[-1], exs)
    pipe = sio.VideoPipeline(paths[:2], 'image_%d', 4, (64, 64, 3), 4, 1, jpeg=True, prefetch_batches=1)
    for _ in range(3):
        assert pipe.next_jpeg() is not None
    with pytest.raises(RuntimeError, match=r'frame 2 .*b\.tfrecords.*geometry'):
        pipe.next_jpeg()
    pipe.close()
    pipe = sio.VideoPipeline(paths[2:], 'image_%d', 4, (64, 64, 3), 4, 1, jpeg=True)
    with pytest.raises(RuntimeError, match=r'frame 3 .*c\.tfrecords'):
        pipe.next_jpeg()
    pipe.close()
    with pytest.raises(sio.JpegError, match='no SOI'):                         # raw records read as JPEG: refused when the pipeline is made
        raw = str(d / 'raw.tfrecords')
        R.write_records(raw, [R.encode_example({'image_%d' % t: bytes(64 * 64 * 3) for t in range(4)})])
        sio.VideoPipeline([raw], 'image_%d', 4, (64, 64, 3), 4, 1, jpeg=True)


def test_decode_threads_default_and_cap(tmp_path):
    """0 means 4, more than 16 means 16, and the result does not depend on the count."""
    paths = _write(tmp_path / 'test', 'image_%d')
    out = []
    for n in (0, 1, 16, 64):
        pipe = sio.VideoPipeline(paths, 'image_%d', FRAMES, (64, 64, 3), FRAMES, 3, jpeg=True, decode_threads=n)
        out.append(pipe.next_jpeg()[0])
        pipe.close()
    assert all(np.array_equal(out[0], o) for o in out[1:])
    src = open(os.path.join(os.path.dirname(HERE), 'video_prediction_amd', 'csrc_host', 'tfrecord_pipeline.cpp')).read()
    assert 'hardware_concurrency' not in src and 'decode_threads > 16 ? 16' in src


# order of (example, first frame) that the parent of the commit adding the JPEG mode delivers for the raw pipeline below
RAW_ORDER = [(7, 6), (9, 2), (10, 4), (6, 2), (8, 0), (11, 0), (14, 0), (13, 6), (12, 0), (1, 2), (2, 6), (5, 2), (0, 6), (3, 2), (5, 0), (8, 4),
             (4, 6), (9, 2), (7, 6), (10, 2), (11, 0), (6, 4), (12, 4), (0, 0), (2, 4), (3, 4), (1, 6), (14, 6), (4, 4), (13, 4)]


def test_raw_path_is_unchanged(tmp_path):
    """The raw (non-JPEG) pipeline draws the same random numbers and delivers the same bytes as before the JPEG mode existed."""
    paths, idx = [], 0
    for f in range(3):
        exs = []
        for _ in range(5):
            feats = {}
            for t in range(10):
                fr = np.full((4, 4, 3), idx, np.uint8)
                fr[0, 0, 1] = t
                feats['%d/image_aux1/encoded' % t] = fr.tobytes()
            exs.append(R.encode_example(feats))
            idx += 1
        paths.append(str(tmp_path / ('traj_%d_to_%d.tfrecords' % (f * 5, f * 5 + 4))))
        R.write_records(paths[-1], exs)
    pipe = sio.VideoPipeline(paths, '%d/image_aux1/encoded', 10, (4, 4, 3), 4, 3, time_shift=2, shuffle=True, shuffle_buffer=4, num_epochs=2, seed=7)
    got = []
    while True:
        batch = pipe.next()
        if batch is None:
            break
        for x in batch[0]:
            got.append((int(x[0, 0, 0, 0]), int(x[0, 0, 0, 1])))
            assert [int(v) for v in x[:, 0, 0, 1]] == [got[-1][1] + j for j in range(4)] and (x[:, 1] == got[-1][0]).all()
    assert got == RAW_ORDER
    with pytest.raises(RuntimeError):
        pipe.next_jpeg()
    pipe.close()
    with pytest.raises(RuntimeError):                                          # random_crop belongs to the jpeg mode
        sio.VideoPipeline(paths, '%d/image_aux1/encoded', 10, (4, 4, 3), 4, 3, random_crop=2)
    tiny = os.path.join(HERE, 'golden', 'tiny.tfrecords')
    from tests.golden.make_wire_fixtures import fixture_arrays
    pipe = sio.VideoPipeline([tiny], '%d/image_aux1/encoded', 3, (4, 4, 3), 3, 2)
    assert np.array_equal(pipe.next()[0], fixture_arrays()[0])
    pipe.close()


# ---- the datasets ----------------------------------------------------------------------------------------------------------------------
def test_registry_names():
    from video_prediction_amd import datasets as D
    assert D.get_dataset_class('google_robot') is D.GoogleRobotVideoDataset
    assert D.get_dataset_class('sv2p') is D.SV2PVideoDataset
    assert D.get_dataset_class('ucf101') is D.UCF101VideoDataset
    assert D.get_dataset_class('UCF101VideoDataset') is D.UCF101VideoDataset
    for name in ('bair', 'kth', 'cartgripper'):
        assert D.get_dataset_class(name).jpeg_encoding.fget(object()) is False
    with pytest.raises(ValueError, match='Invalid dataset'):
        D.get_dataset_class('moving_mnist')


def test_sv2p_class_surface(tmp_path):
    from video_prediction_amd.datasets import SV2PVideoDataset
    for variant in ('shape', 'humans'):
        for mode in ('train', 'val'):
            _write(tmp_path / variant / mode, 'image_%d', floats=True)
    ds = SV2PVideoDataset(str(tmp_path / 'shape'), mode='train')
    assert ds.jpeg_encoding is True and ds.dataset_name == 'shape' and ds.image_shape == ds.output_image_shape == (64, 64, 3)
    hp = ds.hparams
    assert (hp.context_frames, hp.sequence_length, hp.time_shift, hp.use_state) == (1, 6, 0, False)
    assert ds.num_examples_per_epoch() == 43415 and ds.state_like_names_and_shapes == {'images': ('image_%d', (64, 64, 3))}
    assert SV2PVideoDataset(str(tmp_path / 'shape'), mode='val').num_examples_per_epoch() == 2898
    ds = SV2PVideoDataset(str(tmp_path / 'shape'), mode='val', hparams='use_state=true')
    assert ds.state_like_names_and_shapes['states'] == ('state_%d', (2,)) and ds.action_like_names_and_shapes['actions'] == ('action_%d', (2,))
    pipe = ds.make_pipeline(2)
    coef, qtab, _, (states, actions) = pipe.next_jpeg()
    assert coef.shape[:2] == (2, 6) and states.shape == (2, 6, 2) and actions.shape == (2, 5, 2)
    pipe.close()
    ds = SV2PVideoDataset(str(tmp_path / 'humans'), mode='train')
    hp = ds.hparams
    assert (hp.context_frames, hp.sequence_length, hp.time_shift, hp.use_state) == (10, 20, 1, False)
    assert ds.num_examples_per_epoch() == 23910
    with pytest.raises(ValueError, match='use_state'):
        SV2PVideoDataset(str(tmp_path / 'humans'), mode='train', hparams='use_state=true')
    _write(tmp_path / 'other' / 'train', 'image_%d')
    with pytest.raises(NotImplementedError):
        SV2PVideoDataset(str(tmp_path / 'other'), mode='train')
    ds = SV2PVideoDataset(str(tmp_path / 'shape'), mode='val', hparams='scale_size=32')
    assert ds.crop_and_scale == (64, 32) and ds.output_image_shape == (32, 32, 3)


def test_google_robot_class_surface_and_component_check(tmp_path):
    from video_prediction_amd.datasets import GoogleRobotVideoDataset, SV2PVideoDataset
    DS = GoogleRobotVideoDataset
    d = _write(tmp_path / 'push_train', 'move/%d/image/encoded')
    with pytest.raises(ValueError, match=r'64 x 64 with 3 component\(s\)'):     # not the declared 512 x 640 x 3
        DS(str(tmp_path / 'push_train'))
    assert DS.get_default_hparams_dict(object.__new__(DS))['sequence_length'] == 15
    assert DS.get_default_hparams_dict(object.__new__(DS))['context_frames'] == 2
    assert DS.jpeg_encoding.fget(object()) is True
    for name, count in (('push_train', 51615), ('push_testseen', 1038), ('push_testnovel', 995)):
        ds = object.__new__(DS)
        ds.input_dir = str(tmp_path / name)
        assert ds.num_examples_per_epoch() == count
    ds.input_dir = str(tmp_path / 'elsewhere')
    with pytest.raises(NotImplementedError):
        ds.num_examples_per_epoch()
    # a grey stream where three components are declared
    grey = next(i for i, n in enumerate(NAMES) if ' 48x80 grey ' in n)
    g = tmp_path / 'shape' / 'train'
    g.mkdir(parents=True)
    R.write_records(str(g / 'x.tfrecords'), [R.encode_example({'image_%d' % t: _jpeg(grey) for t in range(6)})])
    with pytest.raises(ValueError, match=r'1 component\(s\)'):
        SV2PVideoDataset(str(tmp_path / 'shape'), mode='train')
    assert d


def test_ucf101_class_surface(tmp_path):
    from video_prediction_amd.datasets import UCF101VideoDataset as DS
    hp = DS.get_default_hparams_dict(object.__new__(DS))
    assert (hp['context_frames'], hp['sequence_length'], hp['random_crop_size'], hp['use_state']) == (4, 8, 0, False)
    assert DS.var_len is True and DS.jpeg_encoding.fget(object()) is True
    _write_varlen(tmp_path / 'train', [8, 9])
    for bad in ('crop_size=64', 'scale_size=64'):
        with pytest.raises(NotImplementedError):
            DS(str(tmp_path), mode='train', hparams=bad)
    with pytest.raises(ValueError, match='64 x 64'):                          # the records here are not 240 x 320
        DS(str(tmp_path), mode='train')
    ds = object.__new__(DS)
    ds.filenames = ['/x/sequence_0_to_99.tfrecords', '/x/sequence_100_to_149.tfrecords']
    assert ds.num_examples_per_epoch() == 150


def test_jpeg_wrapper_has_no_cpu_path(hip_lib):
    import torch
    from video_prediction_amd import kernels as K
    info = sio.jpeg_info(_jpeg(SAME[0]))
    assert K.jpeg_workspace_bytes(info, 3) == 3 * info.total_blocks * 64
    coef = torch.zeros(1, info.total_blocks, 64, dtype=torch.int16)
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.jpeg_decode_u8(coef, torch.zeros(1, 3, 64, dtype=torch.int16), info, torch.zeros(1, 64, 64, 3, dtype=torch.uint8),
                         torch.zeros(10, dtype=torch.uint8))
    bad = info.as_dict()
    bad['h'] = [1, 2, 1]
    with pytest.raises(ValueError):
        K.jpeg_workspace_bytes(bad, 1)

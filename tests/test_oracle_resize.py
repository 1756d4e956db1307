"""tests/oracle_resize.py (the unpinned float64 restatement of crop_size / scale_size preprocessing) against known answers that do not
depend on the restatement being right, and the host side of the datasets that use it: crop_size / scale_size are accepted by bair and kth,
and 'cartgripper' resolves, reports the reference's defaults and parses 48 x 64 records with states and actions.  CPU only."""
import numpy as np
import pytest

from oracle import tfrecord as R
from tests import oracle_resize as OR

RATIOS = [(64, 128), (48, 64), (64, 48), (7, 3), (32, 64), (128, 64), (5, 3), (3, 5), (65, 64)]


def test_integer_factor_area_is_the_block_mean():
    rng = np.random.default_rng(0)
    for crop, S in ((128, 64), (64, 16), (9, 3)):
        k = crop // S
        img = rng.integers(0, 256, (2, crop, crop, 3), dtype=np.uint8)
        want = img.astype(np.float64).reshape(2, S, k, S, k, 3).mean(axis=(2, 4)) / 255.0
        assert np.allclose(OR.preprocess(img, scale_size=S), want, rtol=0, atol=1e-14)


def test_bilinear_2x_of_a_ramp_repeats_the_last_value():
    w = OR.bilinear_weights(4, 8)
    assert np.array_equal(w @ np.arange(4.0), [0, .5, 1, 1.5, 2, 2.5, 3, 3])
    ramp = np.tile(np.arange(4, dtype=np.uint8)[None, :, None], (4, 1, 1))                     # [4, 4, 1], value = column
    out = OR.preprocess(ramp, scale_size=8) * 255.0
    assert np.allclose(out[:, :, 0], np.tile([0, .5, 1, 1.5, 2, 2.5, 3, 3], (8, 1)), rtol=0, atol=1e-13)
    assert np.allclose(OR.preprocess(ramp.transpose(1, 0, 2), scale_size=8)[:, :, 0], out[:, :, 0].T / 255.0, rtol=0, atol=1e-15)


def test_this_is_not_half_pixel_bilinear_nor_adaptive_pooling():
    """torch.nn.functional.interpolate(mode='bilinear') uses half-pixel centres, mode='area' equal weights: neither is the reference's op."""
    import torch
    import torch.nn.functional as F
    x = torch.arange(4.0, dtype=torch.float64).view(1, 1, 1, 4).repeat(1, 1, 4, 1)
    half = F.interpolate(x, size=(8, 8), mode='bilinear', align_corners=False)[0, 0, 0].numpy()
    assert not np.allclose(half, OR.bilinear_weights(4, 8) @ np.arange(4.0))
    x7 = torch.arange(7.0, dtype=torch.float64).view(1, 1, 1, 7).repeat(1, 1, 7, 1) ** 2
    pool = F.interpolate(x7, size=(3, 3), mode='area')[0, 0, 0].numpy()
    assert not np.allclose(pool, OR.area_weights(7, 3) @ (np.arange(7.0) ** 2))


def test_area_weights_of_7_to_3_by_hand():
    """s = 7/3: cell 0 = [0, 7/3) takes 1, 1, 1/3 of pixels 0, 1, 2; cell 1 = [7/3, 14/3) takes 2/3, 1, 2/3 of pixels 2, 3, 4; all over s."""
    w = OR.area_weights(7, 3) * (7.0 / 3.0)
    want = np.zeros((3, 7))
    want[0, :3] = [1, 1, 1 / 3]
    want[1, 2:5] = [2 / 3, 1, 2 / 3]
    want[2, 4:] = [1 / 3, 1, 1]
    assert np.allclose(w, want, rtol=0, atol=1e-15)


@pytest.mark.parametrize('crop,S', RATIOS)
def test_every_weight_row_sums_to_one_and_a_constant_stays_constant(crop, S):
    w = OR.resize_weights(crop, S)
    assert w.shape == (S, crop) and (w >= 0).all()
    assert np.allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    img = np.full((crop, crop, 3), 173, dtype=np.uint8)
    assert np.allclose(OR.preprocess(img, scale_size=S), 173 / 255.0, rtol=0, atol=1e-15)


def test_crop_and_pad_offsets():
    assert OR.crop_or_pad_offsets(64, 48) == (8, 0)
    assert OR.crop_or_pad_offsets(65, 64) == (0, 0)                                           # the odd pixel is dropped at the far end
    assert OR.crop_or_pad_offsets(47, 64) == (0, 8)                                           # 8 zeros in front, 9 behind
    assert OR.crop_or_pad_offsets(64, 64) == (0, 0)
    rng = np.random.default_rng(1)
    img = rng.integers(1, 256, (47, 65, 2), dtype=np.uint8)                                    # no zeros inside
    out = OR.crop_or_pad(img, 64)
    assert out.shape == (64, 64, 2)
    assert np.array_equal(out[8:55], img[:, :64]) and not out[:8].any() and not out[55:].any()
    img = rng.integers(0, 256, (3, 64, 64, 3), dtype=np.uint8)
    assert np.array_equal(OR.crop_or_pad(img, 48), img[:, 8:56, 8:56])


def test_crop_equal_to_scale_is_the_identity_and_min_side_is_the_default_crop():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    assert OR.resolve(img.shape[-3:], 0, 64) == (48, 64) and OR.resolve(img.shape[-3:], 0, 0) == (48, 48)
    assert OR.resolve(img.shape[-3:], 32, 0) == (32, 32)
    assert np.array_equal(OR.preprocess(img, crop_size=48), img[:, :, 8:56].astype(np.float64) / 255.0)
    assert np.array_equal(OR.preprocess(img, crop_size=48, scale_size=48), OR.preprocess(img, crop_size=48))
    assert np.array_equal(OR.preprocess(img, scale_size=64), OR.preprocess(img[:, :, 8:56], scale_size=64))


def test_padding_zeros_are_resized_with_the_image():
    img = np.full((2, 4, 1), 255, dtype=np.uint8)                                              # 2 rows: one zero row in front, one behind
    out = OR.preprocess(img, crop_size=4, scale_size=8)[:, :, 0]
    assert np.allclose(out[:, 0], [0, .5, 1, 1, 1, .5, 0, 0], rtol=0, atol=1e-15)


def test_error_bound_tap_counts():
    assert OR.taps(64, 128) == 4 and OR.taps(64, 64) == 1
    assert OR.taps(128, 64) == 9 and OR.taps(64, 48) == 9 and OR.taps(7, 3) == 16


# ---- host side of the datasets ---------------------------------------------------------------------------------------------------
def _write_bair(d, frames):
    d.mkdir(parents=True)
    n, T = frames.shape[:2]
    R.write_records(str(d / ('traj_0_to_%d.tfrecords' % (n - 1))),
                    [R.encode_example({'%d/image_aux1/encoded' % t: frames[i, t].tobytes() for t in range(T)}) for i in range(n)])


def _write_kth(d, frames):
    d.mkdir(parents=True)
    n, T, H, W, C = frames.shape
    R.write_records(str(d / ('sequence_0_to_%d.tfrecords' % (n - 1))),
                    [R.encode_example({'sequence_length': ('int64', [T]), 'height': ('int64', [H]), 'width': ('int64', [W]),
                                       'channels': ('int64', [C]), 'images/encoded': [frames[i, t].tobytes() for t in range(T)]})
                     for i in range(n)])


def _write_cartgripper(d, frames, states, actions):
    d.mkdir(parents=True)
    n, T = frames.shape[:2]
    exs = []
    for i in range(n):
        feats = {}
        for t in range(T):
            feats['%d/image_view0/encoded' % t] = frames[i, t].tobytes()
            feats['%d/endeffector_pos' % t] = [float(v) for v in states[i, t]]
            if t < T - 1:
                feats['%d/action' % t] = [float(v) for v in actions[i, t]]
        exs.append(R.encode_example(feats))
    R.write_records(str(d / ('traj_0_to_%d.tfrecords' % (n - 1))), exs)


def test_bair_accepts_crop_size_and_scale_size(tmp_path):
    from video_prediction_amd.datasets import get_dataset_class
    frames = np.random.default_rng(3).integers(0, 256, (4, 8, 16, 16, 3), dtype=np.uint8)
    _write_bair(tmp_path / 'test', frames)
    DS = get_dataset_class('bair')
    ds = DS(str(tmp_path), mode='test', num_epochs=1, hparams='sequence_length=6,time_shift=0,scale_size=32')
    assert ds.image_shape == (16, 16, 3) and ds.output_image_shape == (32, 32, 3) and ds.crop_and_scale == (16, 32)
    pipe = ds.make_pipeline(2)
    images, _ = pipe.next()
    assert images.shape == (2, 6, 16, 16, 3) and np.array_equal(images, frames[:2, :6])         # the pipeline still delivers the records' frames
    pipe.close()
    ds = DS(str(tmp_path), mode='test', hparams='crop_size=12')
    assert ds.output_image_shape == (12, 12, 3) and ds.crop_and_scale == (12, 12)
    ds = DS(str(tmp_path), mode='test', hparams_dict=dict(crop_size=12, scale_size=8))
    assert ds.output_image_shape == (8, 8, 3) and ds.crop_and_scale == (12, 8)
    ds = DS(str(tmp_path), mode='test')
    assert ds.output_image_shape == ds.image_shape == (16, 16, 3) and ds.crop_and_scale is None


def test_kth_accepts_crop_size_and_scale_size(tmp_path):
    from video_prediction_amd.datasets import get_dataset_class
    frames = np.random.default_rng(4).integers(0, 256, (3, 10, 16, 20, 1), dtype=np.uint8)
    _write_kth(tmp_path / 'train', frames)
    ds = get_dataset_class('kth')(str(tmp_path), mode='train', num_epochs=1, hparams='sequence_length=10,crop_size=12,scale_size=24')
    assert ds.image_shape == (16, 20, 1) and ds.output_image_shape == (24, 24, 1) and ds.crop_and_scale == (12, 24)
    ds = get_dataset_class('kth')(str(tmp_path), mode='train', num_epochs=1, hparams='sequence_length=10,scale_size=8')
    assert ds.crop_and_scale == (16, 8)                                                        # crop defaults to the shorter side
    pipe = ds.make_pipeline(3)
    images, _ = pipe.next()
    assert images.shape == (3, 10, 16, 20, 1)
    pipe.close()


def test_cartgripper_dataset_defaults_and_records(tmp_path):
    from video_prediction_amd.datasets import CartgripperVideoDataset, get_dataset_class
    rng = np.random.default_rng(5)
    n, T = 4, 15
    frames = rng.integers(0, 256, (n, T, 48, 64, 3), dtype=np.uint8)
    states = rng.standard_normal((n, T, 6)).astype(np.float32)
    actions = rng.standard_normal((n, T - 1, 3)).astype(np.float32)
    _write_cartgripper(tmp_path / 'val', frames, states, actions)
    DS = get_dataset_class('cartgripper')
    assert DS is CartgripperVideoDataset
    ds = DS(str(tmp_path), mode='val', num_epochs=1)
    hp = ds.hparams                                                                            # cartgripper_dataset.py:16-24
    assert (hp.context_frames, hp.sequence_length, hp.time_shift, hp.use_state) == (2, 15, 3, True)
    assert hp.long_sequence_length == 30 and hp.crop_size == 0 and hp.scale_size == 0          # softmotion's, inherited
    assert ds.image_key_fmt == '%d/image_view0/encoded' and ds.image_shape == (48, 64, 3) and ds._max_sequence_length == T
    assert ds.state_like_names_and_shapes == {'images': ('%d/image_view0/encoded', (48, 64, 3)), 'states': ('%d/endeffector_pos', (6,))}
    assert ds.action_like_names_and_shapes == {'actions': ('%d/action', (3,))}
    assert ds.output_image_shape == (48, 64, 3) and ds.num_examples_per_epoch() == n and not ds.jpeg_encoding
    pipe = ds.make_pipeline(2)
    for k in range(2):
        images, (st, ac) = pipe.next()
        assert np.array_equal(images, frames[2 * k:2 * k + 2])
        assert np.array_equal(st, states[2 * k:2 * k + 2]) and np.array_equal(ac, actions[2 * k:2 * k + 2])
    assert pipe.next() is None
    pipe.close()
    ds = DS(str(tmp_path), mode='val', hparams='scale_size=64,use_state=false')
    assert ds.crop_and_scale == (48, 64) and ds.output_image_shape == (64, 64, 3) and ds.action_like_names_and_shapes == {}


def test_cartgripper_refuses_records_of_another_frame_size(tmp_path):
    from video_prediction_amd.datasets import get_dataset_class
    frames = np.zeros((1, 4, 32, 32, 3), dtype=np.uint8)
    _write_cartgripper(tmp_path / 'train', frames, np.zeros((1, 4, 6), np.float32), np.zeros((1, 3, 3), np.float32))
    with pytest.raises(ValueError, match='48 x 64'):
        get_dataset_class('cartgripper')(str(tmp_path), mode='train')


def test_resize_wrapper_has_no_cpu_path():
    import torch
    from video_prediction_amd import kernels as K
    with pytest.raises(RuntimeError, match='no CPU path'):
        K.u8_frames_resize_f32(torch.zeros(1, 1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 1, 8, 8, 3), 4)

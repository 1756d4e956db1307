"""Host half of the TensorBoard summaries (video_prediction_amd/summaries.py): the event-file writer read back through a CRC-checking
TFRecord reader and protobuf classes built at run time, the GIF encoder, the tag rules, and the numpy references the GPU tests
(tests/test_gpu_summaries.py) compare the kernels with."""
import os
import struct
import sys

import numpy as np

from tests import oracle_summaries as OS
from video_prediction_amd import summaries as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grey_frames(T=3, H=5, W=7):
    # consecutive frames differ (Pillow merges identical neighbours into one longer frame)
    return ((np.arange(T * H * W).reshape(T, H, W, 1) * 37 + np.arange(T).reshape(T, 1, 1, 1) * 11) % 256).astype(np.uint8)


def _rgb_frames(T=4, H=6, W=5):
    # at most 256 distinct colours per frame: the adaptive palette then holds every one of them
    rng = np.random.RandomState(3)
    palette = rng.randint(0, 256, size=(40, 3)).astype(np.uint8)
    return palette[rng.randint(0, 40, size=(T, H, W))]


def test_event_file_round_trip(tmp_path):
    w = S.EventFileWriter(str(tmp_path))
    scalars = {'g_loss': 0.1, 'eval_psnr/min': 23.456789, 'gen_l1_loss': 1e-30}
    w.add_scalars(scalars, 7)
    w.add_scalars({'psnr': 3.25}, 7, tag_suffix='_1')
    grey, rgb = _grey_frames(), _rgb_frames()
    w.add_gifs({'masks': grey, 'eval_gen_images_psnr/max': rgb}, 12, tag_suffix='_1')
    w.flush()
    w.close()
    files = os.listdir(str(tmp_path))
    assert len(files) == 1 and files[0].startswith('events.out.tfevents.')
    stamp, host = files[0][len('events.out.tfevents.'):].split('.', 1)
    assert stamp.isdigit() and host
    events = OS.read_events(os.path.join(str(tmp_path), files[0]))
    assert len(events) == 4
    assert events[0].file_version == 'brain.Event:2' and events[0].wall_time > 1e9 and not events[0].HasField('summary')
    assert [e.step for e in events[1:]] == [7, 7, 12]
    assert all(e.wall_time > 1e9 for e in events)
    got = {v.tag: v.simple_value for v in events[1].summary.value}
    want = {'g_loss/g_loss': 0.1, 'eval_psnr/eval_psnr/min': 23.456789, 'gen_l1_loss/gen_l1_loss': 1e-30}
    assert set(got) == set(want)
    for k in want:                                                 # exact as float32
        assert struct.pack('<f', got[k]) == struct.pack('<f', want[k]), k
    assert [(v.tag, v.simple_value) for v in events[2].summary.value] == [('psnr_1/psnr', 3.25)]
    vals = {v.tag: v.image for v in events[3].summary.value}
    assert set(vals) == {'masks_1/masks/gif', 'eval_gen_images_psnr_1/eval_gen_images_psnr/max/gif'}
    im = vals['masks_1/masks/gif']
    assert (im.height, im.width, im.colorspace) == (5, 7, 1)
    frames, durations = OS.decode_gif(im.encoded_image_string)
    assert durations == [250] * 3                                  # fps 4
    assert np.array_equal(frames[..., 0], grey[..., 0]) and np.array_equal(frames[..., 1], grey[..., 0])
    im = vals['eval_gen_images_psnr_1/eval_gen_images_psnr/max/gif']
    assert (im.height, im.width, im.colorspace) == (6, 5, 3)
    frames, durations = OS.decode_gif(im.encoded_image_string)
    assert durations == [250] * 4 and np.array_equal(frames, rgb)


def test_hand_encoding_agrees_with_protobuf():
    Event, _ = OS.event_classes()
    ev = Event(wall_time=1234.5, step=1 << 40)
    v = ev.summary.value.add(tag='a/b', simple_value=0.3)
    v = ev.summary.value.add(tag='c/c/gif')
    v.image.height, v.image.width, v.image.colorspace, v.image.encoded_image_string = 4, 300, 3, b'GIF89a\x00\xff'
    ours = S.encode_event(1234.5, step=1 << 40, values=[S.encode_scalar_value('a/b', 0.3),
                                                        S.encode_image_value('c/c/gif', 4, 300, 3, b'GIF89a\x00\xff')])
    back = Event()
    back.ParseFromString(ours)
    assert back == ev
    first = Event()
    first.ParseFromString(S.encode_event(2.0, file_version=S.FILE_VERSION))
    assert first.file_version == 'brain.Event:2' and first.wall_time == 2.0 and first.step == 0


def test_encode_gif_matches_the_files_generate_py_wrote(tmp_path):
    """scripts/generate.py:write_gif goes through encode_gif now: same bytes as Pillow saving to the path with the same settings."""
    from PIL import Image
    sys.path.insert(0, ROOT)
    from scripts import generate as G
    for frames, fps in ((_grey_frames(), 4), (_rgb_frames(), 4), (np.random.RandomState(0).randint(0, 256, (3, 16, 16, 3)).astype(np.uint8), 7)):
        p0, p1 = str(tmp_path / 'a.gif'), str(tmp_path / 'b.gif')
        imgs = [Image.fromarray(f[..., 0], 'L') if f.shape[-1] == 1 else Image.fromarray(f, 'RGB') for f in frames]
        imgs[0].save(p0, save_all=True, append_images=imgs[1:], duration=max(1, int(round(1000.0 / max(fps, 1)))), loop=0)
        G.write_gif(p1, frames, fps)
        assert open(p0, 'rb').read() == open(p1, 'rb').read() == S.encode_gif(frames, fps)


def test_add_tag_suffix():
    assert S.add_tag_suffix('loss', '_1') == 'loss_1'
    assert S.add_tag_suffix('psnr/psnr', '_1') == 'psnr_1/psnr'
    assert S.add_tag_suffix('eval_psnr/eval_psnr/min', '_1') == 'eval_psnr_1/eval_psnr/min'
    assert S.summary_tag('gen_images', gif=True) == 'gen_images/gen_images/gif'
    assert S.summary_tag('eval_ssim/avg') == 'eval_ssim/eval_ssim/avg'


def test_board_references_agree():
    rng = np.random.RandomState(1)
    for shape in ((3, 2, 4, 5, 3), (3, 3, 4, 5, 1), (2, 2, 4, 5, 3, 3), (2, 3, 3, 2, 1, 4)):
        x = rng.uniform(-0.25, 1.25, size=shape).astype(np.float32)
        a, b = OS.board_index(x), OS.board_concat(x)
        M = shape[5] if len(shape) == 6 else 1
        assert a.shape == (shape[0], M * shape[2], shape[1] * shape[3], shape[4]) and a.dtype == np.uint8
        assert np.array_equal(a, b), shape


def test_u8_reference_known_answers():
    f = np.float32
    x = np.array([0.0, -0.0, 1.0, 1 - 2.0 ** -24, 1 / 255.5, 127 / 255.5, 254 / 255.5, 255 / 255.5, 1e9, -1e9, 0.5, np.nan], f)
    want = [0, 0, 255, 255, None, None, None, 255, 255, 0, 127, 0]
    got = OS.u8(x)
    for g, w_, v in zip(got, want, x):
        if w_ is not None:
            assert g == w_, (v, g, w_)
        else:                                                       # k / 255.5 rounded to float32 lands on k or just below it
            k = int(round(float(v) * 255.5))
            assert g in (k - 1, k), (v, g)


def test_hsv_reference_against_matplotlib():
    from matplotlib.colors import hsv_to_rgb
    rng = np.random.RandomState(2)
    h, v = rng.uniform(0, 1, 500), rng.uniform(0, 1, 500)
    h[:7] = np.arange(7) / 6.0 - np.array([0, 0, 0, 0, 0, 0, 1e-12])          # the category boundaries, h < 1
    s = np.ones_like(h)
    ours = OS.hsv_to_rgb64(h, s, v)
    ref = hsv_to_rgb(np.stack([h, s, v], -1))
    assert float(np.abs(ours - ref).max()) < 1e-12

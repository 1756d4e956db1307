"""TensorBoard summaries: the event-file writer, the GIF encoder and the tag rules behind scripts/train.py's four summary frequencies.

What the reference gets from tf.summary.FileWriter, utils/gif_summary.py and utils/tf_utils.py:205-268 (add_scalar_summaries /
add_gif_summaries), without TensorFlow: an event file TensorBoard reads, scalars as `simple_value`, image boards as animated GIFs inside
`Summary.Value.image` (what gif_summary produces: TensorBoard's image dashboard plays them).  The boards themselves are built on the
device (kernels.summary_board_u8, csrc/summary.hip); this module is host code only.

Wire format (tensorflow/core/util/event.proto, framework/summary.proto; protobuf encoded by hand like checkpoint.py):
    file    = TFRecord framing of serialized Event messages (uint64 length, masked crc32c, data, masked crc32c: io.masked_crc32c)
    Event   { wall_time = 1 (double), step = 2 (int64), file_version = 3 (string) | summary = 5 (Summary) }
    Summary { value = 1 (repeated Value) }
    Value   { tag = 1 (string), simple_value = 2 (float), image = 4 (Image) }
    Image   { height = 1, width = 2, colorspace = 3 (int32), encoded_image_string = 4 (bytes) }
The first record is Event{wall_time, file_version = "brain.Event:2"}.

Tags.  A tensor or scalar called `name` gets the tag `<scope>/<name>` with scope = name.split('/')[0] (tf_utils._as_name_scope_map opens
a name scope per first component, so 'gen_images' becomes 'gen_images/gen_images' and 'eval_psnr/min' becomes 'eval_psnr/eval_psnr/min');
GIFs append '/gif' (gif_summary's op name); validation summaries rename the scope to `scope_1`, the accumulated evaluation of the
long_sequence_length model to `scope_2` (add_tag_suffix, reference scripts/train.py:18-26,301-318).  The validation scalars include the
losses (g_loss_1/g_loss, gen_l1_loss_1/gen_l1_loss, ...), taken by a forward-only pass (SAVPEngine.eval_losses).  TensorFlow's outer name scopes (towers) and the `_1`, `_2` suffixes it appends to make op names unique are NOT
reproduced: a dashboard of this writer shows the same groups with cleaner names.

Out of scope (also DESIGN.md): the `pr_curve`-hack plot summaries of add_plot_and_scalar_summaries (they need a patched TensorBoard; the
scalar half is written), boards of `gen_images_samples`, histograms and graph defs.
"""
import io as _io
import os
import socket
import struct
import time

import numpy as np

from . import io as sio
from .checkpoint import _enc_varint

FILE_VERSION = b'brain.Event:2'
GIF_FPS = 4                         # tf_utils.py:241
MAX_OUTPUTS = 8                     # add_gif_summaries(max_outputs=8)


# -- tags ---------------------------------------------------------------------------------------------------------------------------------
def summary_tag(name, gif=False):
    """`<scope>/<name>` (+ '/gif'), scope = the name's first component (tf_utils._as_name_scope_map)."""
    return name.split('/')[0] + '/' + name + ('/gif' if gif else '')


def add_tag_suffix(tag, tag_suffix):
    """reference scripts/train.py:18-26 on one tag: 'a/b/c' -> 'a<suffix>/b/c'."""
    parts = tag.split('/')
    return '/'.join([parts[0] + tag_suffix] + parts[1:])


# -- protobuf, by hand -----------------------------------------------------------------------------------------------------------------------
def _key(field, wire):
    return _enc_varint((field << 3) | wire)


def _ld(field, payload):
    return _key(field, 2) + _enc_varint(len(payload)) + payload


def _int(field, v):
    return _key(field, 0) + _enc_varint(int(v) & 0xffffffffffffffff)


def encode_scalar_value(tag, value):
    return _ld(1, tag.encode('utf-8')) + _key(2, 5) + struct.pack('<f', float(value))


def encode_image_value(tag, height, width, colorspace, encoded):
    image = _int(1, height) + _int(2, width) + _int(3, colorspace) + _ld(4, bytes(encoded))
    return _ld(1, tag.encode('utf-8')) + _ld(4, image)


def encode_event(wall_time, step=None, values=None, file_version=None):
    ev = _key(1, 1) + struct.pack('<d', float(wall_time))
    if step is not None:
        ev += _int(2, step)
    if file_version is not None:
        ev += _ld(3, file_version)
    if values is not None:
        ev += _ld(5, b''.join(_ld(1, v) for v in values))
    return ev


# -- GIF ---------------------------------------------------------------------------------------------------------------------------------------
def encode_gif(frames, fps):
    """frames uint8 [T, H, W, 1 | 3] -> the bytes of an animated, looping GIF at `fps` (Pillow's encoder, adaptive palette per frame: the
    settings scripts/generate.py writes its files with).  Pillow merges identical neighbouring frames into one of longer duration."""
    from PIL import Image
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    if frames.ndim != 4 or frames.shape[-1] not in (1, 3):
        raise ValueError('encode_gif: uint8 frames [T, H, W, 1 | 3] expected, got %r' % (frames.shape,))
    imgs = [Image.fromarray(f[..., 0], 'L') if f.shape[-1] == 1 else Image.fromarray(f, 'RGB') for f in frames]
    buf = _io.BytesIO()
    imgs[0].save(buf, format='GIF', save_all=True, append_images=imgs[1:], duration=max(1, int(round(1000.0 / max(fps, 1)))), loop=0)
    return buf.getvalue()


# -- the writer -------------------------------------------------------------------------------------------------------------------------------
class EventFileWriter(object):
    """tf.summary.FileWriter: <logdir>/events.out.tfevents.<unix time>.<hostname>, one Event per add_* call."""

    def __init__(self, logdir, filename_suffix=''):
        if not os.path.isdir(logdir):
            os.makedirs(logdir)
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s%s' % (int(time.time()), socket.gethostname(), filename_suffix))
        self._f = open(self.path, 'ab')
        self._record(encode_event(time.time(), file_version=FILE_VERSION))
        self.flush()

    def _record(self, data):
        hdr = struct.pack('<Q', len(data))
        self._f.write(hdr + struct.pack('<I', sio.masked_crc32c(hdr)) + data + struct.pack('<I', sio.masked_crc32c(data)))

    def add_values(self, values, step):
        """One Event carrying already encoded Summary.Value messages."""
        values = list(values)
        if values:
            self._record(encode_event(time.time(), step=step, values=values))

    def add_scalars(self, scalars, step, tag_suffix=None):
        """scalars: {name: number}; tags by summary_tag (+ add_tag_suffix)."""
        self.add_values([encode_scalar_value(_suffixed(summary_tag(k), tag_suffix), v) for k, v in scalars.items()], step)

    def add_gifs(self, boards, step, fps=GIF_FPS, tag_suffix=None):
        """boards: {name: uint8 [T, H, W, 1 | 3] host array}: one animated GIF per tag (gif_summary with a batch of one board)."""
        vals = []
        for k, b in boards.items():
            b = np.asarray(b)
            vals.append(encode_image_value(_suffixed(summary_tag(k, gif=True), tag_suffix), b.shape[1], b.shape[2], b.shape[3],
                                           encode_gif(b, fps)))
        self.add_values(vals, step)

    def flush(self):
        self._f.flush()

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None


def _suffixed(tag, tag_suffix):
    return add_tag_suffix(tag, tag_suffix) if tag_suffix else tag


# -- device -> host ----------------------------------------------------------------------------------------------------------------------------
class BoardTransfer(object):
    """uint8 boards leave the device through one pinned staging buffer (a quarter of the bytes of the float tensors, and an asynchronous
    copy per board with one synchronise for all of them)."""

    def __init__(self):
        self.buf = None

    def to_host(self, boards):
        """{name: uint8 device tensor} -> {name: numpy array}, in order."""
        import torch
        total = sum(int(b.numel()) for b in boards.values())
        if self.buf is None or self.buf.numel() < total:
            self.buf = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
        out, lo = {}, 0
        for k, b in boards.items():
            n = int(b.numel())
            self.buf[lo:lo + n].view(b.shape).copy_(b, non_blocking=True)
            out[k] = (lo, n, tuple(b.shape))
            lo += n
        torch.cuda.synchronize()
        host = self.buf.numpy()
        return type(boards)((k, host[lo:lo + n].reshape(shape).copy()) for k, (lo, n, shape) in out.items())

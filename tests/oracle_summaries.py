"""Test-side restatements for the TensorBoard summaries (video_prediction_amd/summaries.py, csrc/summary.hip) -- numpy only.

* board_index / board_concat: tensor_to_clip (utils/tf_utils.py:175-187) twice, once as the index formula the kernel documents, once as
  the literal unstack / concat sequence of the reference.
* u8: tf.image.convert_image_dtype(float32 -> uint8, saturate=True) in float32: scale by 255.5, clamp to [0, 255], truncate.  UNPINNED:
  restated from memory (TensorFlow is not installed here).
* flow_to_rgb64: tf_utils.flow_to_rgb (:588-603) + tf.image.hsv_to_rgb in float64, per time step and batch group.  UNPINNED likewise; the
  HSV step is cross-checked against matplotlib in the tests.
* read_events: an event file parsed with protobuf message classes built at run time from a FileDescriptorProto that carries the field
  numbers of event.proto / summary.proto which the writer uses.
"""
import numpy as np


def u8(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        v = np.minimum(np.maximum(x * np.float32(255.5), np.float32(0)), np.float32(255))
    return np.where(np.isnan(v), 0, v).astype(np.uint8)


def board_index(src):
    """out[t, m * H + y, b * W + x, c] = u8(src[t, b, y, x, c, m]) for src [T, n, H, W, C(, M)]."""
    src = np.asarray(src)
    if src.ndim == 5:
        src = src[..., None]
    T, n, H, W, C, M = src.shape
    out = np.zeros((T, M * H, n * W, C), np.uint8)
    q = u8(src)
    for t in range(T):
        for m in range(M):
            for b in range(n):
                out[t, m * H:(m + 1) * H, b * W:(b + 1) * W, :] = q[t, b, :, :, :, m]
    return out


def board_concat(src):
    """The reference's own sequence: unstack the last axis of a 6-D tensor and concatenate vertically (axis -3), unstack the batch axis
    and concatenate horizontally (axis 2 of the remaining [n, H', W, C] per ... ), then convert.  The reference passes tensor[:max_outputs]
    BATCH-major ([n, T, H, W, C(, M)]: add_gif_summaries slices the batch first); src here is time-major like the engine's buffers."""
    x = np.asarray(src)
    x = np.swapaxes(x, 0, 1)                                                    # [n, T, H, W, C(, M)]
    if x.ndim == 6:
        x = np.concatenate([x[..., m] for m in range(x.shape[-1])], axis=-3)    # [n, T, M * H, W, C]
    x = np.concatenate([x[b] for b in range(x.shape[0])], axis=2)               # [T, M * H, n * W, C]
    return u8(x)


def hsv_to_rgb64(h, s, v):
    """tf.image.hsv_to_rgb as the kernel restates it: c = s v, m = v - c, dh = 6 h, x = c (1 - |dh mod 2 - 1|), category int(dh)."""
    h, s, v = (np.asarray(a, dtype=np.float64) for a in (h, s, v))
    c = s * v
    m = v - c
    dh = h * 6.0
    x = c * (1.0 - np.abs(np.fmod(dh, 2.0) - 1.0))
    cat = dh.astype(np.int64)
    z = np.zeros_like(c)
    table = [(c, x, z), (x, c, z), (z, c, x), (z, x, c), (x, z, c), (c, z, x)]
    rgb = np.zeros(h.shape + (3,), np.float64)
    for k, (r, g, b) in enumerate(table):
        sel = cat == k
        rgb[sel, 0], rgb[sel, 1], rgb[sel, 2] = r[sel], g[sel], b[sel]
    return rgb + m[..., None]


def flow_to_rgb64(flows, K, groups):
    """flows [T1, N, H, W, >= 2K] (x components, then y) -> float64 [T1, N, H, W, 3, K]; the magnitude range is that of one step of one of
    the `groups` equal batch slices."""
    f = np.asarray(flows, dtype=np.float64)
    T1, N = f.shape[:2]
    x, y = f[..., :K], f[..., K:2 * K]
    mag = np.sqrt(x * x + y * y)
    hue = (np.arctan2(y, x) + np.pi) / (2 * np.pi)
    val = np.empty_like(mag)
    Ng = N // groups
    for t in range(T1):
        for g in range(groups):
            sl = mag[t, g * Ng:(g + 1) * Ng]
            val[t, g * Ng:(g + 1) * Ng] = (sl - sl.min()) / (sl.max() - sl.min())
    rgb = hsv_to_rgb64(hue, np.ones_like(hue), val)           # [T1, N, H, W, K, 3]
    return np.swapaxes(rgb, -1, -2)


_CLASSES = {}


def event_classes():
    """(Event, Summary) message classes from a FileDescriptorProto built here: only the fields the writer uses, with the field numbers
    of tensorflow/core/util/event.proto and framework/summary.proto."""
    if _CLASSES:
        return _CLASSES['Event'], _CLASSES['Summary']
    from google.protobuf import descriptor_pb2, descriptor_pool, message_factory
    F = descriptor_pb2.FieldDescriptorProto
    fd = descriptor_pb2.FileDescriptorProto(name='savp_test_event.proto', package='savp_test', syntax='proto3')

    def msg(name, fields):
        m = fd.message_type.add(name=name)
        for fname, num, ftype, label, tname in fields:
            f = m.field.add(name=fname, number=num, type=ftype, label=label)
            if tname:
                f.type_name = '.savp_test.' + tname
    opt, rep = F.LABEL_OPTIONAL, F.LABEL_REPEATED
    msg('Image', [('height', 1, F.TYPE_INT32, opt, None), ('width', 2, F.TYPE_INT32, opt, None), ('colorspace', 3, F.TYPE_INT32, opt, None),
                  ('encoded_image_string', 4, F.TYPE_BYTES, opt, None)])
    msg('Value', [('tag', 1, F.TYPE_STRING, opt, None), ('simple_value', 2, F.TYPE_FLOAT, opt, None), ('image', 4, F.TYPE_MESSAGE, opt, 'Image')])
    msg('Summary', [('value', 1, F.TYPE_MESSAGE, rep, 'Value')])
    msg('Event', [('wall_time', 1, F.TYPE_DOUBLE, opt, None), ('step', 2, F.TYPE_INT64, opt, None), ('file_version', 3, F.TYPE_STRING, opt, None),
                  ('summary', 5, F.TYPE_MESSAGE, opt, 'Summary')])
    pool = descriptor_pool.DescriptorPool()
    pool.Add(fd)
    for n in ('Event', 'Summary'):
        _CLASSES[n] = message_factory.GetMessageClass(pool.FindMessageTypeByName('savp_test.' + n))
    return _CLASSES['Event'], _CLASSES['Summary']


def read_events(path):
    """[Event] of an event file; oracle.tfrecord.read_records checks both CRCs of every record."""
    from oracle import tfrecord
    Event, _ = event_classes()
    out = []
    for rec in tfrecord.read_records(path):
        ev = Event()
        ev.ParseFromString(rec)
        out.append(ev)
    return out


def decode_gif(data):
    """(frames uint8 [T, H, W, C] as RGB or L, durations in ms) of GIF bytes, through Pillow."""
    import io
    from PIL import Image, ImageSequence
    im = Image.open(io.BytesIO(data))
    frames, durations = [], []
    for fr in ImageSequence.Iterator(im):
        durations.append(fr.info.get('duration'))
        frames.append(np.asarray(fr.convert('RGB')))
    return np.stack(frames), durations

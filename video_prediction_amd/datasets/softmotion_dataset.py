"""SoftmotionVideoDataset (BAIR robot pushing) with the reference's class surface
(video_prediction/datasets/softmotion_dataset.py:11-82, base_dataset.py:12-232,235-353) on libsavp_io.so:
C++ TFRecord reading / Example parsing / sub-sequence sampling / shuffling / batching / prefetch, uint8 over PCIe,
conversion to float32 [0,1] on the GPU.  Frames here are raw uint8 (jpeg_encoding False); the JPEG-encoded datasets build on this class in
jpeg_dataset.py.

object_pos pixel distributions (softmotion_dataset.py:42-43,62-68) are opt-in: SoftmotionVideoDataset(..., pix_distribs=True) or
SAVP_PIX_DISTRIBS=1 in the environment.  With it, and when the first example has '%d/object_pos' (2P floats per frame: (y, x) of P
designated pixels), a batch also carries 'pix_distribs' [B, T, H, W, P], built on the device by savp_pixel_distribution (tf_utils.
pixel_distribution restated: a bilinear one-hot on the flat index y * W + x).  Without the opt-in, or without object_pos in the records,
no such key is emitted.  Together with crop_size / scale_size it raises: the reference would yield maps of the records' size beside
resized images.

crop_size / scale_size (base_dataset.py:63-64,85-86,159-184).  The records are read and cross PCIe at the size they were recorded
(image_shape); when either hyper-parameter is set the conversion kernel also centre-crops or zero-pads every frame to crop x crop
(crop = crop_size or min(H, W); tf.image.resize_image_with_crop_or_pad) and resizes it to scale_size (smaller crop: TF1 bilinear,
align_corners=False, no half-pixel offset; larger crop: TF resize_area), so that batch['images'] is [B, T, S, S, C] with
(S, S, C) = output_image_shape (savp_u8_frames_resize_f32, include/savp_hip.h).  Two deliberate differences from the reference:
  * Range.  The reference's resize ops return float32 in [0, 255] and its convert_image_dtype(float32) then leaves a float input alone,
    so a resized batch would reach the model 255 times too large (no published recipe sets scale_size).  Here a batch is
    resize(image) / 255, in [0, 1] in every case; resizing is linear, so this is the reference's tensor divided by 255.
  * Coordinates.  Source positions and weights are taken from the integers (y * crop) / S and (y * crop) % S, not from TF's float32-rounded
    scale; the two differ by a few 1e-6 of a pixel value at most for non-dyadic ratios, far below the uint8 step, and the result is exact.
The reference reshapes to 3 channels; here any channel count the records carry (KTH may hold 1)."""
import glob
import itertools
import os
import re

import numpy as np
import torch

from .. import io as sio
from ..hparams import HParams


class SoftmotionVideoDataset(object):
    def __init__(self, input_dir, mode='train', num_epochs=None, seed=None, hparams_dict=None, hparams=None, pix_distribs=None):
        self._open(input_dir, mode, num_epochs, seed, hparams_dict, hparams, pix_distribs=pix_distribs)
        # infer the image feature name, frames per example and image shape from the first example (softmotion_dataset.py:15-43,
        # base_dataset.py:264-312)
        first = self._first
        names = self._feature_names(first)
        image_names = set(m.group(1) for m in (re.search(r'\d+/(\w+)/encoded', n) for n in names) if m)
        image_name = next((n for n in ('image_aux1', 'image_view0') if n in image_names), None)
        if not image_name:
            if len(image_names) == 1:
                image_name = image_names.pop()
            else:
                raise ValueError('The examples have images under more than one name.')
        self.image_key_fmt = '%%d/%s/encoded' % image_name
        self._max_sequence_length = self._count_frames(names, image_name)
        _, buf = sio.example_feature(first, self.image_key_fmt % 0)
        side = int(round((len(buf) // 3) ** 0.5))
        if side * side * 3 != len(buf):
            raise ValueError('cannot infer a square RGB image shape from %d bytes' % len(buf))
        self.image_shape = (side, side, 3)
        self.state_like_names_and_shapes = {'images': (self.image_key_fmt, self.image_shape)}
        self.action_like_names_and_shapes = {}
        if self.hparams.use_state:
            self.state_like_names_and_shapes['states'] = ('%d/endeffector_pos', (3,))
            self.action_like_names_and_shapes['actions'] = ('%d/action', (4,))

    @staticmethod
    def _count_frames(names, image_name):
        return 1 + max(int(m.group(1)) for m in (re.match(r'(\d+)/%s/encoded' % image_name, n) for n in names) if m)

    object_pos_fmt = '%d/object_pos'                  # softmotion_dataset.py:43
    pix_distribs = False                              # the opt-in; set by _open (a subclass that opens its files itself has none)

    def _open(self, input_dir, mode, num_epochs, seed, hparams_dict, hparams, pix_distribs=None):
        """base_dataset.py:13-58: input_dir holds train/ val/ test/ sub-directories of *.tfrecord* files (or is one of them).
        pix_distribs: the opt-in of the object_pos pixel distributions (None: SAVP_PIX_DISTRIBS=1 in the environment)."""
        self.pix_distribs = bool(pix_distribs) if pix_distribs is not None else os.environ.get('SAVP_PIX_DISTRIBS', '0') == '1'
        self.input_dir = os.path.normpath(os.path.expanduser(input_dir))
        self.mode = mode
        self.num_epochs = num_epochs
        self.seed = seed
        if self.mode not in ('train', 'val', 'test'):
            raise ValueError('Invalid mode %s' % self.mode)
        if not os.path.exists(self.input_dir):
            raise FileNotFoundError('input_dir %s does not exist' % self.input_dir)
        self.filenames = None
        # look for tfrecords in input_dir and input_dir/mode directories (base_dataset.py:36-43)
        for d in (self.input_dir, os.path.join(self.input_dir, self.mode)):
            filenames = glob.glob(os.path.join(d, '*.tfrecord*'))
            if filenames:
                self.input_dir = d
                self.filenames = sorted(filenames)
                break
        if not self.filenames:
            raise FileNotFoundError('No tfrecords were found in %s.' % self.input_dir)
        self.dataset_name = os.path.basename(os.path.split(self.input_dir)[0])
        self.hparams = self.parse_hparams(hparams_dict, hparams)
        self._first = sio.read_records(self.filenames[0])[0]

    @property
    def crop_and_scale(self):
        """(crop, S) of base_dataset.py:166-183 when crop_size or scale_size is set, else None (frames are delivered as recorded)."""
        hp = self.hparams
        if not (hp.crop_size or hp.scale_size):
            return None
        crop = hp.crop_size or min(self.image_shape[:2])
        return crop, (hp.scale_size or crop)

    @property
    def num_designated_pixels(self):
        """P of batch['pix_distribs']: half the width of the first example's object_pos feature; 0 without the opt-in or without the
        feature (softmotion_dataset.py:42-43: the shape is inferred from the first example)."""
        if not self.pix_distribs or (self.object_pos_fmt % 0) not in self._feature_names(self._first):
            return 0
        kind, vals = sio.example_feature(self._first, self.object_pos_fmt % 0)
        if kind != 2 or not vals or len(vals) % 2:
            raise ValueError('%s: expected (y, x) float pairs, got %r' % (self.object_pos_fmt % 0, vals))
        if self.crop_and_scale is not None or getattr(self, 'random_crop', 0):
            raise NotImplementedError('object_pos pixel distributions with crop_size / scale_size (or a random crop): the maps would keep '
                                      'the size of the records beside resized images')
        return len(vals) // 2

    def _float_keys(self):
        """[(key format, width, 0 = one per frame | 1 = one per transition)] of the pipeline: states, actions, then object_pos."""
        float_keys = []
        if self.hparams.use_state:
            (s_fmt, s_shape), (a_fmt, a_shape) = self.state_like_names_and_shapes['states'], self.action_like_names_and_shapes['actions']
            float_keys = [(s_fmt, s_shape[0], 0), (a_fmt, a_shape[0], 1)]
        P = self.num_designated_pixels
        if P:
            float_keys.append((self.object_pos_fmt, 2 * P, 0))
        return float_keys

    def _float_outputs(self, floats, out, K, device):
        """The float features of one batch into the inputs dict: states / actions as read, object_pos as pix_distribs [B, T, H, W, P]."""
        floats = list(floats or [])
        if self.hparams.use_state:
            out['states'] = torch.from_numpy(floats.pop(0)).to(device)
            out['actions'] = torch.from_numpy(floats.pop(0)).to(device)
        if floats:
            H, W = self.output_image_shape[:2]
            out['pix_distribs'] = K.pixel_distribution(torch.from_numpy(floats.pop(0)).to(device), H, W)
        return out

    @property
    def output_image_shape(self):
        """Frame shape of batch['images'] -- what the model is sized from; image_shape stays the shape of the records."""
        cs = self.crop_and_scale
        return tuple(self.image_shape) if cs is None else (cs[1], cs[1], self.image_shape[2])

    @staticmethod
    def _feature_names(example):
        """Feature keys of a serialized tf.train.Example (minimal wire-format walk)."""
        def varint(b, i):
            v = s = 0
            while True:
                c = b[i]; i += 1
                v |= (c & 0x7f) << s; s += 7
                if not c & 0x80:
                    return v, i
        names, i = [], 0
        _, i = varint(example, i)
        n, i = varint(example, i)
        feats, j = example[i:i + n], 0
        while j < len(feats):
            _, j = varint(feats, j)
            m, j = varint(feats, j)
            entry, j = feats[j:j + m], j + m
            _, k = varint(entry, 0)
            ln, k = varint(entry, k)
            names.append(entry[k:k + ln].decode())
        return names

    def get_default_hparams_dict(self):
        """base_dataset.py:60-101 + softmotion_dataset.py:45-53."""
        base = dict(crop_size=0, scale_size=0, context_frames=1, sequence_length=0, long_sequence_length=0, frame_skip=0,
                    time_shift=1, force_time_shift=False, shuffle_on_val=False, use_state=False)
        over = dict(context_frames=2, sequence_length=12, long_sequence_length=30, time_shift=2)
        return dict(itertools.chain(base.items(), over.items()))

    def get_default_hparams(self):
        return HParams(**self.get_default_hparams_dict())

    def parse_hparams(self, hparams_dict, hparams):
        parsed = self.get_default_hparams().override_from_dict(hparams_dict or {})
        if hparams:
            if not isinstance(hparams, (list, tuple)):
                hparams = [hparams]
            for h in hparams:
                parsed.parse(h)
        if parsed.long_sequence_length == 0:
            parsed.long_sequence_length = parsed.sequence_length
        return parsed

    @property
    def jpeg_encoding(self):
        return False

    def num_examples_per_epoch(self):
        """softmotion_dataset.py:70-82: trajectory ranges are encoded in the file names."""
        count = 0
        for filename in self.filenames:
            match = re.search(r'traj_(\d+)_to_(\d+).tfrecords', os.path.basename(filename))
            if not match:
                return sum(len(sio.read_records(f)) for f in self.filenames)
            count += int(match.group(2)) - int(match.group(1)) + 1
        return count

    def _shard(self, rank, world):
        """Files (and the seed) of one data-parallel replica: every replica reads its own share of the record files -- the
        reference feeds all towers from ONE iterator and tf.split()s the batch (base_model.py:523-527), so distinct towers see
        distinct sequences; with one process per GPU that becomes distinct files per rank (round-robin; with fewer files than
        ranks every rank reads everything in its own shuffled order)."""
        files = self.filenames[rank::world] if len(self.filenames) >= world else self.filenames
        seed = ((self.seed or 0) * 1000003 + rank * 7919) & 0xffffffffffffffff
        if self.seed is None and world == 1:
            seed = 0
        return files, seed

    def make_pipeline(self, batch_size, prefetch_batches=2, rank=0, world=1):
        hp = self.hparams
        shuffle = self.mode == 'train' or (self.mode == 'val' and hp.shuffle_on_val)        # base_dataset.py:131
        time_shift = hp.time_shift if ((hp.time_shift and self.mode == 'train') or hp.force_time_shift) else 0   # :198
        float_keys = self._float_keys()
        files, seed = self._shard(rank, world)
        return sio.VideoPipeline(files, self.image_key_fmt, self._max_sequence_length, self.image_shape,
                                 hp.sequence_length, batch_size, frame_skip=hp.frame_skip, time_shift=time_shift, shuffle=shuffle,
                                 num_epochs=self.num_epochs, seed=seed, prefetch_batches=prefetch_batches,
                                 float_keys=float_keys, var_len=self.var_len)

    var_len = False          # one feature per frame (softmotion); KTHVideoDataset: one bytes_list per sequence

    def make_batch(self, batch_size, device='cuda:0', rank=0, world=1):
        """base_dataset.py:153-156: an iterator of input dicts {'images': float32 [B,T,H,W,C] in [0,1] on the device, ('states',
        'actions', 'pix_distribs')}.  Frames cross PCIe as uint8 from pinned memory; conversion + layout change happen in one HIP kernel.
        rank / world: the data-parallel replica this iterator feeds (see _shard)."""
        return _BatchIterator(self, batch_size, device, rank, world)

    def set_sequence_length(self, sequence_length):
        """base_dataset.py:103-104."""
        self.hparams.sequence_length = sequence_length


class _BatchIterator(object):
    def __init__(self, ds, batch_size, device, rank=0, world=1):
        from .. import kernels as K
        self.K = K
        self.ds, self.device = ds, torch.device(device)
        self.pipe = ds.make_pipeline(batch_size, rank=rank, world=world)
        B, T = batch_size, ds.hparams.sequence_length
        self.host = torch.empty((B, T) + ds.image_shape, dtype=torch.uint8).pin_memory()
        self.dev_u8 = torch.empty((B, T) + ds.image_shape, dtype=torch.uint8, device=self.device)
        self.copied = None           # event recorded behind the H2D copy out of the pinned buffer

    def __iter__(self):
        return self

    def __next__(self):
        if self.copied is not None:
            self.copied.synchronize()     # the previous batch has left the pinned buffer before the reader refills it
        got = self.pipe.next(self.host.numpy())
        if got is None:
            raise StopIteration
        _, floats = got
        self.dev_u8.copy_(self.host, non_blocking=True)
        if self.device.type == 'cuda':
            self.copied = torch.cuda.Event()
            self.copied.record(torch.cuda.current_stream(self.device))
        B, T = self.dev_u8.shape[:2]
        images_tm = torch.empty((T, B) + self.ds.output_image_shape, device=self.device)
        cs = self.ds.crop_and_scale
        if cs is None:
            self.K.u8_frames_to_f32(self.dev_u8, images_tm)
        else:
            self.K.u8_frames_resize_f32(self.dev_u8, images_tm, cs[0])
        out = {'images': images_tm.transpose(0, 1)}                      # batch-major view, like the reference's iterator
        return self.ds._float_outputs(floats, out, self.K, self.device)

    next = __next__

"""Datasets whose frames are JPEG streams (jpeg_encoding True: base_dataset.py:161-162): the base of GoogleRobotVideoDataset,
SV2PVideoDataset and UCF101VideoDataset.

tf.image.decode_jpeg is split in two.  The serial Huffman bitstream of the frames that survive sub-sequence sampling is decoded on
worker threads of the C++ pipeline (libsavp_io.so: savp_pipeline_next_jpeg) into int16 coefficients; those cross PCIe from pinned memory and
one HIP launch sequence (savp_jpeg_decode_u8, csrc/jpeg_decode.hip) dequantises, runs libjpeg's integer IDCT, upsamples the chroma and
converts to RGB: uint8 [B, T, H, W, C], sample for sample what libjpeg-turbo (and so TensorFlow) decodes.  From there on the path is the
one of the raw datasets: savp_u8_frames_to_f32, or savp_u8_frames_resize_f32 when crop_size / scale_size is set (softmotion_dataset.py).

Worker threads: 4 unless SAVP_DECODE_THREADS says otherwise (at most 16); the count is never taken from the machine's core count."""
import os
import re

import numpy as np
import torch

from .. import io as sio
from .softmotion_dataset import SoftmotionVideoDataset


class JpegVideoDataset(SoftmotionVideoDataset):
    random_crop = 0            # UCF101: side of the window drawn per sequence (0: none)

    def _init_jpeg(self, image_key_fmt, image_shape):
        """The shared tail of the three constructors: frames per example and the declared shape against the first frame's header."""
        self.image_key_fmt = image_key_fmt
        self.image_shape = tuple(image_shape)
        if self.var_len:
            self._max_sequence_length = 0                                    # per example ('sequence_length' feature)
        else:
            pat = re.compile('^' + re.escape(image_key_fmt).replace(re.escape('%d'), r'(\d+)') + '$')
            frames = [int(m.group(1)) for m in (pat.match(n) for n in self._feature_names(self._first)) if m]
            if not frames:
                raise ValueError('no feature named like %s in the first example of %s' % (image_key_fmt, self.filenames[0]))
            self._max_sequence_length = 1 + max(frames)
        _, buf = sio.example_feature(self._first, image_key_fmt if self.var_len else image_key_fmt % 0)
        try:
            info = sio.jpeg_info(buf)
        except sio.JpegError as e:
            raise ValueError('%s: %s' % (self.filenames[0], e))
        if (info.height, info.width, info.components) != self.image_shape:
            raise ValueError('%s holds JPEG frames of %d x %d with %d component(s), the dataset declares %r'
                             % (self.filenames[0], info.height, info.width, info.components, self.image_shape))
        self.state_like_names_and_shapes = {'images': (image_key_fmt, self.image_shape)}
        self.action_like_names_and_shapes = {}

    @property
    def jpeg_encoding(self):
        return True

    @property
    def decode_threads(self):
        return int(os.environ.get('SAVP_DECODE_THREADS', '0') or 0)

    def make_pipeline(self, batch_size, prefetch_batches=2, rank=0, world=1):
        hp = self.hparams
        shuffle = self.mode == 'train' or (self.mode == 'val' and hp.shuffle_on_val)        # base_dataset.py:131
        time_shift = hp.time_shift if ((hp.time_shift and self.mode == 'train') or hp.force_time_shift) else 0   # :198
        float_keys = self._float_keys()
        files, seed = self._shard(rank, world)
        return sio.VideoPipeline(files, self.image_key_fmt, self._max_sequence_length, self.image_shape,
                                 hp.sequence_length, batch_size, frame_skip=hp.frame_skip, time_shift=time_shift, shuffle=shuffle,
                                 num_epochs=self.num_epochs, seed=seed, prefetch_batches=prefetch_batches,
                                 float_keys=float_keys, var_len=self.var_len, jpeg=True, decode_threads=self.decode_threads,
                                 random_crop=self.random_crop)

    def make_batch(self, batch_size, device='cuda:0', rank=0, world=1):
        """As SoftmotionVideoDataset.make_batch: {'images': float32 [B,T,H,W,C] in [0,1] on the device, ('states', 'actions')}."""
        return _JpegBatchIterator(self, batch_size, device, rank, world)


class _JpegBatchIterator(object):
    def __init__(self, ds, batch_size, device, rank=0, world=1):
        from .. import kernels as K
        self.K = K
        self.ds, self.device = ds, torch.device(device)
        self.pipe = ds.make_pipeline(batch_size, rank=rank, world=world)
        self.info = info = self.pipe.jpeg_info
        B, T = batch_size, ds.hparams.sequence_length
        H, W, C = ds.image_shape
        crop = ds.random_crop
        self.decoded_shape = (crop, crop, C) if crop else (H, W, C)
        # pinned staging: int16 coefficients, the tables as int16 bits (uint16 on the C side), one window per frame
        self.host_coef = torch.empty((B, T, info.total_blocks, 64), dtype=torch.int16).pin_memory()
        self.host_qtab = torch.empty((B, T, C, 64), dtype=torch.int16).pin_memory()
        self.dev_coef = torch.empty_like(self.host_coef, device=self.device)
        self.dev_qtab = torch.empty_like(self.host_qtab, device=self.device)
        self.dev_u8 = torch.empty((B, T) + self.decoded_shape, dtype=torch.uint8, device=self.device)
        self.ws = torch.empty(K.jpeg_workspace_bytes(info, B * T), dtype=torch.uint8, device=self.device)
        self.seq_windows = np.zeros((B, 2), np.int32)
        self.host_win = torch.zeros((B, T, 2), dtype=torch.int32).pin_memory() if crop else None
        self.dev_win = torch.zeros((B, T, 2), dtype=torch.int32, device=self.device) if crop else None
        self.copied = None           # event recorded behind the H2D copies out of the pinned buffers

    def __iter__(self):
        return self

    def __next__(self):
        if self.copied is not None:
            self.copied.synchronize()     # the previous batch has left the pinned buffers before the workers' results overwrite them
        got = self.pipe.next_jpeg(self.host_coef.numpy(), self.host_qtab.numpy().view(np.uint16), self.seq_windows)
        if got is None:
            raise StopIteration
        floats = got[3]
        self.dev_coef.copy_(self.host_coef, non_blocking=True)
        self.dev_qtab.copy_(self.host_qtab, non_blocking=True)
        if self.dev_win is not None:
            self.host_win.numpy()[:] = self.seq_windows[:, None, :]          # one window per sequence, the same for all its frames
            self.dev_win.copy_(self.host_win, non_blocking=True)
        if self.device.type == 'cuda':
            self.copied = torch.cuda.Event()
            self.copied.record(torch.cuda.current_stream(self.device))
        self.K.jpeg_decode_u8(self.dev_coef, self.dev_qtab, self.info, self.dev_u8, self.ws, window=self.dev_win)
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

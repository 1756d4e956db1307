"""UCF101VideoDataset with the reference's class surface (video_prediction/datasets/ucf101_dataset.py:15-69 on base_dataset.py:394-453
VarLenFeatureVideoDataset) on libsavp_io.so and the HIP JPEG kernels (jpeg_dataset.py).

Record layout: ONE tf.train.Example per sequence with the int64 feature 'sequence_length' and a bytes_list 'images/encoded' holding one
JPEG stream of 240 x 320 x 3 per frame (:18).  Shorter sequences are dropped, the sub-sequence is sampled per example (kth_dataset.py in
this package).  random_crop_size (:43-48): one window per sequence, y0 in [0, H - crop), x0 in [0, W - crop) with the upper bound
excluded like tf.random_uniform, drawn from the pipeline's seed, in every mode (the reference's TODO at :55); the kernel decodes the
window only (decode_and_crop_jpeg).  crop_size / scale_size raise NotImplementedError as in the reference (:35-38).  Its record-writing
main() is not restated."""
import itertools
import os
import re

from .. import io as sio
from .jpeg_dataset import JpegVideoDataset


class UCF101VideoDataset(JpegVideoDataset):
    var_len = True

    def __init__(self, input_dir, mode='train', num_epochs=None, seed=None, hparams_dict=None, hparams=None):
        self._open(input_dir, mode, num_epochs, seed, hparams_dict, hparams)
        if self.hparams.crop_size or self.hparams.scale_size:
            raise NotImplementedError('UCF101VideoDataset: crop_size / scale_size are not implemented (use random_crop_size)')
        if self.hparams.use_state:
            raise NotImplementedError('UCF101 records carry no states / actions')
        self._init_jpeg('images/encoded', (240, 320, 3))
        if self.random_crop < 0 or self.random_crop > min(self.image_shape[:2]):
            raise ValueError('random_crop_size %d does not fit frames of %d x %d' % ((self.random_crop,) + self.image_shape[:2]))

    def get_default_hparams_dict(self):
        """base_dataset.py:60-101 + ucf101_dataset.py:20-28."""
        base = dict(crop_size=0, scale_size=0, context_frames=1, sequence_length=0, long_sequence_length=0, frame_skip=0,
                    time_shift=1, force_time_shift=False, shuffle_on_val=False, use_state=False)
        over = dict(context_frames=4, sequence_length=8, random_crop_size=0, use_state=False)
        return dict(itertools.chain(base.items(), over.items()))

    @property
    def random_crop(self):
        return int(self.hparams.random_crop_size)

    @property
    def output_image_shape(self):
        crop = self.random_crop
        return (crop, crop, self.image_shape[2]) if crop else tuple(self.image_shape)

    def num_examples_per_epoch(self):
        """ucf101_dataset.py:58-69: sequence ranges are encoded in the file names (files named otherwise are counted record by record)."""
        count = 0
        for filename in self.filenames:
            match = re.search(r'sequence_(\d+)_to_(\d+).tfrecords', os.path.basename(filename))
            if not match:
                return sum(len(sio.read_records(f)) for f in self.filenames)
            count += int(match.group(2)) - int(match.group(1)) + 1
        return count

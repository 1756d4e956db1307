"""SV2PVideoDataset with the reference's class surface (video_prediction/datasets/sv2p_dataset.py:7-65 on base_dataset.py) on
libsavp_io.so and the HIP JPEG kernels (jpeg_dataset.py).

Record layout: one feature per frame, JPEG streams of 64 x 64 x 3 under 'image_%d' (:11).  Two variants, told apart by the name of the
directory above train/ val/ test/ (:10): 'shape' (2-d 'state_%d' / 'action_%d' with use_state) and 'humans' (no states: use_state raises)."""
import itertools
import os

from .jpeg_dataset import JpegVideoDataset


class SV2PVideoDataset(JpegVideoDataset):
    COUNTS = {'shape': {'train': 43415, 'val': 2898}, 'humans': {'train': 23910, 'val': 10472, 'test': 7722}}

    def __init__(self, input_dir, mode='train', num_epochs=None, seed=None, hparams_dict=None, hparams=None):
        self._open(input_dir, mode, num_epochs, seed, hparams_dict, hparams)      # sets dataset_name before it parses the hparams
        self._init_jpeg('image_%d', (64, 64, 3))
        if self.dataset_name == 'shape':
            if self.hparams.use_state:
                self.state_like_names_and_shapes['states'] = ('state_%d', (2,))
                self.action_like_names_and_shapes['actions'] = ('action_%d', (2,))
        elif self.dataset_name == 'humans':
            if self.hparams.use_state:
                raise ValueError('SV2PVideoDataset does not have states, use_state should be False')
        else:
            raise NotImplementedError

    def get_default_hparams_dict(self):
        """base_dataset.py:60-101 + sv2p_dataset.py:23-40."""
        base = dict(crop_size=0, scale_size=0, context_frames=1, sequence_length=0, long_sequence_length=0, frame_skip=0,
                    time_shift=1, force_time_shift=False, shuffle_on_val=False, use_state=False)
        if self.dataset_name == 'shape':
            over = dict(context_frames=1, sequence_length=6, time_shift=0, use_state=False)
        elif self.dataset_name == 'humans':
            over = dict(context_frames=10, sequence_length=20, use_state=False)
        else:
            raise NotImplementedError
        return dict(itertools.chain(base.items(), over.items()))

    def num_examples_per_epoch(self):
        """sv2p_dataset.py:42-61: by variant and directory name (the shape dataset has no test set)."""
        try:
            return self.COUNTS[self.dataset_name][os.path.basename(self.input_dir)]
        except KeyError:
            raise NotImplementedError

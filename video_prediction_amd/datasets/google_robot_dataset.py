"""GoogleRobotVideoDataset (the Google robot push dataset) with the reference's class surface
(video_prediction/datasets/google_robot_dataset.py:7-40 on base_dataset.py) on libsavp_io.so and the HIP JPEG kernels (jpeg_dataset.py).

Record layout: one feature per frame, JPEG streams of 512 x 640 x 3 under 'move/%d/image/encoded' (:13), 5-d states under
'move/%d/endeffector/vec_pitch_yaw' and 5-d actions under 'move/%d/commanded_pose/vec_pitch_yaw' (:15-16, with use_state).  The published
use is crop_size=512 (centre crop), scale_size=64 (area resize): both run on the device after decoding (softmotion_dataset.py)."""
import itertools
import os

from .jpeg_dataset import JpegVideoDataset


class GoogleRobotVideoDataset(JpegVideoDataset):
    def __init__(self, input_dir, mode='train', num_epochs=None, seed=None, hparams_dict=None, hparams=None):
        self._open(input_dir, mode, num_epochs, seed, hparams_dict, hparams)
        self._init_jpeg('move/%d/image/encoded', (512, 640, 3))
        if self.hparams.use_state:
            self.state_like_names_and_shapes['states'] = ('move/%d/endeffector/vec_pitch_yaw', (5,))
            self.action_like_names_and_shapes['actions'] = ('move/%d/commanded_pose/vec_pitch_yaw', (5,))

    def get_default_hparams_dict(self):
        """base_dataset.py:60-101 + google_robot_dataset.py:19-25."""
        base = dict(crop_size=0, scale_size=0, context_frames=1, sequence_length=0, long_sequence_length=0, frame_skip=0,
                    time_shift=1, force_time_shift=False, shuffle_on_val=False, use_state=False)
        over = dict(context_frames=2, sequence_length=15)
        return dict(itertools.chain(base.items(), over.items()))

    def num_examples_per_epoch(self):
        """google_robot_dataset.py:27-36: by directory name."""
        counts = {'push_train': 51615, 'push_testseen': 1038, 'push_testnovel': 995}
        name = os.path.basename(self.input_dir)
        if name not in counts:
            raise NotImplementedError
        return counts[name]

"""CartgripperVideoDataset with the reference's class surface (video_prediction/datasets/cartgripper_dataset.py:7-24 on
softmotion_dataset.py / base_dataset.py) on libsavp_io.so.

Record layout: one feature per frame like softmotion; raw uint8 frames of 48 x 64 x 3 under '%d/image_view0/encoded'
(cartgripper_dataset.py:10), 6-d states under '%d/endeffector_pos' and 3-d actions under '%d/action' (:11-13, use_state defaults to True).
The frames are not square: without crop_size / scale_size they are delivered as recorded, [B, T, 48, 64, 3]; scale_size=64 (crop_size 0)
centre-crops them to 48 x 48 and enlarges that to 64 x 64 on the device (softmotion_dataset.py in this package)."""
import itertools

from .. import io as sio
from .softmotion_dataset import SoftmotionVideoDataset


class CartgripperVideoDataset(SoftmotionVideoDataset):
    def __init__(self, input_dir, mode='train', num_epochs=None, seed=None, hparams_dict=None, hparams=None, pix_distribs=None):
        self._open(input_dir, mode, num_epochs, seed, hparams_dict, hparams, pix_distribs=pix_distribs)
        self.image_key_fmt = '%d/image_view0/encoded'                                 # cartgripper_dataset.py:10
        self.image_shape = (48, 64, 3)
        _, buf = sio.example_feature(self._first, self.image_key_fmt % 0)
        if len(buf) != 48 * 64 * 3:                                                   # _check_or_infer_shapes (base_dataset.py:264-312)
            raise ValueError('cartgripper frames are 48 x 64 x 3 bytes, the records hold %d' % len(buf))
        self._max_sequence_length = self._count_frames(self._feature_names(self._first), 'image_view0')
        self.state_like_names_and_shapes = {'images': (self.image_key_fmt, self.image_shape)}
        self.action_like_names_and_shapes = {}
        if self.hparams.use_state:                                                    # :11-13
            self.state_like_names_and_shapes['states'] = ('%d/endeffector_pos', (6,))
            self.action_like_names_and_shapes['actions'] = ('%d/action', (3,))

    def get_default_hparams_dict(self):
        """softmotion's defaults + cartgripper_dataset.py:16-24."""
        base = super(CartgripperVideoDataset, self).get_default_hparams_dict()
        over = dict(context_frames=2, sequence_length=15, time_shift=3, use_state=True)
        return dict(itertools.chain(base.items(), over.items()))

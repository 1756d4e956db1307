"""Datasets with the reference's class API (video_prediction/datasets/__init__.py:9-24) on the C++ input pipeline."""
from .softmotion_dataset import SoftmotionVideoDataset
from .kth_dataset import KTHVideoDataset
from .cartgripper_dataset import CartgripperVideoDataset
from .google_robot_dataset import GoogleRobotVideoDataset
from .sv2p_dataset import SV2PVideoDataset
from .ucf101_dataset import UCF101VideoDataset


def get_dataset_class(dataset):
    dataset_mappings = {
        'bair': 'SoftmotionVideoDataset',
        'softmotion': 'SoftmotionVideoDataset',
        'softmotion30_v1': 'SoftmotionVideoDataset',
        'kth': 'KTHVideoDataset',
        'cartgripper': 'CartgripperVideoDataset',
        'google_robot': 'GoogleRobotVideoDataset',
        'sv2p': 'SV2PVideoDataset',
        'ucf101': 'UCF101VideoDataset',
    }
    dataset_class = dataset_mappings.get(dataset, dataset)
    dataset_class = globals().get(dataset_class)
    if dataset_class is None:
        raise ValueError('Invalid dataset %s' % dataset)
    return dataset_class

"""Host-side rules of scripts/train.py's long-sequence evaluation (no GPU): which datasets have a long version, the long model's batch and the
number of updates of one accumulated evaluation."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts import train as TR                                  # noqa: E402
from video_prediction_amd.datasets import get_dataset_class     # noqa: E402


class _Parsed(object):
    """A dataset reduced to what long_eval_length reads: the hparams its class parses from its defaults and the given overrides."""

    def __init__(self, cls, hparams_dict=None, hparams=None):
        self.hparams = cls.parse_hparams(cls.__new__(cls), hparams_dict, hparams)


@pytest.mark.parametrize('name,short,long_', [('softmotion', 12, 30), ('kth', 20, 40)])
def test_the_reference_recipes_have_a_long_version(name, short, long_):
    ds = _Parsed(get_dataset_class(name))
    assert (ds.hparams.sequence_length, ds.hparams.long_sequence_length) == (short, long_)
    assert TR.long_eval_length(ds, False) == long_ == TR.long_eval_length(ds, True)


@pytest.mark.parametrize('name', ['softmotion', 'kth'])
def test_equal_lengths_have_none(name):
    cls = get_dataset_class(name)
    default = _Parsed(cls).hparams.sequence_length
    assert TR.long_eval_length(_Parsed(cls, {'long_sequence_length': default}), True) is None
    assert TR.long_eval_length(_Parsed(cls, hparams='sequence_length=9,long_sequence_length=9'), True) is None
    # long_sequence_length = 0 means "the sequence length" (base_dataset.py:97-98)
    assert TR.long_eval_length(_Parsed(cls, hparams='sequence_length=9,long_sequence_length=0'), True) is None
    assert TR.long_eval_length(_Parsed(cls, hparams='sequence_length=9,long_sequence_length=15'), True) == 15


def test_synthetic_has_a_long_version_only_when_asked_for():
    """Its constant long_sequence_length=12 has nothing to do with the sequence_length asked for."""
    ds = TR.SyntheticVideoDataset('none', hparams='sequence_length=4')
    assert ds.hparams.long_sequence_length == 12 and not TR.long_length_given({}, 'sequence_length=4')
    assert TR.long_eval_length(ds, False) is None
    given = 'sequence_length=4,long_sequence_length=6'
    assert TR.long_length_given({}, given) and TR.long_length_given(None, ['time_shift=1', given])
    assert TR.long_eval_length(TR.SyntheticVideoDataset('none', hparams=given), True) == 6
    assert TR.long_length_given({'long_sequence_length': 6}, None)
    assert TR.long_eval_length(TR.SyntheticVideoDataset('none', hparams_dict={'sequence_length': 4, 'long_sequence_length': 6}), True) == 6
    assert TR.long_eval_length(TR.SyntheticVideoDataset('none', hparams='sequence_length=6,long_sequence_length=6'), True) is None
    assert not TR.long_length_given({'sequence_length': 4}, 'sequence_length=4,frame_skip=0') and not TR.long_length_given(None, None)


def test_set_sequence_length_gives_the_long_dataset_its_frames():
    ds = TR.SyntheticVideoDataset('none', mode='val', hparams='sequence_length=4,long_sequence_length=6', shape=(8, 8, 3))
    ds.set_sequence_length(TR.long_eval_length(ds, True))
    batch = next(iter(ds.make_batch(1, device='cpu')))
    assert tuple(batch['images'].shape) == (1, 6, 8, 8, 3)


@pytest.mark.parametrize('per_gpu,want', [(1, 1), (2, 1), (3, 1), (8, 4), (16, 8)])
def test_long_batch_is_half_the_per_gpu_batch_at_least_one(per_gpu, want):
    assert TR.long_eval_batch(per_gpu) == want


def test_update_count_walks_the_validation_set_once():
    class DS(object):
        def __init__(self, n):
            self.n = n

        def num_examples_per_epoch(self):
            return self.n
    assert TR.accum_eval_updates(DS(8), 2, 1) == 4 and TR.accum_eval_updates(DS(8), TR.long_eval_batch(2), 1) == 8
    assert TR.accum_eval_updates(DS(256), 8, 2) == 16 and TR.accum_eval_updates(DS(256), TR.long_eval_batch(8), 2) == 32
    assert TR.accum_eval_updates(DS(7), 2, 2) == 1 and TR.accum_eval_updates(DS(3), 2, 2) == 0


def test_records_too_short_for_the_long_version_have_none():
    """Fixed-length records: (long - 1) * (frame_skip + 1) + 1 frames are needed; per-example lengths (KTH) are filtered by the reader."""
    cls = get_dataset_class('softmotion')
    ds = _Parsed(cls, hparams='sequence_length=6')
    assert ds.hparams.long_sequence_length == 30
    for frames, want in ((8, None), (29, None), (30, 30), (40, 30)):
        ds._max_sequence_length = frames
        assert TR.long_eval_length(ds, False) == want, frames
    skip = _Parsed(cls, hparams='sequence_length=6,long_sequence_length=10,frame_skip=1')
    for frames, want in ((18, None), (19, 10)):
        skip._max_sequence_length = frames
        assert TR.long_eval_length(skip, True) == want, frames
    kth = _Parsed(get_dataset_class('kth'))
    kth._max_sequence_length = 0
    assert TR.long_eval_length(kth, False) == 40

"""Host side of the training guard (no GPU): the work-list of savp_arena_health built from an arena's slot table, the chunk and workspace
queries against the library's, and the model class's handling of guard= outside training."""
import random
from collections import OrderedDict

import numpy as np
import pytest


def _offsets(shapes):
    """Arena.offsets without a device: name -> (offset, n, shape), slots aligned to 4 floats (video_prediction_amd/engine.py)."""
    from video_prediction_amd.engine import _align4
    out, off = OrderedDict(), 0
    for i, shape in enumerate(shapes):
        n = int(np.prod(shape)) if len(shape) else 1
        out['v%d' % i] = (off, n, tuple(shape))
        off += _align4(n)
    return out, off


def _check_worklist(segs, items, chunk, size):
    """The items tile every segment exactly once, in order, none longer than the chunk, none over padding or past the arena."""
    covered = np.zeros(size, dtype=np.int32)
    at = 0
    for s, (off, n) in enumerate(segs):
        pos = 0
        while pos < n:
            assert at < len(items), 'list ends inside segment %d' % s
            seg, start, count = items[at]
            assert seg == s and start == pos, (items[at], s, pos)          # segment order, and start order inside a segment
            assert 1 <= count <= chunk and start % 4 == 0
            assert start + count <= n                                       # stays inside the variable: never the padding behind it
            covered[off + start:off + start + count] += 1
            pos += count
            at += 1
    assert at == len(items)                                                 # nothing listed beyond the segments
    want = np.zeros(size, dtype=np.int32)
    for off, n in segs:
        want[off:off + n] = 1
    assert np.array_equal(covered, want)                                    # every element once, every padding float never


def test_worklist_tiles_every_segment_once_in_order_and_never_touches_padding():
    from video_prediction_amd import kernels as K
    C = K.arena_health_chunk()
    rng = random.Random(5)
    cases = [[(1,), (3,), (4,), (5,), (C - 1,), (C,), (C + 1,), (2 * C + 7,), (3, 5, 7)], [()], [(C,)], [(4 * C,)]]
    for _ in range(20):
        cases.append([tuple(rng.choice((1, 2, 3, 5, 7, 64, 129)) for _ in range(rng.randint(0, 3))) for _ in range(rng.randint(1, 12))] +
                     [(rng.randint(1, 3 * C),)])
    for shapes in cases:
        offsets, size = _offsets(shapes)
        segs = [(off, n) for off, n, _ in offsets.values()]
        for chunk in (C, 8, 4):
            _check_worklist(segs, K.arena_health_worklist(segs, chunk), chunk, size)
    # the documented split of 2 C + 7 floats: three items, the last one short
    assert K.arena_health_worklist([(0, 2 * C + 7)]) == [(0, 0, C), (0, C, C), (0, 2 * C, 7)]
    assert K.arena_health_worklist([]) == []


def test_chunk_and_workspace_queries_match_the_library(hip_lib):
    from video_prediction_amd import kernels as K
    C = K.arena_health_chunk()
    assert C == hip_lib.savp_arena_health_chunk() and C % 4 == 0 and C >= 4
    for n in (-1, 0, 1, 7, 1 << 20):
        assert K.arena_health_ws_bytes(n) == hip_lib.savp_arena_health_ws_bytes(n)
    assert K.arena_health_ws_bytes(0) == 0 and K.arena_health_ws_bytes(3) % 16 == 0


def test_guard_switch_is_read_in_python_and_ignored_outside_training(monkeypatch):
    """guard=None reads SAVP_GUARD ('1' = on); an explicit flag wins; a mode='test' model ignores the switch (pinned: ignored, not
    refused -- scripts build a test-mode model beside the training one under the same environment)."""
    from video_prediction_amd.models import get_model_class
    from video_prediction_amd.models.savp_model import guard_enabled
    M = get_model_class('savp')
    hp = dict(context_frames=2, sequence_length=5)
    monkeypatch.delenv('SAVP_GUARD', raising=False)
    assert M(mode='train', hparams_dict=hp).guard is False
    assert M(mode='train', hparams_dict=hp, guard=True).guard is True
    assert M(mode='test', hparams_dict=hp, guard=True).guard is False
    monkeypatch.setenv('SAVP_GUARD', '1')
    assert M(mode='train', hparams_dict=hp).guard is True
    assert M(mode='train', hparams_dict=hp, guard=False).guard is False
    assert M(mode='test', hparams_dict=hp).guard is False
    monkeypatch.setenv('SAVP_GUARD', '0')
    assert M(mode='train', hparams_dict=hp).guard is False
    assert guard_enabled(True, 'test') is False and guard_enabled(True, 'train') is True


def test_health_scalars_of_a_step_without_the_guard_are_empty():
    from video_prediction_amd.models import get_model_class
    M = get_model_class('savp')
    assert M.health_scalars({'d_loss': 0.0}) == {} and M.health_scalars(None) == {}
    got = M.health_scalars({'health': {'grad_norm_g': 2.0, 'skipped_g': 1, 'nonfinite_g': 0, 'consecutive_g': 1}})
    assert dict(got) == {'grad_norm_g': 2.0, 'skipped_steps_g': 1}

"""The training guard at op level on the GPU (pytest -m gpu; csrc/health.hip): savp_arena_health -- per-variable float64 sums of squares and
non-finite counts of a gradient arena, its totals, flag and counters -- against numpy float64, where non-finite values may sit, that equal
input gives equal bits with nothing cleared, savp_adam_guarded against savp_adam bit for bit and against "nothing stored", and what both
entries refuse.

Tolerance of the sums: the square of an fp32 is exact in float64 (24-bit significand squared = 48 bits; 1e-20 .. 1e+18 squared stays far
inside the float64 range), so the kernel and numpy add the same float64 terms and differ by the order of addition alone: at most about
n * 2^-53 relative for n positive terms, 2e-12 for the 2 * C + 7 = 16391 terms of the longest segment in the worst case and around
sqrt(n) * 2^-53 = 1.4e-14 in practice.  The bound is the issue's 1e-12."""
import ctypes

import numpy as np
import pytest
import torch

from video_prediction_amd import kernels as K
from video_prediction_amd import lib
from video_prediction_amd.engine import ParamGroup

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C = K.arena_health_chunk()
SHAPES = [(1,), (3,), (4,), (5,), (C - 1,), (C,), (C + 1,), (2 * C + 7,), (3, 5, 7)]
EINVAL = -1
BIG = 7                                   # the segment of 2 C + 7 floats: three items, the last one short


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def _group():
    """A ParamGroup over SHAPES whose gradient arena holds values of both signs from 1e-20 to 1e+18 in its variables and non-zero garbage
    (NaN, Inf, 3e30 in turn) in every padding float between the slots.  Returns (group, the arena as numpy)."""
    from collections import OrderedDict
    grp = ParamGroup(OrderedDict(('v%d' % i, s) for i, s in enumerate(SHAPES)), torch.device(DEV))
    rng = np.random.default_rng(11)
    arena = np.empty(grp.arena.size, dtype=np.float32)
    arena[:] = np.resize(np.array([np.nan, np.inf, 3e30, -np.inf], dtype=np.float32), arena.size)      # the padding keeps this
    for off, n, _ in grp.arena.offsets.values():
        arena[off:off + n] = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-20, 18, n)).astype(np.float32)
    grp.g.copy_(torch.from_numpy(arena))
    grp.enable_health()
    return grp, arena


def _reference(grp, arena):
    sums, bad = [], []
    for off, n, _ in grp.arena.offsets.values():
        x = arena[off:off + n].astype(np.float64)
        fin = np.isfinite(x)
        sums.append(float(np.sum(x[fin] ** 2)))
        bad.append(int((~fin).sum()))
    return np.array(sums), np.array(bad)


def _read(grp):
    torch.cuda.synchronize()
    st = grp.health_state.cpu().tolist()
    return dict(sumsq=grp.health_sumsq.cpu().numpy(), nonfinite=grp.health_nonfinite.cpu().numpy(), total=float(grp.health_total.cpu()[0]),
                total_nonfinite=st[0], ok=st[1], skipped=st[2], consecutive=st[3], first_bad=st[4])


def _check_against(got, sums, bad):
    for s in range(len(sums)):
        print('segment %d  n %6d  sumsq %.17g  ref %.17g  rel %.3e  nonfinite %d' % (
            s, int(np.prod(SHAPES[s])), got['sumsq'][s], sums[s], abs(got['sumsq'][s] - sums[s]) / sums[s], got['nonfinite'][s]))
    assert np.all(np.abs(got['sumsq'] - sums) <= 1e-12 * sums), (got['sumsq'], sums)
    assert abs(got['total'] - sums.sum()) <= 1e-12 * sums.sum(), (got['total'], sums.sum())
    assert np.array_equal(got['nonfinite'], bad), (got['nonfinite'], bad)
    assert got['total_nonfinite'] == int(bad.sum())


def test_reduction_matches_numpy_float64_and_ignores_the_padding():
    grp, arena = _group()
    items = grp.health_items.cpu().tolist()
    assert [it for it in items if it[0] == BIG] == [[BIG, 0, C], [BIG, C, C], [BIG, 2 * C, 7]]
    assert [it for it in items if it[0] == 5] == [[5, 0, C]] and len(items) == 12
    ok = grp.health()
    got = _read(grp)
    sums, bad = _reference(grp, arena)
    assert bad.sum() == 0
    _check_against(got, sums, bad)
    assert got['ok'] == 1 and int(ok.cpu()[0]) == 1 and ok.data_ptr() == grp.health_state.data_ptr() + 4
    assert (got['skipped'], got['consecutive'], got['first_bad']) == (0, 0, -1)
    assert [n for n, _, _ in grp.health_table()] == ['v%d' % i for i in range(len(SHAPES))]
    assert np.allclose([v for _, v, _ in grp.health_table()], np.sqrt(sums), rtol=1e-12)


def test_non_finite_values_are_counted_wherever_they_sit_and_the_counters_run():
    grp, arena = _group()
    clean = arena.copy()
    offs = [o for o, _, _ in grp.arena.offsets.values()]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    big = offs[BIG]
    arena[big] = nan                          # first element of a segment
    arena[big + 2 * C + 6] = -inf             # its last element, inside the tail of the short third item
    arena[big + C - 1] = inf                  # the element before an item boundary
    arena[big + C] = nan                      # ... and the one behind it
    arena[big + 2 * C + 4] = inf              # the first float of that tail
    arena[offs[3] + 4] = -inf                 # (5,): the one-float tail behind one float4
    arena[offs[8] + 104] = nan                # (3, 5, 7) = 105 floats: the tail again, last element of the last segment
    sums, bad = _reference(grp, arena)
    assert bad.tolist() == [0, 0, 0, 1, 0, 0, 0, 5, 1]
    grp.g.copy_(torch.from_numpy(arena))
    grp.health()
    got = _read(grp)
    _check_against(got, sums, bad)            # counts exact, the sums are the finite elements'
    assert got['ok'] == 0 and got['first_bad'] == 3
    assert (got['skipped'], got['consecutive']) == (1, 1)
    grp.health()
    got = _read(grp)
    assert (got['ok'], got['skipped'], got['consecutive'], got['first_bad']) == (0, 2, 2, 3)
    grp.g.copy_(torch.from_numpy(clean))
    grp.health()
    got = _read(grp)
    assert (got['ok'], got['skipped'], got['consecutive'], got['first_bad'], got['total_nonfinite']) == (1, 2, 0, -1, 0)
    # a single NaN in a one-element segment, the lowest index there is
    one = clean.copy()
    one[offs[0]] = nan
    grp.g.copy_(torch.from_numpy(one))
    grp.health()
    got = _read(grp)
    assert (got['ok'], got['first_bad'], got['skipped'], got['consecutive']) == (0, 0, 3, 1)
    assert got['sumsq'][0] == 0.0 and got['nonfinite'].tolist() == [1] + [0] * 8


@pytest.mark.parametrize('dirty', [False, True], ids=['clean', 'non_finite'])
def test_equal_input_gives_equal_bits_with_nothing_cleared(dirty):
    grp, arena = _group()
    if dirty:
        arena[grp.arena.offsets['v7'][0] + C] = np.float32(np.nan)
        grp.g.copy_(torch.from_numpy(arena))
    outs = lambda: [grp.health_sumsq, grp.health_nonfinite, grp.health_total, grp.health_state, grp.health_ws]
    grp.health()
    torch.cuda.synchronize()
    first = [_bits(t) for t in outs()]
    # every output and the workspace filled with 0xFF bytes (NaN as float64, -1 as int32); the two running counters back at their start
    for t in outs():
        t.view(torch.uint8).fill_(0xFF)
    grp.health_state[2:4].zero_()
    grp.health()
    torch.cuda.synchronize()
    second = [_bits(t) for t in outs()]
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert int(grp.health_state[1]) == (0 if dirty else 1)


@pytest.mark.parametrize('S', [K.ARENA_HEALTH_STAGE, K.ARENA_HEALTH_STAGE + 1], ids=['staged_fold', 'unstaged_fold'])
def test_both_paths_of_the_fold_pass_with_more_segments_than_threads(S):
    """One item per segment: a list of HL_STAGE items is the longest the fold pass keeps in LDS, one more takes the path that reads global
    memory; either way a thread owns several segments (S > 256).  Sizes 1 .. 9 floats, a NaN in every 97th segment."""
    from collections import OrderedDict
    grp = ParamGroup(OrderedDict(('v%d' % i, (1 + i % 9,)) for i in range(S)), torch.device(DEV))
    rng = np.random.default_rng(S)
    arena = np.full(grp.arena.size, np.nan, dtype=np.float32)                   # the padding stays NaN
    for i, (off, n, _) in enumerate(grp.arena.offsets.values()):
        arena[off:off + n] = rng.standard_normal(n).astype(np.float32)
        if i % 97 == 5:
            arena[off + n - 1] = np.float32(np.inf)
    grp.g.copy_(torch.from_numpy(arena))
    grp.enable_health()
    assert grp.health_items.shape[0] == S
    grp.health()
    got = _read(grp)
    sums, bad = _reference(grp, arena)
    assert np.all(np.abs(got['sumsq'] - sums) <= 1e-12 * sums) and np.array_equal(got['nonfinite'], bad)
    assert abs(got['total'] - sums.sum()) <= 1e-12 * sums.sum() and got['total_nonfinite'] == int(bad.sum()) > 0
    assert (got['ok'], got['first_bad'], got['skipped'], got['consecutive']) == (0, 5, 1, 1)


def _adam_inputs(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV), (0.1 * torch.randn(n, generator=g)).to(DEV),
            torch.rand(n, generator=g).to(DEV))


@pytest.mark.parametrize('n', [4, C + 4, 1000003])
def test_guarded_adam_equals_adam_when_ok_and_stores_nothing_otherwise(n):
    p0, g0, m0, v0 = _adam_inputs(n, n)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_dev = torch.tensor([3e-4], device=DEV)
    for kw in (dict(lr_t=2e-4), dict(lr_t=0.0, lr_t_dev=lr_dev), dict(lr_t=2e-4, gscale=0.5)):
        lr_t = kw.pop('lr_t')
        want = [t.clone() for t in (p0, m0, v0)]
        K.adam(want[0], g0, want[1], want[2], lr_t, 0.5, 0.999, **kw)
        got = [t.clone() for t in (p0, m0, v0)]
        K.adam_guarded(got[0], g0, got[1], got[2], lr_t, 0.5, 0.999, one, **kw)
        torch.cuda.synchronize()
        for a, b, name in zip(got, want, 'pmv'):
            assert torch.equal(a, b) and torch.equal(_bits(a), _bits(b)), (name, kw)
        assert not torch.equal(got[0], p0)                    # the update did happen
        # ok = 0: nothing is stored, whatever the gradient holds
        gbad = g0.clone()
        gbad[::3] = float('nan')
        gbad[1] = float('inf')
        kept = [t.clone() for t in (p0, m0, v0)]
        K.adam_guarded(kept[0], gbad, kept[1], kept[2], lr_t, 0.5, 0.999, zero, **kw)
        torch.cuda.synchronize()
        for a, b, name in zip(kept, (p0, m0, v0), 'pmv'):
            assert torch.equal(_bits(a), _bits(b)), (name, kw)


def test_refused_arguments_launch_nothing():
    grp, _ = _group()
    L = lib.get()

    def args():
        a = lib.SavpHealthArgs()
        a.x, a.n = grp.g.data_ptr(), grp.g.numel()
        a.S, a.n_items = grp.health_segments.shape[0], grp.health_items.shape[0]
        a.segments, a.items = grp.health_segments.data_ptr(), grp.health_items.data_ptr()
        a.sumsq, a.nonfinite, a.total_sumsq = grp.health_sumsq.data_ptr(), grp.health_nonfinite.data_ptr(), grp.health_total.data_ptr()
        base = grp.health_state.data_ptr()
        a.total_nonfinite, a.ok, a.counters = base, base + 4, base + 8
        a.ws, a.ws_bytes = grp.health_ws.data_ptr(), grp.health_ws.numel() * 8
        return a

    outs = [grp.health_sumsq, grp.health_nonfinite, grp.health_total, grp.health_state, grp.health_ws]
    for t in outs:
        t.view(torch.uint8).fill_(0xA5)
    torch.cuda.synchronize()
    before = [_bits(t) for t in outs]
    cases = [(f, 0) for f in ('x', 'segments', 'items', 'sumsq', 'nonfinite', 'total_sumsq', 'total_nonfinite', 'ok', 'counters', 'ws')]
    cases += [('S', 0), ('S', -1), ('n_items', 0), ('n', 0),                      # no segment, an empty item list, an empty arena
              ('x', grp.g.data_ptr() + 4), ('x', grp.g.data_ptr() + 8),           # misaligned arena
              ('ws', grp.health_ws.data_ptr() + 8),                                # misaligned workspace
              ('ws_bytes', K.arena_health_ws_bytes(grp.health_items.shape[0]) - 1), ('ws_bytes', 0)]      # short workspace
    for field, value in cases:
        a = args()
        setattr(a, field, value)
        assert L.savp_arena_health(lib.stream(), ctypes.byref(a)) == EINVAL, (field, value)
    assert L.savp_arena_health(lib.stream(), None) == EINVAL
    p, g, m, v = _adam_inputs(8, 1)
    ok = torch.ones(1, dtype=torch.int32, device=DEV)
    kept = [_bits(t) for t in (p, m, v)]
    P = lib.ptr
    for bad in ((None, g, m, v, ok), (p, None, m, v, ok), (p, g, None, v, ok), (p, g, m, None, ok), (p, g, m, v, None), (p[1:], g, m, v, ok)):
        assert L.savp_adam_guarded(lib.stream(), 4, P(bad[0]), P(bad[1]), P(bad[2]), P(bad[3]), 1e-3, 0.5, 0.999, 1e-8, 1.0, None,
                                   P(bad[4])) == EINVAL
    assert L.savp_adam_guarded(lib.stream(), 0, P(p), P(g), P(m), P(v), 1e-3, 0.5, 0.999, 1e-8, 1.0, None, P(ok)) == EINVAL
    torch.cuda.synchronize()
    for a, b in zip(before, [_bits(t) for t in outs]):
        assert torch.equal(a, b)
    for a, b in zip(kept, [_bits(t) for t in (p, m, v)]):
        assert torch.equal(a, b)
    # and the same arguments unchanged are accepted
    grp.health_state.zero_()
    assert L.savp_arena_health(lib.stream(), ctypes.byref(args())) == 0
    torch.cuda.synchronize()
    assert int(grp.health_state[1]) == 1

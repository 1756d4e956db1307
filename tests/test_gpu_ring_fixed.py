"""The fixed-problem instantiations of the ring convolution (csrc/conv_ring_fixed.h, option ring_fixed) against the generic conv_ring_kernel
and against fp64.

conv_ring_fixed_kernel<ID> is conv_ring_kernel's body with the geometry of one train-step problem folded at compile time: same entry table, K
walk, MFMA order, split-K and fold order, the float epilogue compiled from the same runtime switches.  So (a) for every table entry, called as
the step calls it (N = 32, dense tensors, bf16 source, bias / statistics / norm-backward sums / column gap / split-K where the call site has
them), destination, statistics and workspaces are bit-equal between ring_fixed = 0 and 1, guard planes in front of and behind the (dense)
destination keep their NaNs, and the counter option ring_fixed_taken rises by exactly 1; (b) a call that differs from an entry in one folded
value -- N, H, Cx, a source stride, the tile, the source dtype, a destination pointer off 16-byte alignment -- takes the generic kernel
(counter unmoved) and gives the ring_fixed = 0 result; (c) one stride-1 and one stride-2 data gradient are checked on the fixed path against
the fp64 tap loop of their bf16-rounded operands at tests/gpu_checks.py's TOL_EXACT, so the fixed path does not rest on equality with the
generic one alone; (d) a whole c2-shaped train step (B = 16, 64 x 64 x 3, context_frames 2, sequence_length 11: the shortest
the engine builds with the video discriminator's clip_length = 10), eager and replayed, gives array_equal losses and variables with the
option off and on, and takes the fixed kernels exactly as often as the layer table says."""
import numpy as np
import pytest
import torch

from tests.gpu_checks import DEV, TOL_EXACT, _taps_ref, pack_wd, pack_wt, rel_err, rne
from video_prediction_amd import kernels as K
from video_prediction_amd import lib

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
N = 32

# The table of csrc/conv_ring_fixed.h, as the train step calls each entry:
# (name, mode, (H, W, Cx) x side, (Ho, Wo, Cy) y side, k, s, pad, tile, splitk, bf16 source, bias + statistics, norm-backward channels, gap)
# Cx of a gapped data gradient counts the physical channels of the destination (logical + gap).
FP, DG = lib.CONV_FPROP, lib.CONV_DGRAD
ENTRIES = [
    ('gate32_dgrad', DG, (32, 32, 72), (32, 32, 128), 5, 1, 2, 0x711, 1, True, False, 32, (32, 8)),
    ('gate16_dgrad', DG, (16, 16, 136), (16, 16, 256), 5, 1, 2, 0x311, 1, True, False, 64, (64, 8)),
    ('gate8_dgrad_splitk2', DG, (8, 8, 264), (8, 8, 512), 5, 1, 2, 0x1311, 2, True, False, 128, (128, 8)),
    ('head3x3_fprop', FP, (64, 64, 32), (64, 64, 64), 3, 1, 1, 0x721, 1, True, True, 0, None),
    ('head3x3_dgrad', DG, (64, 64, 32), (64, 64, 64), 3, 1, 1, 0x721, 1, True, False, 32, None),
    ('down6_64_fprop_f32src', FP, (64, 64, 16), (32, 32, 32), 6, 2, 2, 0x311, 1, False, True, 0, None),
    ('down6_64_dgrad', DG, (64, 64, 16), (32, 32, 32), 6, 2, 2, 0x721, 1, True, False, 0, None),
    ('down4_32_fprop', FP, (32, 32, 40), (16, 16, 64), 4, 2, 1, 0x311, 1, True, True, 0, None),
    ('down4_32_dgrad', DG, (32, 32, 40), (16, 16, 64), 4, 2, 1, 0x711, 1, True, False, 0, None),
    ('down4_16_fprop', FP, (16, 16, 72), (8, 8, 128), 4, 2, 1, 0x311, 1, True, True, 0, None),
    ('down4_16_dgrad', DG, (16, 16, 72), (8, 8, 128), 4, 2, 1, 0x311, 1, True, False, 0, None),
    ('up6_16_fprop', FP, (16, 16, 64), (8, 8, 136), 6, 2, 2, 0x311, 1, True, False, 0, None),
    ('up6_16_dgrad', DG, (16, 16, 64), (8, 8, 136), 6, 2, 2, 0x311, 1, True, True, 0, None),
    ('up6_32_fprop', FP, (32, 32, 32), (16, 16, 136), 6, 2, 2, 0x311, 1, True, False, 0, None),
    ('up6_32_dgrad', DG, (32, 32, 32), (16, 16, 136), 6, 2, 2, 0x711, 1, True, True, 0, None),
    ('up6_64_fprop', FP, (64, 64, 32), (32, 32, 72), 6, 2, 2, 0x712, 1, True, False, 0, None),
    ('up6_64_dgrad', DG, (64, 64, 32), (32, 32, 72), 6, 2, 2, 0x721, 1, True, True, 0, None),
]
IDS = [e[0] for e in ENTRIES]
# launches per generator time step of each entry (a step of T frames runs T - 1 of them; the 32 x 32 and 16 x 16 gate layers exist twice)
PER_TIME_STEP = {'gate32_dgrad': 2, 'gate16_dgrad': 2}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else (torch.int64 if t.dtype == torch.float64 else torch.int32))


def _guarded(shape, dtype, fill=None):
    """A dense tensor between two NaN guard planes of one allocation: (whole buffer, the view)."""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), float('nan'), device=DEV, dtype=dtype)
    v = buf[1:-1]
    if fill is not None:
        v.copy_(fill)
    return buf, v


_DATA = {}


def _data(name, n=N, dims=None):
    """Operands of one entry, drawn once and left unchanged (bias, weights, norm parameters included)."""
    key = (name, n, dims)
    if key not in _DATA:
        e = ENTRIES[IDS.index(name)]
        _, mode, xs, ys, k, s, pad, tile, sk, src16, bs, nbc, gap = e
        if dims is not None:
            xs, ys = dims
        g = torch.Generator(device=DEV).manual_seed(1000 + IDS.index(name))

        def rn(*shape):
            return torch.randn(*shape, generator=g, device=DEV, dtype=F32)

        fprop = mode == FP
        x32, y32 = rn(n, *xs), rn(n, *ys)
        w32 = rn(1, k, k, xs[2], ys[2]) * 0.1
        wp = (pack_wt(w32) if fprop else pack_wd(w32)).contiguous()
        cdst = ys[2] if fprop else xs[2]
        d = dict(x32=x32, y32=y32, w32=w32, wp=wp, w16=wp.to(BF), bias=rn(cdst) if bs else None)
        if nbc:
            hw = xs[:2]
            d['nb'] = dict(x=rn(n, hw[0], hw[1], nbc), mean=rn(n, nbc) * 0.1, rstd=rn(n, nbc).abs() + 0.5, gamma=rn(nbc) * 0.3 + 1,
                           beta=rn(nbc) * 0.3)
        _DATA[key] = d
    return _DATA[key]


def _call(name, fixed, n=N, dims=None, tile=None, src_dtype=None, src_wide=0, dst_off=0):
    """One savp_conv call of entry `name` with option ring_fixed = fixed.  Returns (destination buffer with its guards, destination view,
    statistics, norm-backward sums, ring_fixed_taken afterwards).  The keyword arguments build the near misses."""
    e = ENTRIES[IDS.index(name)]
    _, mode, xs, ys, k, s, pad, tile0, sk, src16, bs, nbc, gap = e
    if dims is not None:
        xs, ys = dims
    d = _data(name, n, dims)
    fprop = mode == FP
    sdt = src_dtype or (BF if src16 else F32)
    src_fill, dshape = (d['x32'], (n,) + tuple(ys)) if fprop else (d['y32'], (n,) + tuple(xs))
    if src_wide:                                              # the source as a channel slice of a wider parent buffer
        parent = torch.full(tuple(src_fill.shape[:-1]) + (src_fill.shape[-1] + src_wide,), float('nan'), device=DEV, dtype=sdt)
        src = parent[..., :src_fill.shape[-1]]
        src.copy_(src_fill)
    else:
        src = src_fill.to(sdt).contiguous()
    if dst_off:                                               # a dense destination whose pointer is off 16-byte alignment
        numel = int(np.prod(dshape))
        buf = torch.full((numel + 2 * 64,), float('nan'), device=DEV, dtype=F32)
        dst = buf[64 + dst_off:64 + dst_off + numel].view(dshape)
    else:
        buf, dst = _guarded(dshape, F32)
    if gap:
        dst[..., gap[0]:gap[0] + gap[1]] = 123.0              # the gap's channels are not computed
    cdst = dshape[-1] - (gap[1] if gap else 0)
    stats = torch.zeros(n, cdst, 2, device=DEV, dtype=torch.float64) if bs else None
    nb = None
    if nbc:
        nb = dict(d['nb'], ws=torch.zeros(n, nbc, 2, device=DEV, dtype=torch.float64), c0=0, act='relu')
    geom = K.ConvGeom((1, k, k), (1, s, s), (0, pad, pad))
    xv, yv = (src, dst) if fprop else (dst, src)
    lib.set_option('ring_fixed', fixed)
    lib.set_option('ring_fixed_taken', 0)
    K.conv(mode, geom, xv, yv, d['wp'], bias=d['bias'], splitk=sk, tile=tile0 if tile is None else tile, precision=1, w16=d['w16'],
           stats=stats, dst_gap=gap, norm_bwd=nb)
    torch.cuda.synchronize()
    return buf, dst, stats, (nb['ws'] if nb else None), lib.get_option('ring_fixed_taken')


def _same(a, b):
    if a is None:
        return b is None
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('name', IDS)
def test_bitwise_equal_to_generic(name):
    e = ENTRIES[IDS.index(name)]
    try:
        b0, d0, s0, w0, t0 = _call(name, 0)
        b1, d1, s1, w1, t1 = _call(name, 1)
    finally:
        lib.set_option('ring_fixed', 1)
    assert (t0, t1) == (0, 1), 'ring_fixed_taken after the option-off / option-on call: %r' % ((t0, t1),)
    assert _same(b0, b1), 'destination (guards included) differs between ring_fixed 0 and 1'
    assert _same(s0, s1), 'statistics differ'
    assert _same(w0, w1), 'norm-backward sums differ'
    assert bool(torch.isnan(b1[0]).all()) and bool(torch.isnan(b1[-1]).all()), 'a guard plane was written'
    gap = e[12]
    keep = d1 if not gap else torch.cat([d1[..., :gap[0]], d1[..., gap[0] + gap[1]:]], dim=-1)
    assert bool(torch.isfinite(keep).all())
    if gap and e[8] == 1:
        assert bool((d1[..., gap[0]:gap[0] + gap[1]] == 123.0).all()), 'the gap was written'
    if s1 is not None:
        assert float(s1[..., 1].min()) > 0.0
    if w1 is not None:
        assert float(w1.abs().max()) > 0.0


NEAR = 'head3x3_fprop'
NEAR_MISSES = [
    ('N', dict(n=16)),
    ('H', dict(dims=((32, 64, 32), (32, 64, 64)))),
    ('Cx', dict(dims=((64, 64, 40), (64, 64, 64)))),
    ('source_stride', dict(src_wide=8)),
    ('tile', dict(tile=0x711)),
    ('fp32_source', dict(src_dtype=F32)),
    ('dst_misaligned', dict(dst_off=1)),
]


@pytest.mark.parametrize('what,kw', NEAR_MISSES, ids=[m[0] for m in NEAR_MISSES])
def test_near_miss_takes_generic(what, kw):
    try:
        b0, d0, s0, _, t0 = _call(NEAR, 0, **kw)
        b1, d1, s1, _, t1 = _call(NEAR, 1, **kw)
        hit = _call(NEAR, 1)[4]
    finally:
        lib.set_option('ring_fixed', 1)
    assert hit == 1, 'the unchanged call no longer takes the fixed kernel: the near misses prove nothing'
    assert (t0, t1) == (0, 0), '%s: ring_fixed_taken moved (%r)' % (what, (t0, t1))
    assert _same(b0, b1) and _same(s0, s1)
    assert bool(torch.isfinite(d1).all())


@pytest.mark.parametrize('name', ['gate16_dgrad', 'up6_32_dgrad'])
def test_fixed_path_against_fp64(name):
    """The rounded-operand check of tests/gpu_checks.py (check_tuning_table's `_exact` rows): fp64 tap loop of the bf16-rounded source and
    weights, bias in fp64, at TOL_EXACT."""
    e = ENTRIES[IDS.index(name)]
    _, mode, xs, ys, k, s, pad, tile, sk, src16, bs, nbc, gap = e
    d = _data(name)
    try:
        _, dst, stats, _, taken = _call(name, 1)
    finally:
        lib.set_option('ring_fixed', 1)
    assert taken == 1
    kk, ss, pp = (1, k, k), (1, s, s), (0, pad, pad)
    x5, y5 = d['x32'][:, None], d['y32'][:, None]
    # a bf16 source holds the rounded values already; the weights are rounded by the bf16 pack
    refq = _taps_ref(mode, rne(x5).double(), rne(d['w32']).double(), rne(y5).double(), kk, ss, pp)[:, 0]
    sumq = refq
    if d['bias'] is not None:
        refq = refq + d['bias'].double()
    got = dst
    if gap:
        keep = [c for c in range(dst.shape[-1]) if not (gap[0] <= c < gap[0] + gap[1])]
        got, refq = dst[..., keep], refq[..., keep]
    err = rel_err(got, refq)
    print('%s: rel err against the fp64 tap loop %.3g (bound %.3g)' % (name, err, TOL_EXACT))
    assert err <= TOL_EXACT
    if stats is not None:
        r2 = sumq.reshape(N, -1, sumq.shape[-1])
        e1, e2 = rel_err(stats[..., 0], r2.sum(1)), rel_err(stats[..., 1], (r2 * r2).sum(1))
        print('%s: statistics rel err %.3g / %.3g' % (name, e1, e2))
        assert e1 <= TOL_EXACT and e2 <= TOL_EXACT


def _step_run(fixed):
    """A c2-shaped engine (B = 16 -> N = 32, 64 x 64 x 3) from one seed: one eager train step, then the captured step and one replay."""
    import os
    from tests.gpu_model_checks import make_hparams
    from video_prediction_amd.models.savp_model import SAVPEngine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B, T = 16, 11
    K.set_conv_precision('bf16')
    K.enable_autotune(True)
    K.load_tuning(os.path.join(root, 'video_prediction_amd', 'tuning_gfx950_bf16.json'))
    lib.set_option('ring_fixed', fixed)
    # sequence_length 11 is the shortest the video discriminator's clip_length = 10 admits (a shorter clip_length is refused further down, by
    # the discriminator's batched spectral-norm kernel, so a 4-frame step cannot be built)
    hp = make_hparams(context_frames=2, sequence_length=T, batch_size=B, lr=2e-4, beta1=0.5, beta2=0.999, l1_weight=100.0,
                      l2_weight=0.0, kl_weight=1.0, video_sn_vae_gan_weight=0.1, video_sn_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0,
                      gan_feature_cdist_weight=0.0)
    eng = SAVPEngine(hp, (64, 64, 3), B, mode='train')
    g = torch.Generator(device='cpu').manual_seed(7)
    eng.set_images(torch.rand(T, B, 64, 64, 3, generator=g).to(DEV), time_major=True)
    losses = []
    lib.set_option('ring_fixed_taken', 0)
    losses.append(_to_np(eng.train_step()))                   # eager
    torch.cuda.synchronize()
    taken = lib.get_option('ring_fixed_taken')
    for _ in range(2):                                        # capture + first run, replay (the returned scalars are rewritten by a replay)
        losses.append(_to_np(eng.train_step()))
    torch.cuda.synchronize()
    assert eng.use_graph and eng.graph is not None, 'the step was not captured'
    variables = {n: eng.store[n].detach().cpu().numpy().copy() for n in eng.store.specs}
    return losses, variables, taken, T


def _to_np(l):
    if isinstance(l, dict):
        return {k: _to_np(v) for k, v in sorted(l.items())}
    if isinstance(l, (tuple, list)):
        return [_to_np(v) for v in l]
    return l.detach().cpu().numpy().copy() if torch.is_tensor(l) else np.asarray(l)


def _eq(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_eq(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b, equal_nan=False)


def test_whole_step_same_bits_and_count():
    try:
        l0, v0, t0, T = _step_run(0)
        l1, v1, t1, _ = _step_run(1)
    finally:
        lib.set_option('ring_fixed', 1)
        K.set_conv_precision('f32')
        K.enable_autotune(False)
    # every table entry runs once per generator time step (the two-layer gate convolutions twice), T - 1 time steps per train step
    expected = sum(PER_TIME_STEP.get(n, 1) for n in IDS) * (T - 1)
    assert expected > 0 and t0 == 0
    assert t1 == expected, 'fixed ring launches in one eager step: %d, the layer table says %d' % (t1, expected)
    assert _eq(l0, l1), 'losses differ between ring_fixed 0 and 1'
    assert v0.keys() == v1.keys()
    bad = [k for k in v0 if not np.array_equal(v0[k], v1[k])]
    assert not bad, 'variables differ between ring_fixed 0 and 1: %s' % bad[:5]

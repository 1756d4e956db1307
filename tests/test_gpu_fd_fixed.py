"""The fixed-problem instantiations of the implicit-GEMM FPROP / DGRAD kernel (csrc/conv_fd_fixed.h, option fd_fixed) against the generic
conv_fd_kernel and against fp64.

conv_fd_fixed_kernel<ID> is conv_fd_kernel's body with the geometry of one problem folded at compile time: same tile, K order, split-K
partition and MFMA sequence, the float epilogue compiled from the same runtime switches; only the gather's integer arithmetic differs.  So
(a) every table entry, called once at its real shape with each epilogue variant the train step uses for it (bias, leaky ReLU, the ReLU
gradient mask `aux`, beta = 1), writes a destination that is torch.equal to the generic kernel's (option off, same build, same inputs),
NaN guard planes around it untouched, split slices of a split-K entry included, and moves the counter fd_fixed_taken by exactly 1;
(b) the table's small probe problems -- 4x4x4 with stride (1,2,2) and (2,2,2), forward and data gradient, an odd H (output phases of
different extents, one of which leaves its second row tile at once), 72 destination channels, M = 36, split-K 1 and 2, 100 reduction
channels (the K tail inside the last K-tile) -- are also checked against the fp64 tap loop on their bf16-rounded operands at the existing
convolution tests' TOL_EXACT; (c) a call that differs from a probe in one folded value takes the generic kernel (counter unmoved) and still
matches fp64; (d) a whole train step of the bench configuration, eager and replayed, gives array_equal losses and variables with the option
off and on and takes the fixed kernels as often as a step logged on a -DSAVP_FD_LOG build (tests/tools/fd_problems.py) says."""
import ctypes

import numpy as np
import pytest
import torch

from tests.gpu_checks import DEV, TOL_EXACT, _taps_ref, pack_wd, pack_wt, rel_err, rne
from video_prediction_amd import kernels as K
from video_prediction_amd import lib

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
FP, DG = lib.CONV_FPROP, lib.CONV_DGRAD
LINE = ('mode', 'N', 'D', 'H', 'W', 'Cx', 'Do', 'Ho', 'Wo', 'Cy', 'kd', 'kh', 'kw', 'sd', 'sh', 'sw', 'pd', 'ph', 'pw', 'WM', 'WN', 'splitk',
        'flags', 'rank')


def _table():
    L = lib.get()
    out = []
    for i in range(L.savp_fd_fixed_count()):
        buf = (ctypes.c_int64 * 32)()
        assert L.savp_fd_fixed_probe(i, 0, buf, 32) == len(LINE)
        out.append(dict(zip(LINE, buf[:len(LINE)])))
    return out


TABLE = _table()
# the probe problems are the table's lines with N <= 3; everything else is a problem of the train step
PROBES = [i for i, e in enumerate(TABLE) if e['N'] <= 3]
STEP = [i for i, e in enumerate(TABLE) if e['N'] > 3]

# What a step of the bench configuration (batch 16, sequence 30, shipped tuning table) launches on conv_fd_kernel, from a -DSAVP_FD_LOG
# build: (mode, N, source dims of F, Cy) -> (launches per step, epilogue variants as (beta, act, alpha, bias)).  act 1: leaky ReLU;
# act 3: times (aux > 0 ? 1 : alpha), aux addressed like the destination.  One more problem recurs, the image discriminator's first layer
# (FPROP, N = 464, 64 x 64 x 6 -> 32 x 32 x 64, once per step): it was slower on a fixed instantiation and is not in the table.
LRELU, DMASK = lib.ACT_LRELU, lib.ACT_DLRELU_FROM_OUT
STEP_CALLS = {
    (FP, 32, (10, 64, 64, 32), 64): (3, [(0, LRELU, 0.1, True)]),
    (FP, 32, (9, 32, 32, 64), 128): (3, [(0, LRELU, 0.1, True)]),
    (FP, 32, (8, 16, 16, 128), 256): (3, [(0, LRELU, 0.1, True)]),
    (FP, 16, (10, 64, 64, 32), 64): (1, [(0, LRELU, 0.1, True)]),
    (FP, 16, (8, 16, 16, 128), 256): (1, [(0, LRELU, 0.1, True)]),
    (DG, 32, (8, 16, 16, 128), 256): (2, [(0, DMASK, 0.1, False)]),
    (DG, 32, (9, 32, 32, 64), 128): (2, [(0, DMASK, 0.1, False)]),
    (DG, 16, (8, 16, 16, 128), 256): (2, [(0, DMASK, 0.1, False), (1, DMASK, 0.1, False)]),
    (DG, 16, (9, 32, 32, 64), 128): (2, [(0, DMASK, 0.1, False), (1, DMASK, 0.1, False)]),
    (DG, 464, (1, 32, 32, 64), 128): (1, [(0, DMASK, 0.2, False)]),
    (DG, 32, (1, 1, 1, 8192), 100): (29, [(0, 0, 0.0, False)]),
    (FP, 464, (1, 1, 1, 256), 8): (2, [(0, 0, 0.0, True)]),
    (DG, 464, (1, 1, 1, 256), 8): (2, [(0, 0, 0.0, False), (1, 0, 0.0, False)]),
    (DG, 32, (1, 1, 1, 65536), 1): (2, [(0, DMASK, 0.1, False)]),
    (DG, 16, (1, 1, 1, 65536), 1): (2, [(0, DMASK, 0.1, False), (1, DMASK, 0.1, False)]),
}


def _key(e):
    return (e['mode'], e['N'], (e['D'], e['H'], e['W'], e['Cx']), e['Cy'])


def _name(i):
    e = TABLE[i]
    return '%d_%s_N%d_%dx%dx%dx%d_%dx%dx%dx%d' % (i, 'dgrad' if e['mode'] == DG else 'fprop', e['N'], e['D'], e['H'], e['W'], e['Cx'], e['Do'],
                                                  e['Ho'], e['Wo'], e['Cy'])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _shapes(e, n=None, xdims=None, s=None):
    """(x shape, y shape, kernel, stride, padding) of a table line in the rank the line names; n / xdims / s build the near misses."""
    n = e['N'] if n is None else n
    k, s, p = (e['kd'], e['kh'], e['kw']), s or (e['sd'], e['sh'], e['sw']), (e['pd'], e['ph'], e['pw'])
    xd = xdims or (e['D'], e['H'], e['W'])
    yd = tuple((i + 2 * pp - kk) // ss + 1 for i, pp, kk, ss in zip(xd, p, k, s))
    if xdims is None and s == (e['sd'], e['sh'], e['sw']):
        assert yd == (e['Do'], e['Ho'], e['Wo'])
    cut = {5: 0, 4: 1, 2: 3}[e['rank']]
    return (n,) + xd[cut:] + (e['Cx'],), (n,) + yd[cut:] + (e['Cy'],), k, s, p


def _operands(e, seed, **kw):
    xs, ys, k, s, p = _shapes(e, **kw)
    g = torch.Generator(device=DEV).manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=DEV, dtype=F32)

    fprop = e['mode'] == FP
    w32 = rn(k[0], k[1], k[2], e['Cx'], e['Cy']) * 0.1
    wp = (pack_wt(w32) if fprop else pack_wd(w32)).contiguous()
    d = dict(xs=xs, ys=ys, k=k, s=s, p=p, w32=w32, wp=wp, w16=wp.to(BF) if e['flags'] & 4 else None)
    d['src'] = rn(*(xs if fprop else ys))
    dshape = ys if fprop else xs
    d['dshape'] = dshape
    d['bias'] = rn(dshape[-1])
    d['lazy'] = lambda name: d.setdefault(name, rn(*dshape))  # 'aux' / 'old': drawn when a variant first needs them, then left unchanged
    return d


def _call(e, d, fixed, variant=(0, 0, 0.0, False), tile=None, src_wide=0, dst_off=0):
    """One savp_conv call with option fd_fixed = fixed.  Returns (destination buffer with its NaN guards, destination view, the split-K
    slices or None, fd_fixed_taken afterwards)."""
    beta, act, alpha, use_bias = variant
    fprop = e['mode'] == FP
    dshape = d['dshape']
    if src_wide:                                              # the source as a channel slice of a wider parent buffer
        parent = torch.full(tuple(d['src'].shape[:-1]) + (d['src'].shape[-1] + src_wide,), float('nan'), device=DEV, dtype=F32)
        src = parent[..., :d['src'].shape[-1]]
        src.copy_(d['src'])
    else:
        src = d['src']
    numel = int(np.prod(dshape))
    plane = numel // dshape[0]
    if dst_off:                                               # a dense destination whose pointer is off 16-byte alignment
        buf = torch.full((numel + 2 * plane,), float('nan'), device=DEV, dtype=F32)
        dst = buf[plane + dst_off:plane + dst_off + numel].view(dshape)
    else:
        buf = torch.full((dshape[0] + 2,) + tuple(dshape[1:]), float('nan'), device=DEV, dtype=F32)
        dst = buf[1:-1]
    if beta:
        dst.copy_(d['lazy']('old'))                           # beta = 1 adds to it
    else:
        dst.fill_(7.0)                                        # beta = 0 must overwrite it
    geom = K.ConvGeom(d['k'], d['s'], d['p'])
    xv, yv = (src, dst) if fprop else (dst, src)
    lib.set_option('fd_fixed', fixed)
    lib.set_option('fd_fixed_taken', 0)
    K.conv(e['mode'], geom, xv, yv, d['wp'], bias=d['bias'] if use_bias else None, beta=beta, act=act, alpha=alpha,
           aux=d['lazy']('aux') if act == DMASK else None, splitk=e['splitk'], tile=(0x100 | (e['WM'] << 4) | e['WN']) if tile is None else tile,
           precision=1, w16=d['w16'])
    torch.cuda.synchronize()
    parts = None
    if e['splitk'] > 1:
        parts = K.scratch(dst.device, e['splitk'] * numel)[:e['splitk'] * numel].clone()
    return buf, dst, parts, lib.get_option('fd_fixed_taken')


def _reference(e, d, variant=(0, 0, 0.0, False)):
    """fp64 tap loop on the bf16-rounded operands, then the epilogue in fp64."""
    beta, act, alpha, use_bias = variant
    fprop = e['mode'] == FP

    def five(t, shape):
        n, c = shape[0], shape[-1]
        sp = (1, 1, 1)[:5 - len(shape)] + tuple(shape[1:-1])
        return t.reshape((n,) + sp + (c,))

    xs, ys = d['xs'], d['ys']
    zx = torch.zeros(xs, device=DEV, dtype=torch.float64)
    zy = torch.zeros(ys, device=DEV, dtype=torch.float64)
    x5 = five(rne(d['src']).double() if fprop else zx, xs)
    y5 = five(zy if fprop else rne(d['src']).double(), ys)
    ref = _taps_ref(e['mode'], x5, rne(d['w32']).double(), y5, d['k'], d['s'], d['p']).reshape(d['dshape'])
    if use_bias:
        ref = ref + d['bias'].double()
    if beta:
        ref = ref + d['lazy']('old').double()
    if act == LRELU:
        ref = torch.maximum(ref, alpha * ref)
    elif act == DMASK:
        ref = ref * torch.where(d['lazy']('aux') > 0, 1.0, alpha).double()
    return ref


def _pair(e, d, variant):
    try:
        b0, d0, p0, t0 = _call(e, d, 0, variant)
        if b0.numel() > (8 << 20):                            # the largest problems: one destination on the device at a time
            del d0
            b0 = b0.cpu()
        b1, d1, p1, t1 = _call(e, d, 1, variant)
    finally:
        lib.set_option('fd_fixed', 1)
    what = 'variant (beta, act, alpha, bias) = %r' % (variant,)
    assert (t0, t1) == (0, 1), '%s: fd_fixed_taken after the option-off / option-on call: %r' % (what, (t0, t1))
    assert torch.equal(_bits(b0), _bits(b1.to(b0.device))), '%s: destination (guards included) differs between fd_fixed 0 and 1' % what
    assert bool(torch.isnan(b1[0]).all()) and bool(torch.isnan(b1[-1]).all()), '%s: a guard plane was written' % what
    assert bool(torch.isfinite(d1).all()), what
    if e['splitk'] > 1:
        assert torch.equal(_bits(p0), _bits(p1)), '%s: split-K slices differ' % what
        assert float(p1.abs().max()) > 0.0
    return d1


@pytest.mark.parametrize('i', STEP, ids=[_name(i) for i in STEP])
def test_step_entry_bitwise_equal_to_generic(i):
    """Each problem of the step once at its real shape, every epilogue variant the step uses for it."""
    e = TABLE[i]
    assert _key(e) in STEP_CALLS, 'table line %d is not a problem of the logged step' % i
    d = _operands(e, 2000 + i)
    for variant in STEP_CALLS[_key(e)][1]:
        _pair(e, d, variant)


def test_every_logged_problem_is_in_the_table():
    assert sorted(STEP_CALLS) == sorted(_key(TABLE[i]) for i in STEP)


@pytest.mark.parametrize('i', PROBES, ids=[_name(i) for i in PROBES])
def test_probe_against_generic_and_fp64(i):
    e = TABLE[i]
    d = _operands(e, 3000 + i)
    for variant in [(0, 0, 0.0, False), (1, DMASK, 0.1, True)] if e['splitk'] == 1 else [(0, 0, 0.0, False), (1, 0, 0.0, False)]:
        got = _pair(e, d, variant)
        err = rel_err(got, _reference(e, d, variant))
        print('%s %r: rel err against the fp64 tap loop %.3g (bound %.3g)' % (_name(i), variant, err, TOL_EXACT))
        assert err <= TOL_EXACT


def test_probes_cover_what_the_kernel_can_get_wrong():
    """The probe lines keep the properties they were chosen for (a table edit that loses one fails here)."""
    P = [TABLE[i] for i in PROBES]
    up = lambda a, b: -(-a // b)
    assert {(e['mode'], (e['sd'], e['sh'], e['sw'])) for e in P if e['kd'] == 4} == {(FP, (1, 2, 2)), (FP, (2, 2, 2)), (DG, (1, 2, 2)), (DG, (2, 2, 2))}
    assert {e['splitk'] for e in P} == {1, 2}
    assert any((e['Cy'] if e['mode'] == FP else e['Cx']) % 64 for e in P), 'no destination channel count off the tile'
    assert any(e['mode'] == FP and (e['N'] * e['Do'] * e['Ho'] * e['Wo']) % 64 for e in P), 'no M off the tile'
    assert any((e['Cy'] if e['mode'] == DG else e['Cx']) == 100 for e in P), 'no K tail inside the last K-tile'
    # a data gradient with an odd H: the largest output phase has two row tiles, another phase one
    odd = [e for e in P if e['mode'] == DG and e['H'] % 2 and e['sh'] == 2]
    assert odd
    for e in odd:
        m = lambda h: e['N'] * up(e['D'], e['sd']) * h * up(e['W'], e['sw'])
        assert up(m(up(e['H'], 2)), 64 * e['WM']) > up(m(e['H'] // 2), 64 * e['WM']), 'no output phase leaves a row tile early'


NEAR = PROBES[0]                                              # forward, 4x4x4, stride (1,2,2)
NEAR_MISSES = [
    ('N_plus_1', dict(n=TABLE[NEAR]['N'] + 1), {}),
    ('stride', dict(s=(1, 1, 1)), {}),
    ('tile', {}, dict(tile=0x112)),
    ('view_into_wider_buffer', {}, dict(src_wide=8)),
    ('base_not_16_byte_aligned', {}, dict(dst_off=1)),
    ('option_off', {}, {}),
]


@pytest.mark.parametrize('what,shape_kw,call_kw', NEAR_MISSES, ids=[m[0] for m in NEAR_MISSES])
def test_near_miss_takes_generic(what, shape_kw, call_kw):
    e = TABLE[NEAR]
    d = _operands(e, 4000, **shape_kw)
    try:
        hit = _call(e, _operands(e, 4000), 1)[3]
        _, got, _, taken = _call(e, d, 0 if what == 'option_off' else 1, **call_kw)
    finally:
        lib.set_option('fd_fixed', 1)
    assert hit == 1, 'the unchanged call no longer takes the fixed kernel: the near misses prove nothing'
    assert taken == 0, '%s: fd_fixed_taken moved' % what
    err = rel_err(got, _reference(e, d))
    print('%s: rel err against the fp64 tap loop %.3g (bound %.3g)' % (what, err, TOL_EXACT))
    assert err <= TOL_EXACT


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


def _step_run(fixed):
    """An engine of the bench configuration (batch 16, 64 x 64 x 3, sequence 30) from one seed: two eager train steps' worth of launches --
    one eager step, then the captured step -- and one replay."""
    import os
    from tests.gpu_model_checks import make_hparams
    from video_prediction_amd.models.savp_model import SAVPEngine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    B, T = 16, 30
    K.set_conv_precision('bf16')
    K.enable_autotune(True)
    K.load_tuning(os.path.join(root, 'video_prediction_amd', 'tuning_gfx950_bf16.json'))
    lib.set_option('fd_fixed', fixed)
    hp = make_hparams(context_frames=2, sequence_length=T, batch_size=B, lr=2e-4, beta1=0.5, beta2=0.999, l1_weight=100.0,
                      l2_weight=0.0, kl_weight=1.0, video_sn_vae_gan_weight=0.1, video_sn_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0,
                      gan_feature_cdist_weight=0.0)
    eng = SAVPEngine(hp, (64, 64, 3), B, mode='train')
    g = torch.Generator(device='cpu').manual_seed(7)
    eng.set_images(torch.rand(T, B, 64, 64, 3, generator=g).to(DEV), time_major=True)
    losses = []
    lib.set_option('fd_fixed_taken', 0)
    losses.append(_to_np(eng.train_step()))                   # eager
    torch.cuda.synchronize()
    taken = lib.get_option('fd_fixed_taken')
    for _ in range(2):                                        # capture + first run, replay (the returned scalars are rewritten by a replay)
        losses.append(_to_np(eng.train_step()))
    torch.cuda.synchronize()
    assert eng.use_graph and eng.graph is not None, 'the step was not captured'
    variables = {n: eng.store[n].detach().cpu().numpy().copy() for n in eng.store.specs}
    return losses, variables, taken


def test_whole_step_same_bits_and_count():
    try:
        l0, v0, t0 = _step_run(0)
        l1, v1, t1 = _step_run(1)
    finally:
        lib.set_option('fd_fixed', 1)
        K.set_conv_precision('f32')
        K.enable_autotune(False)
    expected = sum(n for n, _ in STEP_CALLS.values())         # the logged step's launches that match a table line
    assert expected > 0 and t0 == 0
    assert t1 == expected, 'fixed implicit-GEMM launches in one eager step: %d, the logged step says %d' % (t1, expected)
    assert _eq(l0, l1), 'losses differ between fd_fixed 0 and 1'
    assert v0.keys() == v1.keys()
    bad = [k for k in v0 if not np.array_equal(v0[k], v1[k])]
    assert not bad, 'variables differ between fd_fixed 0 and 1: %s' % bad[:5]

"""The shape-specialised instance-norm apply kernels (csrc/inorm_stream_fwd.hip / inorm_stream_bwd.hip, option inorm_fast) against the generic
ones and against the fp64 oracle.  The apply passes are elementwise and the specialisations compute every element by the generic kernels'
operations, so (a) every output, mean, rstd, dx, dgamma, dbeta must be bitwise equal between inorm_fast = 0 and 1; (b) the option-on result
agrees with oracle.ops.fused_instance_norm + activation (autograd for the backward) within check_inorm's tolerances: TOL_OP forward, 5e-5
backward; a bf16 destination must hold exactly the fp32 result rounded to bf16.  Shapes: the smallest that reach each way the kernels can go
wrong (a bf16 channel slice of a wider buffer, a ragged plane whose last workgroup is partial, two and three outputs routed by channel range,
C = 256, 2 / 4 / 8 pixel rows per thread, which the launcher only picks from N * HW >= 32 k pixels, a doubled grid, strided gradient views), and three calls that no specialisation
covers, which must take the generic kernels (counter option inorm_fast_taken)."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests.gpu_checks import DEV, TOL_OP, dev, rel_err, rnd
from video_prediction_amd import kernels as K
from video_prediction_amd import lib

pytestmark = pytest.mark.gpu
TOL_BWD = 5e-5
PAD = 4            # channels of NaN pattern on either side of every destination view
BF, F32 = torch.bfloat16, torch.float32

# (N, H, W, C, act, alpha, outputs [(first channel, count or 0 = all, dtype)], a specialisation covers it)
FWD_CASES = [
    (2, 16, 16, 32, 'relu', 0.0, [(0, 0, BF)], True),
    (3, 9, 31, 8, 'none', 0.0, [(0, 0, F32)], True),
    (2, 64, 64, 64, 'lrelu', 0.2, [(0, 32, F32), (32, 32, BF)], True),
    (2, 32, 32, 128, 'relu', 0.0, [(0, 0, F32), (0, 64, BF), (64, 64, F32)], True),
    (1, 16, 16, 256, 'relu', 0.0, [(0, 0, F32)], True),
    (2, 16, 16, 24, 'relu', 0.0, [(0, 0, F32)], False),
    (2, 16, 16, 32, 'elu', 0.0, [(0, 0, F32)], False),
    (2, 16, 16, 32, 'relu', 0.0, [(0, 0, F32), (0, 16, BF), (16, 16, F32), (0, 0, BF)], False),
    # more pixel rows per thread (the launcher picks them from N * HW): 2 on a ragged plane, 4, and 8 (backward: 2, 4, 4)
    (8, 63, 65, 32, 'relu', 0.0, [(0, 0, BF)], True),
    (16, 64, 64, 32, 'lrelu', 0.2, [(0, 16, F32), (16, 16, BF)], True),
    (32, 64, 64, 32, 'relu', 0.0, [(0, 0, F32)], True),
    # 16 rows of a generic workgroup's share against 8 per thread: the launcher doubles the grid; two outputs at 8 rows (forward only: the
    # backward doubles its grid in the two cases above already)
    (32, 64, 64, 64, 'relu', 0.0, [(0, 32, F32), (32, 32, BF)], True),
]
FWD_ONLY = {(32, 64, 64, 64)}
IDS = ['%dx%dx%dx%d_%s_%dout' % (c[0], c[1], c[2], c[3], c[4], len(c[6])) for c in FWD_CASES]
_REF = {}


def _act(t, act, alpha):
    return {'relu': torch.relu, 'lrelu': lambda v: O.lrelu(v, alpha), 'elu': torch.nn.functional.elu, 'none': lambda v: v}[act](t)


def _reference(case):
    """Inputs and the fp64 oracle of one shape, computed once and shared by the forward and backward tests."""
    N, H, W, C, act, alpha = case[:6]
    key = (N, H, W, C, act)
    if key not in _REF:
        rng = np.random.default_rng(11 + C + H)
        x = (rnd(rng, N, H, W, C) * 2 + 0.7).requires_grad_(True)
        g = (rnd(rng, C) * 0.5 + 1).requires_grad_(True)
        b = rnd(rng, C).requires_grad_(True)
        y = _act(O.fused_instance_norm(x, g, b), act, alpha)
        dys = [rnd(rng, N, H, W, C) for _ in range(3)]
        _REF[key] = dict(x=x, g=g, b=b, y=y.detach(), dys=dys, shift=rnd(rng, C) * 0.3, dx0=rnd(rng, N, H, W, C))
    return _REF[key]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _nan_buffers(N, H, W, C, outs):
    bufs, views = [], []
    for (c0, nc, dt) in outs:
        nc = nc or C
        buf = torch.full((N, H, W, nc + 2 * PAD), float('nan'), device=DEV, dtype=dt)
        bufs.append(buf)
        views.append(buf[..., PAD:PAD + nc])
    return bufs, views


def _sums_fwd(r):
    """What a producing convolution's epilogue leaves: float64 sum / sum of squares of x around a per-channel shift (its bias)."""
    d = r['x'].detach() - r['shift']
    N, C = d.shape[0], d.shape[-1]
    d = d.reshape(N, -1, C)
    return torch.stack([d.sum(1), (d * d).sum(1)], dim=-1).to(DEV).contiguous(), dev(r['shift'])


def _fwd(case, fast, with_stats):
    N, H, W, C, act, alpha, outs, _ = case
    r = _reference(case)
    bufs, views = _nan_buffers(N, H, W, C, outs)
    mean, rstd = torch.full((N, C), float('nan'), device=DEV), torch.full((N, C), float('nan'), device=DEV)
    kw = {}
    if with_stats:
        kw['stats'], kw['stats_shift'] = _sums_fwd(r)
    lib.set_option('inorm_fast', fast)
    lib.set_option('inorm_fast_taken', 0)
    K.instnorm_act_fwd(dev(r['x']), dev(r['g']), dev(r['b']), views, mean, rstd, act=act, alpha=alpha,
                       out_ranges=[(c0, nc) for (c0, nc, _) in outs], **kw)
    torch.cuda.synchronize()
    return bufs, views, mean, rstd, lib.get_option('inorm_fast_taken')


@pytest.mark.parametrize('with_stats', [False, True], ids=['own_stats', 'conv_stats'])
@pytest.mark.parametrize('case', FWD_CASES, ids=IDS)
def test_forward(case, with_stats):
    N, H, W, C, act, alpha, outs, covered = case
    r = _reference(case)
    if with_stats and 256 % (C // 4):
        # the apply pass alone needs a whole number of pixel rows per 256-thread workgroup: savp_instnorm_act_fwd refuses C = 24 with ready
        # statistics (SAVP_EINVAL), with either option value
        for fast in (0, 1):
            try:
                with pytest.raises(RuntimeError, match='savp_instnorm_act_fwd'):
                    _fwd(case, fast, True)
            finally:
                lib.set_option('inorm_fast', 1)
        return
    try:
        b0, v0, m0, r0, taken0 = _fwd(case, 0, with_stats)
        b1, v1, m1, r1, taken1 = _fwd(case, 1, with_stats)
        # the fp32 result of the same path, for the bf16 destinations
        full = _fwd(case[:6] + ([(0, 0, F32)], covered), 1, with_stats)[1][0]
    finally:
        lib.set_option('inorm_fast', 1)
    assert taken0 == 0 and taken1 == (1 if covered else 0), (taken0, taken1)
    for k, (c0, nc, dt) in enumerate(outs):
        nc = nc or C
        assert torch.equal(_bits(b0[k]), _bits(b1[k])), 'output %d differs between inorm_fast 0 and 1' % k       # pads included
        pads = torch.cat([b1[k][..., :PAD], b1[k][..., PAD + nc:]], dim=-1)
        assert bool(torch.isnan(pads).all()), 'output %d: channels outside its range were written' % k
        err = rel_err(full[..., c0:c0 + nc], r['y'][..., c0:c0 + nc])
        print('fwd %s out %d rel err %.3g' % (IDS[FWD_CASES.index(case)], k, err))
        if dt == BF:
            assert torch.equal(_bits(v1[k]), _bits(full[..., c0:c0 + nc].to(BF))), 'bf16 output %d is not the rounded fp32 result' % k
        else:
            assert torch.equal(_bits(v1[k]), _bits(full[..., c0:c0 + nc]))
        assert err <= TOL_OP, (k, err)
    assert torch.equal(_bits(m0), _bits(m1)) and torch.equal(_bits(r0), _bits(r1))
    assert not bool(torch.isnan(m1).any() | torch.isnan(r1).any())


# gradient views: (first channel, count as a fraction of C: 0 = all)
DY_VIEWS = {1: [(0, 0)], 2: [(0, 2), (1, 2)], 3: [(0, 0), (0, 2), (1, 2)]}
DX_MODES = [('f32', F32, 0), ('f32_acc', F32, 1), ('bf16', BF, 0)]


def _bwd(case, fast, ndy, dxm, with_stats, fwd):
    N, H, W, C, act, alpha = case[:6]
    r = _reference(case)
    mean, rstd = fwd
    ranges = [(h * C // d, C // d) if d else (0, 0) for (h, d) in DY_VIEWS[ndy]]
    dys = []
    for k, (c0, nc) in enumerate(ranges):          # every gradient view a channel slice of a wider buffer: pixel stride != channel count
        buf = torch.full((N, H, W, (nc or C) + 2 * PAD), float('nan'), device=DEV)
        buf[..., PAD:PAD + (nc or C)] = dev(r['dys'][k][..., c0:c0 + (nc or C)])
        dys.append(buf[..., PAD:PAD + (nc or C)])
    _, dt, beta = dxm
    dx = dev(r['dx0']).to(dt) if beta else torch.full((N, H, W, C), float('nan'), device=DEV, dtype=dt)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    kw = {}
    if with_stats:
        kw['stats'] = r['bwd_sums'][ndy].to(DEV).contiguous()
    lib.set_option('inorm_fast', fast)
    lib.set_option('inorm_fast_taken', 0)
    K.instnorm_act_bwd(dev(r['x']), dev(r['g']), dev(r['b']), None, mean, rstd, dys, dx, dg, db, dx_beta=beta, act=act, alpha=alpha,
                       dy_ranges=ranges, **kw)
    torch.cuda.synchronize()
    return dx, dg, db, lib.get_option('inorm_fast_taken')


def _bwd_reference(case, ndy):
    """fp64 autograd of the oracle for the sum of the gradient views, and the sums a data gradient's epilogue would leave: sum(dz), sum(dz * xhat)."""
    N, H, W, C, act, alpha = case[:6]
    r = _reference(case)
    if ('grads', ndy) not in r:
        dy = torch.zeros(N, H, W, C, dtype=torch.float64)
        for k, (h, d) in enumerate(DY_VIEWS[ndy]):
            c0, nc = (h * C // d, C // d) if d else (0, C)
            dy[..., c0:c0 + nc] += r['dys'][k][..., c0:c0 + nc]
        x, g, b = r['x'], r['g'], r['b']
        z = O.fused_instance_norm(x, g, b)
        y = _act(z, act, alpha)
        gx, gg, gb, gz = torch.autograd.grad((y * dy).sum(), [x, g, b, z])
        xhat = ((z - b) / g).detach().reshape(N, -1, C)
        gz = gz.reshape(N, -1, C)
        r[('grads', ndy)] = (gx, gg, gb)
        r.setdefault('bwd_sums', {})[ndy] = torch.stack([gz.sum(1), (gz * xhat).sum(1)], dim=-1)
    return r[('grads', ndy)]


@pytest.mark.parametrize('with_stats', [False, True], ids=['own_sums', 'conv_sums'])
@pytest.mark.parametrize('case', [c for c in FWD_CASES if c[7] and c[:4] not in FWD_ONLY],
                         ids=[i for i, c in zip(IDS, FWD_CASES) if c[7] and c[:4] not in FWD_ONLY])
def test_backward(case, with_stats):
    N, H, W, C, act, alpha = case[:6]
    r = _reference(case)
    try:
        lib.set_option('inorm_fast', 1)
        mean, rstd = torch.empty(N, C, device=DEV), torch.empty(N, C, device=DEV)
        K.instnorm_act_fwd(dev(r['x']), dev(r['g']), dev(r['b']), [torch.empty(N, H, W, C, device=DEV)], mean, rstd, act=act, alpha=alpha)
        for ndy in (1, 2, 3):
            gx, gg, gb = _bwd_reference(case, ndy)
            dx32 = None
            for dxm in DX_MODES:
                dx0, dg0, db0, taken0 = _bwd(case, 0, ndy, dxm, with_stats, (mean, rstd))
                dx1, dg1, db1, taken1 = _bwd(case, 1, ndy, dxm, with_stats, (mean, rstd))
                tag = '%s ndy %d dx %s' % (IDS[FWD_CASES.index(case)], ndy, dxm[0])
                assert (taken0, taken1) == (0, 1), (tag, taken0, taken1)
                assert torch.equal(_bits(dx0), _bits(dx1)), tag + ': dx differs between inorm_fast 0 and 1'
                assert torch.equal(_bits(dg0), _bits(dg1)) and torch.equal(_bits(db0), _bits(db1)), tag + ': dgamma / dbeta differ'
                if dxm[0] == 'f32':
                    dx32 = dx1
                    errs = (rel_err(dx1, gx), rel_err(dg1, gg), rel_err(db1, gb))
                    print('bwd %s rel err dx %.3g dgamma %.3g dbeta %.3g' % ((tag,) + errs))
                    assert max(errs) <= TOL_BWD, (tag, errs)
                elif dxm[0] == 'f32_acc':
                    err = rel_err(dx1, gx + r['dx0'])
                    print('bwd %s rel err dx %.3g' % (tag, err))
                    assert err <= TOL_BWD, (tag, err)
                else:
                    assert torch.equal(_bits(dx1), _bits(dx32.to(BF))), tag + ': bf16 dx is not the rounded fp32 result'
                assert rel_err(dg1, gg) <= TOL_BWD and rel_err(db1, gb) <= TOL_BWD, tag
    finally:
        lib.set_option('inorm_fast', 1)


def test_backward_fallbacks_take_the_generic_kernel():
    """C = 24, ELU and four gradient views: no specialisation, same result with the option on, right against the oracle."""
    try:
        for case, ndy in ((FWD_CASES[5], 1), (FWD_CASES[6], 2), (FWD_CASES[7], 4)):
            N, H, W, C, act, alpha = case[:6]
            r = _reference(case)
            lib.set_option('inorm_fast', 1)
            mean, rstd = torch.empty(N, C, device=DEV), torch.empty(N, C, device=DEV)
            K.instnorm_act_fwd(dev(r['x']), dev(r['g']), dev(r['b']), [torch.empty(N, H, W, C, device=DEV)], mean, rstd, act=act, alpha=alpha)
            dys64 = (r['dys'] + [r['dx0']])[:ndy]
            y = _act(O.fused_instance_norm(r['x'], r['g'], r['b']), act, alpha)
            gx, gg, gb = torch.autograd.grad((y * sum(dys64)).sum(), [r['x'], r['g'], r['b']])
            res = []
            for fast in (0, 1):
                lib.set_option('inorm_fast', fast)
                lib.set_option('inorm_fast_taken', 0)
                dx, dg, db = torch.empty(N, H, W, C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
                K.instnorm_act_bwd(dev(r['x']), dev(r['g']), dev(r['b']), None, mean, rstd, [dev(t) for t in dys64], dx, dg, db, act=act, alpha=alpha)
                torch.cuda.synchronize()
                assert lib.get_option('inorm_fast_taken') == 0
                res.append((dx, dg, db))
            for a, b in zip(*res):
                assert torch.equal(_bits(a), _bits(b))
            errs = (rel_err(res[1][0], gx), rel_err(res[1][1], gg), rel_err(res[1][2], gb))
            print('bwd fallback C %d %s ndy %d rel err %.3g %.3g %.3g' % ((C, act, ndy) + errs))
            assert max(errs) <= TOL_BWD, errs
    finally:
        lib.set_option('inorm_fast', 1)

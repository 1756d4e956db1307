"""The layer-norm Conv2DGRUCell (conv_rnn='gru' with conv_rnn_norm_layer='layer', opt-in; csrc/gru_two_pass.hip, K.convgru_ln_*): the four chunked
two-pass gate blocks against fp64 autograd (every view a strided slice of a guarded buffer, the workspace NaN-filled, the bounds TOL_OP and
AUX.TOL_GRAD as tests/test_gpu_gru_large.py uses them), what they refuse, and the opt-in model against the fp64 oracle extended by
tests/oracle_ln_gru.py with the helpers and bounds of tests/gpu_model_checks.py."""
import numpy as np
import pytest
import torch

from tests import gpu_checks_aux as AUX
from tests import gpu_model_checks as MC
from tests import oracle_ln_gru as OLG
from tests.bf16_exact import rel_err
from tests.gpu_checks import TOL_OP, dev, rnd
from video_prediction_amd import kernels as K
from video_prediction_amd import lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_GRAD = AUX.TOL_GRAD
GUARD = 9.0
EPS_LN = 1e-12


def _chunk_edge_case():
    """N = 2 and a plane of 3 chunks + 1 pixel, for the chunk size the launchers really use at that problem."""
    c = K.convgru_ln_chunk(2, 97)
    HW = 3 * c + 1
    assert K.convgru_ln_chunk(2, HW) == c
    return (2, 1, HW, 8, 2, 0.3)


# N, H, W, F, number of h' destinations / dy sources, offset of the gate pre-activations
CASES = [(1, 1, 1, 4, 1, 0.3),            # the smallest legal problem; its candidate group has variance 0 (see _reference)
         (3, 5, 7, 8, 2, 0.3),            # a small odd plane
         (2, 33, 40, 32, 4, 0.3),         # several chunks, four destinations / sources
         _chunk_edge_case(),              # HW = 3 * chunk + 1
         (2, 8, 8, 264, 3, 0.3),          # a group wider than one 256-channel slab
         (1, 32, 40, 4, 1, 8.0)]          # a mean far from zero: cancellation in the variance


def _assert_ok(res):
    for n, e, t in res:
        print('%-90s err %.3e  tol %.3e' % (n, e, t))
    bad = [(n, e, t) for (n, e, t) in res if not (e <= t)]
    assert not bad, 'parity failures (name, err, tol): %r' % bad


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _ln(x, gamma, beta):
    """tf.contrib.layers.layer_norm: per sample over (H, W, C), biased variance, eps 1e-12."""
    m = x.mean(dim=(1, 2, 3), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(1, 2, 3), keepdim=True)
    return (x - m) / torch.sqrt(v + EPS_LN) * gamma + beta


def _moments(x):
    m = x.mean(dim=(1, 2, 3))
    v = ((x - m[:, None, None, None]) ** 2).mean(dim=(1, 2, 3))
    return m, 1.0 / torch.sqrt(v + EPS_LN)


def gru_gates(pre, h, g1, b1):
    """(u, r*h) of the cell: reset and update normalised on their own."""
    F = h.shape[-1]
    r = torch.sigmoid(_ln(pre[..., :F], g1[:F], b1[:F]))
    u = torch.sigmoid(_ln(pre[..., F:], g1[F:], b1[F:]))
    return u, r * h


def gru_out(pre, h, u, g2, b2):
    return u * h + (1 - u) * torch.tanh(_ln(pre, g2, b2))


def _reference(case, scale_u=1.0):
    """Seeded fp64 inputs, outputs and autograd gradients of one case; computed once and only read afterwards.  The inputs are rounded to
    fp32 first, so that both sides see the same numbers.  scale_u: the update half of the gate pre-activations times this."""
    key = case + (scale_u,)
    if key not in _REF:
        N, H, W, F, nio, off = case
        rng = np.random.default_rng(311)
        f32 = lambda t: t.float().double()                  # noqa: E731
        pg = rnd(rng, N, H, W, 2 * F) * 1.5 + off
        pg[..., F:] *= scale_u
        pre_g = f32(pg).requires_grad_(True)
        pc = rnd(rng, N, H, W, F) * 1.5 - 0.2
        if H * W == 1:
            pc[0] = 0.37                                    # one sample's candidate group with variance 0: rstd = 1e6, the output finite
        pre_c = f32(pc).requires_grad_(True)
        h = f32(rnd(rng, N, H, W, F)).requires_grad_(True)
        g1, b1 = f32(rnd(rng, 2 * F) * 0.3 + 1).requires_grad_(True), f32(rnd(rng, 2 * F) * 0.3).requires_grad_(True)
        g2, b2 = f32(rnd(rng, F) * 0.3 + 1).requires_grad_(True), f32(rnd(rng, F) * 0.3).requires_grad_(True)
        u, rh = gru_gates(pre_g, h, g1, b1)
        u.retain_grad()
        hn = gru_out(pre_c, h, u, g2, b2)
        dys = [f32(rnd(rng, N, H, W, F)) for _ in range(nio)]
        drh = f32(rnd(rng, N, H, W, F))
        ((hn * sum(dys)).sum() + (rh * drh).sum()).backward()
        with torch.no_grad():
            mr, rr = _moments(pre_g[..., :F])
            mu, ru = _moments(pre_g[..., F:])
            m2, r2 = _moments(pre_c)
        _REF[key] = dict(pre_g=pre_g, pre_c=pre_c, h=h, g1=g1, b1=b1, g2=g2, b2=b2, u=u.detach(), du=u.grad, rh=rh.detach(),
                         hn=hn.detach(), dys=dys, drh=drh, dh_garbage=f32(rnd(rng, N, H, W, F)), m1=torch.stack([mr, mu], 1),
                         r1=torch.stack([rr, ru], 1), m2=m2[:, None], r2=r2[:, None])
    return _REF[key]


def _guarded(N, H, W, width, slots):
    """A buffer [N, H, W, width] full of GUARD and the channel slices `slots` = [(offset, count)] of it."""
    buf = torch.full((N, H, W, width), GUARD, device=DEV)
    return buf, [buf[..., o:o + c] for o, c in slots]


def _untouched(buf, slots):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    for o, c in slots:
        keep[o:o + c] = False
    return AUX.untouched(buf[..., keep], GUARD)


def _run_blocks(case, scale_u=1.0, forward_only=False):
    """The four blocks on one case: every view a strided slice of a wider guarded buffer.  Returns the buffers by name."""
    N, H, W, F, nio, _ = case
    ref = _reference(case, scale_u)
    Cx = 8
    ws = K.convgru_ln_ws(DEV, N, H * W, F)
    ws.fill_(float('nan'))                                     # the blocks never read what they did not write
    # the candidate conv's input buffer [x | h | r*h | guard]
    a_slots = [(Cx, F), (Cx + F, F)]
    abuf, (hv, rhv) = _guarded(N, H, W, Cx + 2 * F + 4, a_slots)
    hv.copy_(dev(ref['h'].detach()))
    pgd, pcd = dev(ref['pre_g'].detach()), dev(ref['pre_c'].detach())
    g1, b1, g2, b2 = (dev(ref[k].detach()) for k in ('g1', 'b1', 'g2', 'b2'))
    # the statistics [N][G], inside guarded rows of their own
    sbuf = torch.full((2, N + 2, 2), GUARD, device=DEV)
    m1, r1 = sbuf[0, 1:N + 1], sbuf[1, 1:N + 1]
    m2 = torch.full((N + 2, 1), GUARD, device=DEV)
    r2 = torch.full((N + 2, 1), GUARD, device=DEV)
    ud = torch.empty(N, H, W, F, device=DEV)
    K.convgru_ln_gates_fwd(pgd, hv, g1, b1, m1, r1, ud, rhv, ws)
    o_slots = [(k * (F + 4), F) for k in range(nio)]
    obuf, outs = _guarded(N, H, W, nio * (F + 4), o_slots)
    K.convgru_ln_out_fwd(pcd, hv, g2, b2, m2[1:N + 1], r2[1:N + 1], ud, outs, ws)
    stat_guards = (AUX.untouched(sbuf[:, 0], GUARD) + AUX.untouched(sbuf[:, N + 1], GUARD)
                   + sum(AUX.untouched(t[i], GUARD) for t in (m2, r2) for i in (0, N + 1)))
    got = dict(u=ud, rh=rhv, outs=outs, h_in=hv, m1=m1, r1=r1, m2=m2[1:N + 1], r2=r2[1:N + 1])
    if forward_only:
        torch.cuda.synchronize()
        got['guards'] = _untouched(abuf, a_slots) + _untouched(obuf, o_slots) + stat_guards
        return got
    dy_slots = [(4 + k * (F + 4), F) for k in range(nio)]
    dybuf, dyv = _guarded(N, H, W, 4 + nio * (F + 4), dy_slots)
    for v, d in zip(dyv, ref['dys']):
        v.copy_(dev(d))
    dhbuf, (dh,) = _guarded(N, H, W, F + 8, [(4, F)])
    dh.copy_(dev(ref['dh_garbage']))                           # out_bwd must overwrite this
    dpc, du = torch.empty(N, H, W, F, device=DEV), torch.empty(N, H, W, F, device=DEV)
    dpg = torch.empty(N, H, W, 2 * F, device=DEV)
    dq = [torch.zeros(c, dtype=torch.float64, device=DEV) for c in (2 * F, 2 * F, F, F)]
    K.convgru_ln_out_bwd(pcd, hv, g2, b2, m2[1:N + 1], r2[1:N + 1], ud, dyv, dpc, du, dh, dq[2], dq[3], ws)
    dh_out = dh.clone()
    drhbuf, (drhv,) = _guarded(N, H, W, F + 8, [(4, F)])
    drhv.copy_(dev(ref['drh']))
    K.convgru_ln_gates_bwd(pgd, hv, g1, b1, m1, r1, du, drhv, dpg, dh, dq[0], dq[1], ws)      # ... and this one adds to it
    torch.cuda.synchronize()
    got['guards'] = (_untouched(abuf, a_slots) + _untouched(obuf, o_slots) + _untouched(dybuf, dy_slots) + _untouched(dhbuf, [(4, F)])
                     + _untouched(drhbuf, [(4, F)]) + stat_guards)
    got.update(dpre_c=dpc, du=du, dpre_g=dpg, dh=dh, dh_out=dh_out, dg1=dq[0], db1=dq[1], dg2=dq[2], db2=dq[3])
    return got


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%d_%dx%dx%d_n%d_off%g' % c)
def test_ln_gate_blocks_vs_fp64(case):
    N, H, W, F, nio, off = case
    HW = H * W
    # the chunk size and workspace size kernels.py states are the launchers' own
    assert int(lib.get().savp_convgru_ln_chunk(N, HW)) == K.convgru_ln_chunk(N, HW)
    assert int(lib.get().savp_convgru_ln_ws_bytes(N, HW, F)) == K.convgru_ln_ws_bytes(N, HW, F)
    ref = _reference(case)
    got = _run_blocks(case)
    res = [('u', rel_err(got['u'], ref['u']), TOL_OP), ('rh', rel_err(got['rh'], ref['rh']), TOL_OP)]
    res += [('h_new%d' % k, rel_err(o, ref['hn']), TOL_OP) for k, o in enumerate(got['outs'])]
    # mean and rstd are [N][G]: G = 2 for the gates, 1 for the candidate
    assert tuple(got['m1'].shape) == tuple(got['r1'].shape) == (N, 2) and tuple(got['m2'].shape) == tuple(got['r2'].shape) == (N, 1)
    res += [(nm, rel_err(got[nm], ref[nm]), TOL_OP) for nm in ('m1', 'r1', 'm2', 'r2')]
    res.append(('finite', float(sum(int((~torch.isfinite(got[k])).sum()) for k in ('u', 'rh', 'dpre_c', 'dpre_g', 'dh', 'du'))
                                + sum(int((~torch.isfinite(o)).sum()) for o in got['outs'])), 0.0))
    res.append(('h_unchanged', rel_err(got['h_in'], ref['h'].detach().float()), 0.0))
    res.append(('guards', got['guards'], 0.0))
    u, dhp = ref['u'], sum(ref['dys'])
    for nm, key in (('dpre_c', 'pre_c'), ('dpre_g', 'pre_g')):
        res.append((nm, rel_err(got[nm], ref[key].grad), TOL_GRAD))
    res.append(('du', rel_err(got['du'], ref['du']), TOL_GRAD))
    res.append(('dh_after_out_bwd(overwritten)', rel_err(got['dh_out'], dhp * u), TOL_GRAD))
    res.append(('dh(accumulated)', rel_err(got['dh'], ref['h'].grad), TOL_GRAD))
    for nm, key in (('dg1', 'g1'), ('db1', 'b1'), ('dg2', 'g2'), ('db2', 'b2')):
        res.append((nm, rel_err(got[nm], ref[key].grad), TOL_GRAD))
    # a second run gives the same bits
    again = _run_blocks(case)
    for nm in ('u', 'rh', 'dpre_c', 'du', 'dpre_g', 'dh', 'dh_out', 'm1', 'r1', 'm2', 'r2', 'dg1', 'db1', 'dg2', 'db2'):
        res.append(('bits/' + nm, AUX.bits_equal(got[nm], again[nm]), 0.0))
    res += [('bits/h_new%d' % k, AUX.bits_equal(a, b), 0.0) for k, (a, b) in enumerate(zip(got['outs'], again['outs']))]
    _assert_ok([('convgru_ln_N%d_HW%d_F%d_off%g/%s' % (N, HW, F, off, n), e, t) for n, e, t in res])


def test_zero_variance_group_gives_the_activation_of_beta():
    """The candidate group of the 1 x 1 x 1 x 4 case holds four equal values: xhat = 0, rstd = 1e6, c = tanh(beta)."""
    case = CASES[0]
    ref, got = _reference(case), _run_blocks(case, forward_only=True)
    assert float(ref['pre_c'].detach().var(unbiased=False)) == 0.0
    assert float(got['r2'][0, 0]) == pytest.approx(1e6, rel=1e-6) and float(got['m2'][0, 0]) == float(ref['pre_c'].detach().float()[0, 0, 0, 0])
    want = ref['u'] * ref['h'].detach() + (1 - ref['u']) * torch.tanh(ref['b2'].detach())
    assert bool(torch.isfinite(got['outs'][0]).all()) and rel_err(got['outs'][0], want) <= TOL_OP


def test_reset_and_update_have_their_own_statistics():
    """Scaling the update half of the gate pre-activations leaves r (here r*h) and the reset statistics bit-identical; statistics over
    all 2F channels would move them.  (u itself stays within rounding, a layer norm being scale-invariant: its rstd takes the factor.)"""
    case = (3, 5, 7, 8, 2, 0.3)
    a, b = _run_blocks(case, forward_only=True), _run_blocks(case, scale_u=3.0, forward_only=True)
    assert AUX.bits_equal(a['rh'], b['rh']) == 0.0
    assert AUX.bits_equal(a['m1'][:, 0].contiguous(), b['m1'][:, 0].contiguous()) == 0.0
    assert AUX.bits_equal(a['r1'][:, 0].contiguous(), b['r1'][:, 0].contiguous()) == 0.0
    assert float((a['r1'][:, 1] / b['r1'][:, 1] - 3.0).abs().max()) < 1e-4
    assert float((a['m1'][:, 1] * 3.0 - b['m1'][:, 1]).abs().max()) < 1e-5
    assert rel_err(b['u'], _reference(case, 3.0)['u']) <= TOL_OP
    assert a['guards'] == 0.0 and b['guards'] == 0.0


def test_ln_gate_blocks_refuse_what_breaks_float4_access_or_lacks_a_workspace():
    """SAVP_EINVAL for F = 6, for a view whose base is 8 bytes off a 16-byte boundary, for one whose pixel stride is no multiple of 4, and for
    a null or short workspace; nothing is launched by a refused call.  The aligned twins with a whole workspace are accepted."""
    N, HW, F = 1, 16, 8
    ws = K.convgru_ln_ws(DEV, N, HW, F)
    short = ws[:ws.numel() - 1]
    assert ws.numel() * 8 == int(lib.get().savp_convgru_ln_ws_bytes(N, HW, F)) > 0
    pre_g, pre_c = torch.zeros(N, HW, 2 * F, device=DEV), torch.zeros(N, HW, F, device=DEV)
    u, du = torch.zeros(N, HW, F, device=DEV), torch.zeros(N, HW, F, device=DEV)
    g1, b1, g2, b2 = torch.ones(2 * F, device=DEV), torch.zeros(2 * F, device=DEV), torch.ones(F, device=DEV), torch.zeros(F, device=DEV)
    s1 = [torch.zeros(N, 2, device=DEV) for _ in range(2)]
    s2 = [torch.zeros(N, 1, device=DEV) for _ in range(2)]
    d1 = [torch.zeros(2 * F, dtype=torch.float64, device=DEV) for _ in range(2)]
    d2 = [torch.zeros(F, dtype=torch.float64, device=DEV) for _ in range(2)]
    wide = torch.zeros(N, HW, F + 4, device=DEV)
    good, off2 = wide[..., 4:], wide[..., 2:2 + F]
    odd = torch.zeros(N, HW, F + 2, device=DEV)[..., :F]
    ok = torch.zeros(N, HW, F, device=DEV)

    def gates_fwd(h=good, rh=ok, w=ws):
        K.convgru_ln_gates_fwd(pre_g, h, g1, b1, s1[0], s1[1], u, rh, w)

    def out_fwd(h=good, dst=(ok,), w=ws):
        K.convgru_ln_out_fwd(pre_c, h, g2, b2, s2[0], s2[1], u, list(dst), w)

    def out_bwd(dys=(ok,), dh=ok, w=ws):
        K.convgru_ln_out_bwd(pre_c, good, g2, b2, s2[0], s2[1], u, list(dys), ok.clone(), du, dh, d2[0], d2[1], w)

    def gates_bwd(drh=ok, dh=ok, w=ws):
        K.convgru_ln_gates_bwd(pre_g, good, g1, b1, s1[0], s1[1], du, drh, pre_g.clone(), dh, d1[0], d1[1], w)
    res = []
    p6, h6 = torch.zeros(N, HW, 12, device=DEV), torch.zeros(N, HW, 6, device=DEV)
    w6 = K.convgru_ln_ws(DEV, N, HW, 8)
    res.append(('f6/gates_fwd', AUX.refused(lambda: K.convgru_ln_gates_fwd(p6, h6, torch.ones(12, device=DEV), torch.zeros(12, device=DEV),
                                                                           torch.zeros(N, 2, device=DEV), torch.zeros(N, 2, device=DEV),
                                                                           h6.clone(), h6.clone(), w6)), 0.0))
    res.append(('f6/out_fwd', AUX.refused(lambda: K.convgru_ln_out_fwd(h6.clone(), h6, torch.ones(6, device=DEV), torch.zeros(6, device=DEV),
                                                                       torch.zeros(N, 1, device=DEV), torch.zeros(N, 1, device=DEV),
                                                                       h6.clone(), [h6.clone()], w6)), 0.0))
    for nm, bad in (('base', off2), ('stride', odd)):
        res.append(('%s/gates_fwd_h' % nm, AUX.refused(lambda: gates_fwd(h=bad)), 0.0))
        res.append(('%s/gates_fwd_rh' % nm, AUX.refused(lambda: gates_fwd(rh=bad)), 0.0))
        res.append(('%s/out_fwd_dst' % nm, AUX.refused(lambda: out_fwd(dst=(ok, bad))), 0.0))
        res.append(('%s/out_bwd_dy' % nm, AUX.refused(lambda: out_bwd(dys=(bad,))), 0.0))
        res.append(('%s/out_bwd_dh' % nm, AUX.refused(lambda: out_bwd(dh=bad)), 0.0))
        res.append(('%s/gates_bwd_drh' % nm, AUX.refused(lambda: gates_bwd(drh=bad)), 0.0))
        res.append(('%s/gates_bwd_dh' % nm, AUX.refused(lambda: gates_bwd(dh=bad)), 0.0))
    for nm, w in (('null', None), ('short', short)):
        for fn_nm, fn in (('gates_fwd', gates_fwd), ('out_fwd', out_fwd), ('out_bwd', out_bwd), ('gates_bwd', gates_bwd)):
            res.append(('ws_%s/%s' % (nm, fn_nm), AUX.refused(lambda: fn(w=w)), 0.0))
    # nothing ran: the statistics a launch would have written are untouched
    res.append(('nothing_launched', float(sum(int((t != 0).sum()) for t in s1 + s2)), 0.0))
    # the aligned twins with a whole workspace are accepted
    gates_fwd()
    out_fwd(dst=(ok.clone(), wide[..., :F]))
    out_bwd()
    gates_bwd()
    torch.cuda.synchronize()
    assert float(s1[1][0, 0]) == pytest.approx(1e6, rel=1e-6)          # a plane of zeros: rstd = 1 / sqrt(eps)
    _assert_ok([('convgru_ln_refuse/' + n, e, t) for n, e, t in res])


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: the opt-in model against the fp64 oracle, bounds of tests/gpu_model_checks.py
# ---------------------------------------------------------------------------------------------------------------------------------
LN_GRU = dict(conv_rnn='gru', conv_rnn_norm_layer='layer')
MODEL_CASES = [('default', LN_GRU), ('flow', dict(LN_GRU, transformation='flow')), ('learn_init', dict(LN_GRU, learn_initial_state=True)),
               ('norm_layer', dict(LN_GRU, norm_layer='layer'))]
CELL_NORMS = ('gates/reset/gamma', 'gates/reset/beta', 'gates/update/gamma', 'gates/update/beta', 'candidate/state/gamma',
              'candidate/state/beta')


@pytest.fixture
def ln_gru(monkeypatch):
    """The opt-in through the environment, the oracle extended by the layer-norm GRU branch."""
    monkeypatch.setenv('SAVP_LN_GRU', '1')
    OLG.install(monkeypatch)
    return monkeypatch


@pytest.mark.parametrize('tag,over', MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_generator_forward_vs_oracle(ln_gru, tag, over):
    _assert_ok(MC.check_generator_forward(nz=8, B=2, T=5, tag='gen_fwd_ln_gru_' + tag, **over))


@pytest.mark.parametrize('tag,over', MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_train_step_vs_oracle(ln_gru, tag, over):
    _assert_ok(MC.check_train_step(B=2, T=5, nz=8, steps=1, tag='train_ln_gru_' + tag, **over))


def test_generator_forward_at_64x80_vs_oracle(ln_gru):
    """Two layers above 1024 pixels (32 x 40): the same blocks, several chunks per plane."""
    _assert_ok(MC.check_generator_forward(nz=8, B=2, T=5, H=64, W=80, tag='gen_fwd_ln_gru_64x80', **LN_GRU))


def test_training_at_64x80_is_refused_at_build_time_with_the_plane_named(ln_gru):
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = MC.make_hparams(context_frames=2, sequence_length=4, nz=8, **LN_GRU)
    with pytest.raises(NotImplementedError, match=r"layer norm.*32x40 = 1280 pixels.*mode='train'"):
        SAVPEngine(hp, (64, 80, 3), 2, mode='train', seed=1)


def test_bf16_datapath_forward_vs_oracle(ln_gru):
    """The generator on the bf16 datapath against the fp64 oracle with the bounds of gpu_model_checks.check_model_bf16 (5e-2 on every row,
    the argmax rows reported)."""
    K.set_conv_precision('bf16')
    try:
        res = MC.check_generator_forward(nz=8, B=2, T=5, tag='bf16_gen_fwd_ln_gru', **LN_GRU)
    finally:
        K.set_conv_precision('f32')
    _assert_ok([(n + '(reported)', e, 1.0) if 'argmax' in n else (n, e, 5e-2) for n, e, t in res])


def _train_engine(graph):
    from video_prediction_amd import variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    B, T, H, W = 2, 4, 64, 64
    # T = 4 leaves clips of 3 frames, fewer than the video discriminator's strided 3-D convolutions take (4): the single-frame
    # discriminator stands in, so that the step still has both optimiser groups
    hp = MC.make_hparams(context_frames=2, sequence_length=T, clip_length=3, nz=8, lr=2e-4, beta1=0.5, beta2=0.999, l1_weight=100.0,
                         l2_weight=0.0, kl_weight=1.0, kl_anneal='none', video_sn_vae_gan_weight=0.0, video_sn_gan_weight=0.0,
                         image_sn_vae_gan_weight=0.1, image_sn_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0,
                         gan_feature_cdist_weight=0.0, **LN_GRU)
    vals = V.init_variables(V.variable_specs(hp, (H, W, 3), mode='train'), seed=4)
    rng = np.random.default_rng(9)
    for k in vals:
        if k.endswith('gamma'):
            vals[k] = (1 + 0.2 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('beta') or k.endswith('bias'):
            vals[k] = (0.1 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('kernel') and k.startswith('generator'):
            vals[k] = (vals[k] * 3).astype(np.float32)
    eng = SAVPEngine(hp, (H, W, 3), B, mode='train', values=vals, device=DEV)
    eng.use_graph = graph
    eng.set_images(MC.synth(hp, B, H, W, 3, 0).float().to(DEV), time_major=True)
    return eng, MC.make_noise(hp, B, seed=100, sampling=True)


def test_train_steps_from_one_state_repeat_their_bits_eagerly_and_replayed(ln_gru):
    """B = 2, T = 4.  Two eager train steps from one state, then four calls of an engine that captures its step (eager, capture + first
    run, replay, replay), each from that same state: every variable, both Adam moments and the losses agree bit for bit across all six."""
    from tests.test_gpu_soak import _bits, _restore, _state

    def run(eng, noise, calls):
        s0, outs = _state(eng), []
        for _ in range(calls):
            _restore(eng, s0)
            info = eng.train_step(noise)
            torch.cuda.synchronize()
            o = _state(eng)
            o['losses'] = torch.stack([info['d_loss'].reshape(()).double(), info['g_loss'].reshape(()).double()]).clone()
            outs.append((o, eng.graph is not None))
        return s0, outs
    eng, noise = _train_engine(False)
    s0, eager = run(eng, noise, 2)
    assert [g for _, g in eager] == [False, False]
    names = eng.store.names()
    cell = [n for n in names if n.endswith(CELL_NORMS) and '/conv2dgru_cell/' in n]
    assert len(cell) == 6 * 5
    first = eager[0][0]
    assert not torch.equal(_bits(first['g.p']), _bits(s0['g.p'])) and bool(torch.isfinite(first['losses']).all())
    arena = eng.store.groups['g'].arena
    for n in cell:                                             # the step moved each of the cell's norm variables
        assert not torch.equal(_bits(arena.view_of(first['g.p'], n)), _bits(arena.view_of(s0['g.p'], n))), n
    del eng
    eng, noise = _train_engine(True)
    _, replayed = run(eng, noise, 4)
    assert [g for _, g in replayed] == [False, True, True, True]          # eager, captured + run, replayed twice
    bad = [(i, k) for i, (o, _) in enumerate(eager[1:] + replayed) for k in first if not torch.equal(_bits(o[k]), _bits(first[k]))]
    assert not bad, bad


def test_checkpoint_holds_the_six_names_per_layer_and_restores_the_same_bits(ln_gru, tmp_path):
    from video_prediction_amd import checkpoint
    from video_prediction_amd.models import get_model_class
    Model = get_model_class('savp')
    hp = dict(LN_GRU, context_frames=2, sequence_length=5, nz=8)
    images = torch.rand(2, 5, 64, 64, 3, generator=torch.Generator().manual_seed(3)).cuda()
    a = Model(mode='test', hparams_dict=hp)
    a.build_graph({'images': images}, seed=5)
    for n in a.engine.store.names():                      # norm parameters that matter
        if n.endswith('beta'):
            a.engine.store[n].add_(0.1)
    a.engine.step = 7
    a.save(str(tmp_path / 'model-7'))
    names = set(checkpoint.variable_names(checkpoint.latest_checkpoint(str(tmp_path))))
    for i in range(5):
        for nm in CELL_NORMS:
            assert 'generator/rnn/savp_cell/gru_h%d/conv2dgru_cell/%s' % (i, nm) in names
    assert not [n for n in names if 'reset_update' in n]
    b = Model(mode='test', hparams_dict=hp)
    b.build_graph({'images': images}, seed=6)
    b.restore(str(tmp_path))
    for n in a.engine.store.names():
        assert torch.equal(a.engine.store[n], b.engine.store[n]), n
    noise = a.engine.default_noise()
    a.engine.set_images(images)
    b.engine.set_images(images)
    ga = a.engine.generate(noise).clone()
    gb = b.engine.generate(noise)
    assert bool(torch.isfinite(ga).all()) and AUX.bits_equal(ga, gb) == 0.0

"""The instance-norm Conv2DGRUCell on planes above 1024 pixels (csrc/gru_two_pass.hip, K.convgru_large_*): the four chunked two-pass gate
blocks against fp64 autograd on tests/aux_refs.gru_gates / gru_out (rows and bounds of tests/gpu_checks_aux.check_convgru_blocks, plus the
saved statistics, guard bands and bit-reproducibility), what they refuse, and a 64 x 80 generator -- conv-RNN planes of 32 x 40 in two
layers, 16 x 20 and 8 x 10 in the other three -- against the fp64 oracle: the generator forward on both datapaths.

The train step is NOT pinned at the model level.  The issue's rule was to use the first of 64 x 80 and 96 x 96 at which the ConvLSTM twin
(conv_rnn='lstm') passes gpu_model_checks.check_generator_forward and check_train_step(steps=1) at B = 2, T = 5, nz = 8, and otherwise to
pin the forward only and refuse mode='train' at build time.  Measured on an MI355X: the twin's forward passes at both frames; its train
step misses one gradient row at each -- 64 x 80: d_grads worst err/tol 2.04 (encoder/video/sn_conv0_1/conv3d/kernel, rel 4.09e-3);
96 x 96: g_grads worst err/tol 1.75 (lstm_z/basic_lstm_cell/kernel, rel 3.49e-3).  (The GRU model itself passed every row of both checks
at both frames in the same probe, gradients at 0.06 - 0.08 of their bound, before the refusal went in.)"""
import numpy as np
import pytest
import torch

from tests import aux_refs as R
from tests import gpu_checks_aux as AUX
from tests import gpu_model_checks as MC
from tests.bf16_exact import rel_err
from tests.gpu_checks import TOL_OP, dev, rnd
from video_prediction_amd import kernels as K
from video_prediction_amd import lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_GRAD = AUX.TOL_GRAD
GUARD = 9.0


def _chunk_edge_case():
    """N = 2 and a plane of 3 chunks + 1 pixel, for the chunk size the launchers really use at that problem."""
    c = K.convgru_large_chunk(2, 97)
    HW = 3 * c + 1
    assert K.convgru_large_chunk(2, HW) == c
    return (2, 1, HW, 8, 2, 0.3)


# N, H, W, F, number of h' destinations / dy sources, offset of the gate pre-activations
CASES = [(1, 1, 1, 4, 1, 0.3),            # the smallest legal problem
         (2, 5, 7, 8, 2, 0.3),            # a small odd plane through the new path
         (1, 1, 1025, 4, 1, 0.3),         # the first size the one-workgroup blocks refuse
         (1, 32, 40, 32, 3, 0.3),         # the 64 x 80 model's plane
         (2, 48, 48, 12, 4, 0.3),         # F not a power of two, four destinations
         (1, 60, 80, 4, 1, 0.3),          # KTH at native size, the narrowest F
         _chunk_edge_case(),              # HW = 3 * chunk + 1, two samples
         (1, 60, 80, 4, 1, 8.0)]          # a mean far from zero: cancellation in the variance


def _assert_ok(res):
    for n, e, t in res:
        print('%-90s err %.3e  tol %.3e' % (n, e, t))
    bad = [(n, e, t) for (n, e, t) in res if not (e <= t)]
    assert not bad, 'parity failures (name, err, tol): %r' % bad


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _moments(x):
    m = x.mean(dim=(1, 2))
    v = ((x - m[:, None, None, :]) ** 2).mean(dim=(1, 2))
    return m, 1.0 / torch.sqrt(v + R.EPS_IN)


def _reference(case):
    """Seeded fp64 inputs, outputs and autograd gradients of one case; computed once and only read afterwards."""
    if case not in _REF:
        N, H, W, F, nio, off = case
        rng = np.random.default_rng(307)
        pre_g = (rnd(rng, N, H, W, 2 * F) * 1.5 + off).requires_grad_(True)
        pre_c = (rnd(rng, N, H, W, F) * 1.5 - 0.2).requires_grad_(True)
        h = rnd(rng, N, H, W, F).requires_grad_(True)
        g1, b1 = (rnd(rng, 2 * F) * 0.3 + 1).requires_grad_(True), (rnd(rng, 2 * F) * 0.3).requires_grad_(True)
        g2, b2 = (rnd(rng, F) * 0.3 + 1).requires_grad_(True), (rnd(rng, F) * 0.3).requires_grad_(True)
        u, rh = R.gru_gates(pre_g, h, g1, b1)
        u.retain_grad()
        hn = R.gru_out(pre_c, h, u, g2, b2)
        dys = [rnd(rng, N, H, W, F) for _ in range(nio)]
        drh = rnd(rng, N, H, W, F)
        ((hn * sum(dys)).sum() + (rh * drh).sum()).backward()
        with torch.no_grad():
            m1, r1 = _moments(pre_g)
            m2, r2 = _moments(pre_c)
        _REF[case] = dict(pre_g=pre_g, pre_c=pre_c, h=h, g1=g1, b1=b1, g2=g2, b2=b2, u=u.detach(), du=u.grad, rh=rh.detach(),
                          hn=hn.detach(), dys=dys, drh=drh, dh_garbage=rnd(rng, N, H, W, F), m1=m1, r1=r1, m2=m2, r2=r2)
    return _REF[case]


def _guarded(N, H, W, width, slots):
    """A buffer [N, H, W, width] full of GUARD and the channel slices `slots` = [(offset, count)] of it."""
    buf = torch.full((N, H, W, width), GUARD, device=DEV)
    return buf, [buf[..., o:o + c] for o, c in slots]


def _untouched(buf, slots):
    keep = torch.ones(buf.shape[-1], dtype=torch.bool, device=buf.device)
    for o, c in slots:
        keep[o:o + c] = False
    return AUX.untouched(buf[..., keep], GUARD)


def _run_blocks(case):
    """The four blocks on one case: every view a strided slice of a wider guarded buffer.  Returns the buffers by name."""
    N, H, W, F, nio, _ = case
    ref = _reference(case)
    Cx = 8
    ws = K.convgru_large_ws(DEV, N, H * W, F)
    ws.fill_(float('nan'))                                     # the blocks never read what they did not write
    # the candidate conv's input buffer [x | h | r*h | guard]
    a_slots = [(Cx, F), (Cx + F, F)]
    abuf, (hv, rhv) = _guarded(N, H, W, Cx + 2 * F + 4, a_slots)
    hv.copy_(dev(ref['h'].detach()))
    pgd, pcd = dev(ref['pre_g'].detach()), dev(ref['pre_c'].detach())
    g1, b1, g2, b2 = (dev(ref[k].detach()) for k in ('g1', 'b1', 'g2', 'b2'))
    m1, r1 = torch.empty(N, 2 * F, device=DEV), torch.empty(N, 2 * F, device=DEV)
    m2, r2 = torch.empty(N, F, device=DEV), torch.empty(N, F, device=DEV)
    ud = torch.empty(N, H, W, F, device=DEV)
    K.convgru_large_gates_fwd(pgd, hv, g1, b1, m1, r1, ud, rhv, ws)
    o_slots = [(k * (F + 4), F) for k in range(nio)]
    obuf, outs = _guarded(N, H, W, nio * (F + 4), o_slots)
    K.convgru_large_out_fwd(pcd, hv, g2, b2, m2, r2, ud, outs, ws)
    dy_slots = [(4 + k * (F + 4), F) for k in range(nio)]
    dybuf, dyv = _guarded(N, H, W, 4 + nio * (F + 4), dy_slots)
    for v, d in zip(dyv, ref['dys']):
        v.copy_(dev(d))
    dhbuf, (dh,) = _guarded(N, H, W, F + 8, [(4, F)])
    dh.copy_(dev(ref['dh_garbage']))                           # out_bwd must overwrite this
    dpc, du = torch.empty(N, H, W, F, device=DEV), torch.empty(N, H, W, F, device=DEV)
    dpg = torch.empty(N, H, W, 2 * F, device=DEV)
    dq = [torch.zeros(c, dtype=torch.float64, device=DEV) for c in (2 * F, 2 * F, F, F)]
    K.convgru_large_out_bwd(pcd, hv, g2, b2, m2, r2, ud, dyv, dpc, du, dh, dq[2], dq[3], ws)
    dh_out = dh.clone()
    drhbuf, (drhv,) = _guarded(N, H, W, F + 8, [(4, F)])
    drhv.copy_(dev(ref['drh']))
    K.convgru_large_gates_bwd(pgd, hv, g1, b1, m1, r1, du, drhv, dpg, dh, dq[0], dq[1], ws)      # ... and this one adds to it
    torch.cuda.synchronize()
    guards = (_untouched(abuf, a_slots) + _untouched(obuf, o_slots) + _untouched(dybuf, dy_slots) + _untouched(dhbuf, [(4, F)])
              + _untouched(drhbuf, [(4, F)]))
    return dict(u=ud, rh=rhv, outs=outs, dpre_c=dpc, du=du, dpre_g=dpg, dh=dh, dh_out=dh_out, guards=guards, h_in=hv,
                m1=m1, r1=r1, m2=m2, r2=r2, dg1=dq[0], db1=dq[1], dg2=dq[2], db2=dq[3])


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%d_%dx%dx%d_n%d_off%g' % c)
def test_large_gate_blocks_vs_fp64(case):
    N, H, W, F, nio, off = case
    HW = H * W
    # the chunk size and workspace size kernels.py states are the launchers' own
    assert int(lib.get().savp_convgru_large_chunk(N, HW)) == K.convgru_large_chunk(N, HW)
    assert int(lib.get().savp_convgru_large_ws_bytes(N, HW, F)) == K.convgru_large_ws_bytes(N, HW, F)
    ref = _reference(case)
    got = _run_blocks(case)
    res = [('u', rel_err(got['u'], ref['u']), TOL_OP), ('rh', rel_err(got['rh'], ref['rh']), TOL_OP)]
    res += [('h_new%d' % k, rel_err(o, ref['hn']), TOL_OP) for k, o in enumerate(got['outs'])]
    res += [(nm, rel_err(got[nm], ref[nm]), TOL_OP) for nm in ('m1', 'r1', 'm2', 'r2')]
    res.append(('h_unchanged', rel_err(got['h_in'], ref['h'].detach().float()), 0.0))
    res.append(('guards', got['guards'], 0.0))
    u, dhp = ref['u'], sum(ref['dys'])
    floor = float(ref['h'].grad.abs().max())      # HW = 1: the norm's input gradient is 0 exactly; measure it on the scale of dh
    for nm, key in (('dpre_c', 'pre_c'), ('dpre_g', 'pre_g')):
        g = ref[key].grad
        res.append((nm, float((got[nm].double().cpu() - g).abs().max()) / max(float(g.abs().max()), 1e-6 * floor if HW == 1 else 0),
                    TOL_GRAD))
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
    _assert_ok([('convgru_large_N%d_HW%d_F%d_off%g/%s' % (N, HW, F, off, n), e, t) for n, e, t in res])


def test_large_gate_blocks_refuse_what_breaks_float4_access_or_lacks_a_workspace():
    """SAVP_EINVAL for F = 6, for a view whose base is 8 bytes off a 16-byte boundary, for one whose pixel stride is no multiple of 4, and for
    a null or short workspace; the aligned twin of each call with a whole workspace is accepted."""
    N, HW, F = 1, 16, 8
    ws = K.convgru_large_ws(DEV, N, HW, F)
    short = ws[:ws.numel() - 1]
    assert ws.numel() * 8 == int(lib.get().savp_convgru_large_ws_bytes(N, HW, F)) > 0
    pre_g, pre_c = torch.zeros(N, HW, 2 * F, device=DEV), torch.zeros(N, HW, F, device=DEV)
    u, du = torch.zeros(N, HW, F, device=DEV), torch.zeros(N, HW, F, device=DEV)
    g1, b1, g2, b2 = torch.ones(2 * F, device=DEV), torch.zeros(2 * F, device=DEV), torch.ones(F, device=DEV), torch.zeros(F, device=DEV)
    s1 = [torch.zeros(N, 2 * F, device=DEV) for _ in range(2)]
    s2 = [torch.zeros(N, F, device=DEV) for _ in range(2)]
    d1 = [torch.zeros(2 * F, dtype=torch.float64, device=DEV) for _ in range(2)]
    d2 = [torch.zeros(F, dtype=torch.float64, device=DEV) for _ in range(2)]
    wide = torch.zeros(N, HW, F + 4, device=DEV)
    good, off2 = wide[..., 4:], wide[..., 2:2 + F]
    odd = torch.zeros(N, HW, F + 2, device=DEV)[..., :F]
    ok = torch.zeros(N, HW, F, device=DEV)

    def gates_fwd(h=good, rh=ok, w=ws):
        K.convgru_large_gates_fwd(pre_g, h, g1, b1, s1[0], s1[1], u, rh, w)

    def out_fwd(h=good, dst=(ok,), w=ws):
        K.convgru_large_out_fwd(pre_c, h, g2, b2, s2[0], s2[1], u, list(dst), w)

    def out_bwd(dys=(ok,), dh=ok, w=ws):
        K.convgru_large_out_bwd(pre_c, good, g2, b2, s2[0], s2[1], u, list(dys), ok.clone(), du, dh, d2[0], d2[1], w)

    def gates_bwd(drh=ok, dh=ok, w=ws):
        K.convgru_large_gates_bwd(pre_g, good, g1, b1, s1[0], s1[1], du, drh, pre_g.clone(), dh, d1[0], d1[1], w)
    res = []
    p6, h6 = torch.zeros(N, HW, 12, device=DEV), torch.zeros(N, HW, 6, device=DEV)
    w6 = K.convgru_large_ws(DEV, N, HW, 8)
    res.append(('f6/gates_fwd', AUX.refused(lambda: K.convgru_large_gates_fwd(p6, h6, torch.ones(12, device=DEV), torch.zeros(12, device=DEV),
                                                                              torch.zeros(N, 12, device=DEV), torch.zeros(N, 12, device=DEV),
                                                                              h6.clone(), h6.clone(), w6)), 0.0))
    res.append(('f6/out_fwd', AUX.refused(lambda: K.convgru_large_out_fwd(h6.clone(), h6, torch.ones(6, device=DEV), torch.zeros(6, device=DEV),
                                                                          torch.zeros(N, 6, device=DEV), torch.zeros(N, 6, device=DEV),
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
    # the aligned twins with a whole workspace are accepted
    gates_fwd()
    out_fwd(dst=(ok.clone(), wide[..., :F]))
    out_bwd()
    gates_bwd()
    torch.cuda.synchronize()
    _assert_ok([('convgru_large_refuse/' + n, e, t) for n, e, t in res])


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: 64 x 80 frames against the fp64 oracle, bounds of tests/gpu_model_checks.py
# ---------------------------------------------------------------------------------------------------------------------------------
GRU = dict(conv_rnn='gru')
FRAME = dict(H=64, W=80)
SMALL = dict(B=2, T=5, nz=8, **FRAME)
LARGE_LAYERS, SMALL_LAYERS = [0, 4], [1, 2, 3]
MODEL_CASES = [('default', GRU), ('flow', dict(GRU, transformation='flow')), ('learn_init', dict(GRU, learn_initial_state=True))]


class _Spy(object):
    """Counts the calls of the forward gate-block wrappers the generator makes, by family."""

    def __init__(self, monkeypatch):
        self.n = {'large': 0, 'small': 0}
        for fam, names in (('large', ['convgru_large_gates_fwd', 'convgru_large_out_fwd']), ('small', ['convgru_gates_fwd', 'convgru_out_fwd'])):
            for nm in names:
                monkeypatch.setattr(K, nm, self._wrap(getattr(K, nm), fam))

    def _wrap(self, fn, fam):
        def counted(*a, **kw):
            self.n[fam] += 1
            return fn(*a, **kw)
        return counted

    def check(self):
        # two large and three small layers, the same number of blocks per step in each
        assert self.n['large'] > 0 and self.n['large'] * len(SMALL_LAYERS) == self.n['small'] * len(LARGE_LAYERS), self.n


@pytest.mark.parametrize('tag,over', MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_generator_forward_vs_oracle(monkeypatch, tag, over):
    spy = _Spy(monkeypatch)
    res = MC.check_generator_forward(tag='gen_fwd_gru_large_' + tag, **SMALL, **over)
    spy.check()
    _assert_ok(res)


def test_bf16_datapath_forward_vs_oracle(monkeypatch):
    """The generator on the bf16 datapath against the fp64 oracle with the bounds of gpu_model_checks.check_model_bf16 (5e-2 on every row,
    the argmax rows reported)."""
    spy = _Spy(monkeypatch)
    K.set_conv_precision('bf16')
    try:
        res = MC.check_generator_forward(tag='bf16_gen_fwd_gru_large', **SMALL, **GRU)
    finally:
        K.set_conv_precision('f32')
    spy.check()
    _assert_ok([(n + '(reported)', e, 1.0) if 'argmax' in n else (n, e, 5e-2) for n, e, t in res])


def test_the_layers_above_1024_pixels_take_the_new_blocks_and_repeat_their_bits():
    """An inference engine at 64 x 80: layers 0 and 4 carry the flag, a workspace of the helper's size and a non-zero launch counter, layers
    1 - 3 do not; a second forward from the same inputs gives the same generated frames bit for bit."""
    from video_prediction_amd import variables as V
    from video_prediction_amd.models.savp_cell import gru_large_layers
    from video_prediction_amd.models.savp_model import SAVPEngine
    B, T, H, W = SMALL['B'], SMALL['T'], SMALL['H'], SMALL['W']
    hp = MC.make_hparams(context_frames=2, sequence_length=T, nz=SMALL['nz'], schedule_sampling='inverse_sigmoid', **GRU)
    vals = V.init_variables(V.variable_specs(hp, (H, W, 3), mode='test'), seed=4)
    eng = SAVPEngine(hp, (H, W, 3), B, mode='test', values=vals, device=DEV)
    eng.mode = 'train'                                       # the posterior + prior unroll, as gpu_model_checks.check_generator_forward runs it
    eng.set_images(MC.synth(hp, B, H, W, 3, 0).float().to(DEV), time_major=True)
    noise = MC.make_noise(hp, B, sampling=True)
    outs = []
    for _ in range(2):
        eng.prep_generator_weights()
        outs.append(eng.forward_generator(noise).clone())
        torch.cuda.synchronize()
    gen = eng.gen
    assert gru_large_layers(H, W, hp.ngf) == LARGE_LAYERS
    assert [L['idx'] for L in gen.layers if L['rnn']] == sorted(LARGE_LAYERS + SMALL_LAYERS)
    for L in gen.layers:
        if L['rnn']:
            assert L['gru_large'] == (L['idx'] in LARGE_LAYERS), (L['idx'], L['hw'])
            if L['gru_large']:
                assert L['gru_large_calls'] == 2 * 2 * (T - 1)
                assert L['gru_ws'].numel() * 8 == K.convgru_large_ws_bytes(gen.N, L['hw'][0] * L['hw'][1], L['f'])
            else:
                assert 'gru_ws' not in L
    assert bool(torch.isfinite(outs[0]).all()) and AUX.bits_equal(outs[0], outs[1]) == 0.0


def test_training_at_such_a_frame_is_refused_at_build_time_with_the_plane_named():
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = MC.make_hparams(context_frames=2, sequence_length=4, nz=8, **GRU)
    with pytest.raises(NotImplementedError, match=r"32x40 = 1280 pixels.*mode='train'"):
        SAVPEngine(hp, (64, 80, 3), 2, mode='train', seed=1)
    SAVPEngine(hp, (64, 64, 3), 2, mode='train', seed=1)     # planes of 32 x 32 and below: unchanged

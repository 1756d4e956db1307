"""Conv2DGRUCell without a normaliser on the HIP path (conv_rnn = 'gru' with conv_rnn_norm_layer = 'none' or ablation_conv_rnn_norm):
the four pointwise gate blocks savp_convgru_plain_* against fp64 autograd on tests/gru_plain_refs.py (rows and bounds of
tests/gpu_checks_aux.check_convgru_blocks), the generator and one train step against the fp64 oracle on both datapaths, bit-reproducibility,
and the combinations that stay refused."""
import numpy as np
import pytest
import torch

from tests import gpu_checks_aux as AUX
from tests import gpu_model_checks as MC
from tests import gru_plain_refs as R
from tests import oracle_gru_plain
from tests.bf16_exact import rel_err
from tests.gpu_checks import TOL_OP, dev, rnd
from video_prediction_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL_GRAD = AUX.TOL_GRAD
GUARD = 9.0

# N, H, W, F, number of h' destinations / dy sources
CASES = [(1, 1, 1, 4, 1),           # the smallest legal problem
         (3, 5, 7, 12, 2),          # F not a power of two; N * HW * F / 4 = 315 items: not a multiple of the 256-thread block
         (2, 1, 257, 128, 4),       # four destinations
         (1, 32, 41, 8, 1),         # a plane of 1312 pixels: the normalised blocks refuse more than 1024
         (2, 32, 32, 32, 3)]        # three destinations


def _assert_ok(res):
    for n, e, t in res:
        print('%-90s err %.3e  tol %.3e' % (n, e, t))
    bad = [(n, e, t) for (n, e, t) in res if not (e <= t)]
    assert not bad, 'parity failures (name, err, tol): %r' % bad


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _reference(case):
    """Seeded fp64 inputs, outputs and autograd gradients of one case; computed once and only read afterwards."""
    if case not in _REF:
        N, H, W, F, nio = case
        rng = np.random.default_rng(211)
        pre_g = (rnd(rng, N, H, W, 2 * F) * 1.5 + 0.3).requires_grad_(True)
        pre_c = (rnd(rng, N, H, W, F) * 1.5 - 0.2).requires_grad_(True)
        h = rnd(rng, N, H, W, F).requires_grad_(True)
        u, rh = R.gru_plain_gates(pre_g, h)
        u.retain_grad()
        hn = R.gru_plain_out(pre_c, h, u)
        dys = [rnd(rng, N, H, W, F) for _ in range(nio)]
        drh = rnd(rng, N, H, W, F)
        ((hn * sum(dys)).sum() + (rh * drh).sum()).backward()
        _REF[case] = dict(pre_g=pre_g, pre_c=pre_c, h=h, u=u.detach(), du=u.grad, rh=rh.detach(), hn=hn.detach(), dys=dys, drh=drh,
                          dh_garbage=rnd(rng, N, H, W, F))
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
    """The four kernels on one case: every view a strided slice of a wider guarded buffer.  Returns the buffers by name."""
    N, H, W, F, nio = case
    ref = _reference(case)
    Cx = 8
    # the candidate conv's input buffer [x | h | r*h | guard]
    a_slots = [(Cx, F), (Cx + F, F)]
    abuf, (hv, rhv) = _guarded(N, H, W, Cx + 2 * F + 4, a_slots)
    hv.copy_(dev(ref['h'].detach()))
    pgd, pcd = dev(ref['pre_g'].detach()), dev(ref['pre_c'].detach())
    ud = torch.empty(N, H, W, F, device=DEV)
    K.convgru_plain_gates_fwd(pgd, hv, ud, rhv)
    o_slots = [(k * (F + 4), F) for k in range(nio)]
    obuf, outs = _guarded(N, H, W, nio * (F + 4), o_slots)
    K.convgru_plain_out_fwd(pcd, hv, ud, outs)
    dy_slots = [(4 + k * (F + 4), F) for k in range(nio)]
    dybuf, dyv = _guarded(N, H, W, 4 + nio * (F + 4), dy_slots)
    for v, d in zip(dyv, ref['dys']):
        v.copy_(dev(d))
    dhbuf, (dh,) = _guarded(N, H, W, F + 8, [(4, F)])
    dh.copy_(dev(ref['dh_garbage']))                           # out_bwd must overwrite this
    dpc, du = torch.empty(N, H, W, F, device=DEV), torch.empty(N, H, W, F, device=DEV)
    dpg = torch.empty(N, H, W, 2 * F, device=DEV)
    K.convgru_plain_out_bwd(pcd, hv, ud, dyv, dpc, du, dh)
    dh_out = dh.clone()
    drhbuf, (drhv,) = _guarded(N, H, W, F + 8, [(4, F)])
    drhv.copy_(dev(ref['drh']))
    K.convgru_plain_gates_bwd(pgd, hv, du, drhv, dpg, dh)      # ... and this one must add to what out_bwd left
    torch.cuda.synchronize()
    guards = (_untouched(abuf, a_slots) + _untouched(obuf, o_slots) + _untouched(dybuf, dy_slots) + _untouched(dhbuf, [(4, F)])
              + _untouched(drhbuf, [(4, F)]))
    return dict(u=ud, rh=rhv, outs=outs, dpre_c=dpc, du=du, dpre_g=dpg, dh=dh, dh_out=dh_out, guards=guards, h_in=hv)


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'N%d_%dx%dx%d_n%d' % c)
def test_plain_gate_blocks_vs_fp64(case):
    N, H, W, F, nio = case
    ref = _reference(case)
    got = _run_blocks(case)
    res = [('u', rel_err(got['u'], ref['u']), TOL_OP), ('rh', rel_err(got['rh'], ref['rh']), TOL_OP)]
    res += [('h_new%d' % k, rel_err(o, ref['hn']), TOL_OP) for k, o in enumerate(got['outs'])]
    res.append(('h_unchanged', rel_err(got['h_in'], ref['h'].detach().float()), 0.0))
    res.append(('guards', got['guards'], 0.0))
    u, dhp = ref['u'], sum(ref['dys'])
    res.append(('dpre_c', rel_err(got['dpre_c'], ref['pre_c'].grad), TOL_GRAD))
    res.append(('du', rel_err(got['du'], ref['du']), TOL_GRAD))
    res.append(('dh_after_out_bwd(overwritten)', rel_err(got['dh_out'], dhp * u), TOL_GRAD))
    res.append(('dpre_g', rel_err(got['dpre_g'], ref['pre_g'].grad), TOL_GRAD))
    res.append(('dh(accumulated)', rel_err(got['dh'], ref['h'].grad), TOL_GRAD))
    # a second run gives the same bits
    again = _run_blocks(case)
    for nm in ('u', 'rh', 'dpre_c', 'du', 'dpre_g', 'dh'):
        res.append(('bits/' + nm, AUX.bits_equal(got[nm], again[nm]), 0.0))
    res += [('bits/h_new%d' % k, AUX.bits_equal(a, b), 0.0) for k, (a, b) in enumerate(zip(got['outs'], again['outs']))]
    _assert_ok([('convgru_plain_N%d_HW%d_F%d/%s' % (N, H * W, F, n), e, t) for n, e, t in res])


def test_plain_gate_blocks_refuse_what_breaks_float4_access():
    """SAVP_EINVAL for F = 6, for a view whose base is 8 bytes off a 16-byte boundary, and for one whose pixel stride is no multiple of 4."""
    N, HW, F = 1, 16, 8
    pre_g, pre_c = torch.zeros(N, HW, 2 * F, device=DEV), torch.zeros(N, HW, F, device=DEV)
    u, du = torch.zeros(N, HW, F, device=DEV), torch.zeros(N, HW, F, device=DEV)
    wide = torch.zeros(N, HW, F + 4, device=DEV)
    good, off2 = wide[..., 4:], wide[..., 2:2 + F]
    odd = torch.zeros(N, HW, F + 2, device=DEV)[..., :F]
    ok = torch.zeros(N, HW, F, device=DEV)
    res = []
    p6, h6 = torch.zeros(N, HW, 12, device=DEV), torch.zeros(N, HW, 6, device=DEV)
    res.append(('f6/gates_fwd', AUX.refused(lambda: K.convgru_plain_gates_fwd(p6, h6, h6.clone(), h6.clone())), 0.0))
    res.append(('f6/out_fwd', AUX.refused(lambda: K.convgru_plain_out_fwd(h6.clone(), h6, h6.clone(), [h6.clone()])), 0.0))
    for nm, bad in (('base', off2), ('stride', odd)):
        res.append(('%s/gates_fwd_h' % nm, AUX.refused(lambda: K.convgru_plain_gates_fwd(pre_g, bad, u, ok)), 0.0))
        res.append(('%s/gates_fwd_rh' % nm, AUX.refused(lambda: K.convgru_plain_gates_fwd(pre_g, good, u, bad)), 0.0))
        res.append(('%s/out_fwd_dst' % nm, AUX.refused(lambda: K.convgru_plain_out_fwd(pre_c, good, u, [ok, bad])), 0.0))
        res.append(('%s/out_bwd_dy' % nm, AUX.refused(lambda: K.convgru_plain_out_bwd(pre_c, good, u, [bad], ok.clone(), du, ok)), 0.0))
        res.append(('%s/out_bwd_dh' % nm, AUX.refused(lambda: K.convgru_plain_out_bwd(pre_c, good, u, [ok], ok.clone(), du, bad)), 0.0))
        res.append(('%s/gates_bwd_drh' % nm, AUX.refused(lambda: K.convgru_plain_gates_bwd(pre_g, good, du, bad, pre_g.clone(), ok)), 0.0))
        res.append(('%s/gates_bwd_dh' % nm, AUX.refused(lambda: K.convgru_plain_gates_bwd(pre_g, good, du, ok, pre_g.clone(), bad)), 0.0))
    # the aligned twin of the same calls is accepted
    K.convgru_plain_gates_fwd(pre_g, good, u, ok)
    K.convgru_plain_out_fwd(pre_c, good, u, [ok.clone(), wide[..., :F]])
    torch.cuda.synchronize()
    _assert_ok([('convgru_plain_refuse/' + n, e, t) for n, e, t in res])


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: 32 x 32 frames -- GRU planes of 16 x 16, 8 x 8 and 16 x 16 -- against the fp64 oracle, bounds of tests/gpu_model_checks.py
# ---------------------------------------------------------------------------------------------------------------------------------
NONE = dict(conv_rnn='gru', conv_rnn_norm_layer='none')
ABL = dict(conv_rnn='gru', ablation_conv_rnn_norm=True)
MODEL_CASES = [('none', NONE), ('ablation', ABL), ('none_learn_init', dict(NONE, learn_initial_state=True)),
               ('none_flow', dict(NONE, transformation='flow')),
               ('ablation_layer_norm', dict(ABL, norm_layer='layer', conv_rnn_norm_layer='layer'))]
SMALL = dict(B=2, T=5, H=32, W=32, nz=8)


@pytest.mark.parametrize('tag,over', MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_generator_and_train_step_vs_oracle(monkeypatch, tag, over):
    oracle_gru_plain.install(monkeypatch)
    res = MC.check_generator_forward(tag='gen_fwd_gru_' + tag, **SMALL, **over)
    res += MC.check_train_step(steps=1, tag='train_gru_' + tag, **SMALL, **over)
    _assert_ok(res)


def test_bf16_datapath_forward_vs_oracle():
    """The generator on the bf16 datapath against the fp64 oracle with the bounds of gpu_model_checks.check_model_bf16 (5e-2 on every row,
    the argmax rows reported)."""
    K.set_conv_precision('bf16')
    try:
        res = MC.check_generator_forward(tag='bf16_gen_fwd_gru_none', **SMALL, **NONE)
    finally:
        K.set_conv_precision('f32')
    _assert_ok([(n + '(reported)', e, 1.0) if 'argmax' in n else (n, e, 5e-2) for n, e, t in res])


def _train_once(prec, over):
    from video_prediction_amd import variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    B, T, H, W = SMALL['B'], SMALL['T'], SMALL['H'], SMALL['W']
    hp = MC.make_hparams(context_frames=2, sequence_length=T, clip_length=4, nz=SMALL['nz'], lr=2e-4, beta1=0.5, beta2=0.999, l1_weight=100.0,
                         l2_weight=0.0, kl_weight=1.0, kl_anneal='none', video_sn_vae_gan_weight=0.1, video_sn_gan_weight=0.1,
                         vae_gan_feature_cdist_weight=10.0, gan_feature_cdist_weight=0.0, **over)
    vals = V.init_variables(V.variable_specs(hp, (H, W, 3), mode='train'), seed=4)
    rng = np.random.default_rng(9)
    for k in vals:
        if k.endswith('gamma'):
            vals[k] = (1 + 0.2 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('beta') or k.endswith('bias'):
            vals[k] = (0.1 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('kernel') and k.startswith('generator'):
            vals[k] = (vals[k] * 3).astype(np.float32)
    images = MC.synth(hp, B, H, W, 3, 0)
    noise = MC.make_noise(hp, B, seed=100, sampling=True)
    K.set_conv_precision(prec)
    try:
        eng = SAVPEngine(hp, (H, W, 3), B, mode='train', values=vals, device=DEV)
        eng.set_images(images.float().to(DEV), time_major=True)
        return eng, noise
    except Exception:
        K.set_conv_precision('f32')
        raise


def test_bf16_datapath_train_step_tracks_the_fp32_datapath():
    """One train step on the bf16 datapath against the same engine on the exact-fp32 datapath (itself held to the oracle above), with the
    gates of gpu_model_checks.check_action_conditioned_bf16: losses 2e-2 / 6e-2 of max(|ref|, 0.05), frames 5e-2 absolute, per-variable
    gradients 0.25 relative L2 with the 2e-3-of-gmax absolute floor."""
    runs = {}
    for prec in ('f32', 'bf16'):
        try:
            eng, noise = _train_once(prec, NONE)
            info = eng.train_step(noise, return_grads=True)
            torch.cuda.synchronize()
            runs[prec] = (info, eng.gen.gen.v.double().cpu())
        finally:
            K.set_conv_precision('f32')
    (ref, gen_r), (got, gen_g) = runs['f32'], runs['bf16']

    def lrel(a, b):
        return abs(float(a) - float(b)) / max(abs(float(b)), 0.05)
    t = 'bf16_train_gru_none'
    res = [(t + '/d_loss', lrel(got['d_loss'], ref['d_loss']), 2e-2), (t + '/g_loss', lrel(got['g_loss'], ref['g_loss']), 2e-2)]
    for nm, (l, w) in got['g_losses'].items():
        res.append((t + '/' + nm, lrel(l, ref['g_losses'][nm][0]), 6e-2))
    res.append((t + '/gen_images_abs', float((gen_g - gen_r).abs().max()), 5e-2))
    for grp, key in (('d', 'd_grads'), ('g', 'g_grads')):
        gmax = max(float(v.abs().max()) for v in ref[key].values())
        worst, wname = 0.0, ''
        for name, gref in ref[key].items():
            g_ = got[key][name]
            if float(gref.abs().max()) < 1e-9 * gmax:
                e, tol = float(g_.abs().max()) / gmax, 1e-2
            else:
                e, tol = MC._l2rel(g_, gref), 0.25
                if float((g_.double() - gref.double()).abs().max()) <= 2e-3 * gmax:
                    e = min(e, tol)
            if e / tol > worst:
                worst, wname = e / tol, name
        res.append((t + '/%s_grads_worst_err_over_tol[%s]' % (grp, wname.split('/', 1)[-1][-36:]), worst, 1.0))
    _assert_ok(res)


@pytest.mark.parametrize('tag,over', [('none', NONE), ('ablation', ABL)], ids=['none', 'ablation'])
def test_two_eager_train_steps_from_one_state_give_equal_bits(tag, over):
    from tests.test_gpu_soak import _bits, _restore, _state
    eng, noise = _train_once('f32', over)
    s0 = _state(eng)
    outs = []
    for _ in range(2):
        _restore(eng, s0)
        info = eng.train_step(noise, return_grads=True)
        torch.cuda.synchronize()
        o = {'g/' + k: v for k, v in info['g_grads'].items()}
        o.update({'d/' + k: v for k, v in info['d_grads'].items()})
        o['losses'] = torch.stack([info['d_loss'].reshape(()).double(), info['g_loss'].reshape(()).double()]).clone()
        o['gen_images'] = eng.gen.gen.v.clone()
        outs.append(o)
    assert any(k.endswith('conv2dgru_cell/gates/bias') and float(v.abs().max()) > 0 for k, v in outs[0].items())
    bad = [k for k in outs[0] if not torch.equal(_bits(outs[0][k]), _bits(outs[1][k]))]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals that stay
# ---------------------------------------------------------------------------------------------------------------------------------
def test_untiled_latent_and_normaliser_none_ablation_stay_refused():
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = MC.make_hparams(context_frames=2, sequence_length=4, nz=8, where_add='all', use_tile_concat=False, **NONE)
    with pytest.raises(NotImplementedError, match='use_tile_concat=False'):
        SAVPEngine(hp, (32, 32, 3), 2, mode='train', seed=1)
    hp = MC.make_hparams(context_frames=2, sequence_length=4, nz=8, where_add='all', use_tile_concat=False, **ABL)
    with pytest.raises(NotImplementedError, match="conv_rnn='gru'"):
        SAVPEngine(hp, (32, 32, 3), 2, mode='train', seed=1)
    hp = MC.make_hparams(context_frames=2, sequence_length=4, nz=8, ablation_conv_rnn_norm=True, conv_rnn_norm_layer='none', conv_rnn='gru')
    with pytest.raises(TypeError):
        SAVPEngine(hp, (32, 32, 3), 2, mode='train', seed=1)

"""downsample_layer = conv2d, upsample_layer = deconv2d, activation_layer = elu on the HIP path: the ELU code of savp_instnorm_act_* and
savp_groupnorm_act_* and the 'down' / 'deconv' convolution kinds against fp64 autograd, the generator and a train step against the fp64
oracle with the layer-choice extension (tests/oracle_layer_choices.py), bit-reproducibility, hipGraph replay, checkpoints and the scripts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import aux_refs as R
from tests import gpu_checks_aux as AUX
from tests import gpu_model_checks as MC
from tests import oracle_layer_choices as OLC
from tests.bf16_exact import RNE_MISMATCH, TOL_EXACT, bf16_bracket, rne, wgrad_tol
from tests.gpu_checks import TOL_OP
from video_prediction_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL3 = dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu')


def _assert_ok(res):
    for n, e, t in res:
        print('%-90s err %.3e  tol %.3e' % (n, e, t))
    bad = [(n, e, t) for (n, e, t) in res if not (e <= t)]
    assert not bad, 'parity failures (name, err, tol): %r' % bad


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


# ---------------------------------------------------------------------------------------------------------------------------------
# ELU in the fused norm + activation kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def test_instance_norm_elu_every_option_vs_fp64(monkeypatch):
    """tests/gpu_checks_aux.check_inorm_options -- the single-kernel and the coalesced path, the HW boundary, multi-destination outputs with
    channel ranges, bf16 destinations, several dy, dx_beta, a bf16 dx, dgamma / dbeta -- over its own shape list (INORM_CASES) and with its
    own bounds, every case with act = 'elu'."""
    monkeypatch.setattr(AUX, 'INORM_CASES', [(n, h, w, c, 'elu', 0.0) for (n, h, w, c, _, _) in AUX.INORM_CASES])
    act_fn = R.act_fn
    monkeypatch.setattr(R, 'act_fn', lambda act, alpha: OLC.elu if act == 'elu' else act_fn(act, alpha))
    _assert_ok(AUX.check_inorm_options())


def _inputs(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + torch.randn(C, generator=g) * 2 + 0.5).to(DEV)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(C, generator=g)).to(DEV)
    dy = torch.randn(N, H, W, C, generator=g).to(DEV)
    return x, gamma, beta, dy


def _ref(x, gamma, beta, dy, G, eps):
    """fp64 autograd of y = elu(gamma * xhat + beta), statistics per (sample, group of C/G channels); also xhat and dy * elu'(z)."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    g64 = gamma.detach().double().cpu().requires_grad_(True)
    b64 = beta.detach().double().cpu().requires_grad_(True)
    N, C = x.shape[0], x.shape[-1]
    xg = x64.reshape(N, -1, G, C // G)
    m = xg.mean(dim=(1, 3), keepdim=True)
    v = ((xg - m) ** 2).mean(dim=(1, 3), keepdim=True)
    r = torch.rsqrt(v + eps)
    xhat = ((xg - m) * r).reshape(x.shape)
    z = xhat * g64 + b64
    y = torch.nn.functional.elu(z)
    d = dy.detach().double().cpu()
    (y * d).sum().backward()
    dz = d * torch.where(z > 0, torch.ones_like(z), torch.exp(z))
    return dict(y=y.detach(), mean=m.reshape(N, G), rstd=r.reshape(N, G), dx=x64.grad, dgamma=g64.grad, dbeta=b64.grad,
                xhat=xhat.detach(), dz=dz.detach())


@pytest.mark.parametrize('case', AUX.INORM_CASES, ids=lambda c: 'N%d_%dx%dx%d' % c[:4])
def test_layer_norm_elu_fwd_bwd_vs_fp64(case):
    """savp_groupnorm_act_fwd / _bwd with act = 'elu' over the instance-norm option list's shapes (one group: the layer norm), bounds of
    tests/test_gpu_layer_norm.py::test_layer_norm_fwd_bwd_vs_fp64 (:76-77); a bf16 destination and a bf16 dx by bracketing as
    gpu_checks_aux does for the instance norm; a second run gives the same bits."""
    N, H, W, C = case[:4]
    x, gamma, beta, dy = _inputs(N, H, W, C, 3)
    ref = _ref(x, gamma, beta, dy, 1, 1e-12)
    y, y16 = torch.empty_like(x), torch.empty(N, H, W, C, device=DEV, dtype=torch.bfloat16)
    mean, rstd = torch.empty(N, 1, device=DEV), torch.empty(N, 1, device=DEV)
    K.groupnorm_act_fwd(x, gamma, beta, [y, y16], mean, rstd, groups=1, act='elu')
    dx = torch.empty_like(x)
    acc = [torch.zeros(C, device=DEV, dtype=torch.float64) for _ in range(3)]
    K.groupnorm_act_bwd(x, gamma, beta, mean, rstd, [dy], dx, acc[0], acc[1], groups=1, act='elu', dsum=acc[2])
    errs = dict(y=_rel(y, ref['y']), mean=_rel(mean, ref['mean']), rstd=_rel(rstd, ref['rstd']), dx=_rel(dx, ref['dx']),
                dgamma=_rel(acc[0], ref['dgamma']), dbeta=_rel(acc[1], ref['dbeta']))
    print(case, errs)
    assert errs['y'] < 2e-5 and errs['mean'] < 1e-5 and errs['rstd'] < 1e-5
    assert errs['dx'] < 5e-4 and errs['dgamma'] < 5e-4 and errs['dbeta'] < 5e-4
    scale = ref['dx'].abs().sum(dim=(0, 1, 2))
    assert float(((acc[2].cpu() - ref['dx'].sum(dim=(0, 1, 2))).abs() / scale).max()) < 1e-5
    # bf16 destinations: the fp32 value the kernel rounds is within the fp32 rows' bound of the exact one
    n_out, frac = bf16_bracket(y16, ref['y'], atol=2e-5 * float(ref['y'].abs().max()))
    assert n_out == 0 and frac <= RNE_MISMATCH, (n_out, frac)
    dx16 = torch.empty(N, H, W, C, device=DEV, dtype=torch.bfloat16)
    K.groupnorm_act_bwd(x, gamma, beta, mean, rstd, [dy], dx16, torch.zeros_like(acc[0]), torch.zeros_like(acc[1]), groups=1, act='elu')
    n_out, frac = bf16_bracket(dx16, ref['dx'], atol=5e-4 * float(ref['dx'].abs().max()))
    assert n_out == 0, (n_out, frac)
    y2, dx2 = torch.empty_like(x), torch.empty_like(x)
    acc2 = [torch.zeros(C, device=DEV, dtype=torch.float64) for _ in range(2)]
    K.groupnorm_act_fwd(x, gamma, beta, [y2], mean, rstd, groups=1, act='elu')
    K.groupnorm_act_bwd(x, gamma, beta, mean, rstd, [dy], dx2, acc2[0], acc2[1], groups=1, act='elu')
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and torch.equal(acc[0], acc2[0]) and torch.equal(acc[1], acc2[1])


@pytest.mark.parametrize('kind', ['instance', 'layer'])
def test_elu_with_ready_statistics(kind):
    """stats_ready, forward (the producing convolution's per-(sample, channel) sums around a shift) and backward (sum(dy'), sum(dy' * xhat)
    with dy' = dy * elu'(z): what a data-gradient epilogue would leave -- the model takes its own sums for ELU, the entry still honours
    them), two destinations with channel ranges, one of them bf16."""
    N, H, W, C = 4, 16, 16, 64
    x, gamma, beta, dy = _inputs(N, H, W, C, 5)
    G = C if kind == 'instance' else 1
    eps = 1e-6 if kind == 'instance' else 1e-12
    ref = _ref(x, gamma, beta, dy, G, eps)
    shift = (torch.randn(C) * 2).to(DEV)
    xd = (x.double() - shift.double()).reshape(N, -1, C)
    stats = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1).contiguous()
    ya = torch.empty(N, H, W, 32, device=DEV)
    yb = torch.empty(N, H, W, 32, device=DEV, dtype=torch.bfloat16)
    mean, rstd = torch.empty(N, G, device=DEV), torch.empty(N, G, device=DEV)
    kw = dict(act='elu', out_ranges=[(0, 32), (32, 32)], stats=stats, stats_shift=shift)
    if kind == 'instance':
        K.instnorm_act_fwd(x, gamma, beta, [ya, yb], mean, rstd, eps=eps, **kw)
    else:
        K.groupnorm_act_fwd(x, gamma, beta, [ya, yb], mean, rstd, groups=1, **kw)
    assert _rel(ya, ref['y'][..., 0:32]) < 2e-5 and _rel(mean, ref['mean']) < 1e-5 and _rel(rstd, ref['rstd']) < 1e-5
    n_out, frac = bf16_bracket(yb, ref['y'][..., 32:], atol=2e-5 * float(ref['y'].abs().max()))
    assert n_out == 0 and frac <= RNE_MISMATCH, (n_out, frac)
    bst = torch.stack([ref['dz'].reshape(N, -1, C).sum(1), (ref['dz'] * ref['xhat']).reshape(N, -1, C).sum(1)], dim=-1).contiguous().to(DEV)
    dx = torch.empty_like(x)
    dg, db = torch.zeros(C, device=DEV, dtype=torch.float64), torch.zeros(C, device=DEV, dtype=torch.float64)
    if kind == 'instance':
        K.instnorm_act_bwd(x, gamma, beta, None, mean, rstd, [dy], dx, dg, db, act='elu', eps=eps, stats=bst)
    else:
        K.groupnorm_act_bwd(x, gamma, beta, mean, rstd, [dy], dx, dg, db, groups=1, act='elu', stats=bst)
    assert _rel(dx, ref['dx']) < 5e-4 and _rel(dg, ref['dgamma']) < 5e-4 and _rel(db, ref['dbeta']) < 5e-4


def test_the_conv_epilogue_refuses_elu_norm_backward_sums():
    """SavpConvArgs.nb_act knows the 0 / 1 / alpha masks; for an ELU norm the plan query says no (the model then takes the un-fused path).
    The 3x3 head shape of tests/gpu_checks.check_norm_bwd_stats_epilogue ('head64'), which that check requires to be offered for ReLU."""
    from video_prediction_amd import lib
    N, H, C, Cout = 2, 64, 32, 64
    geom = K.ConvGeom((1, 3, 3), (1, 1, 1), (0, 1, 1))
    dx = torch.zeros(N, H, H, C, device=DEV)
    dy = torch.zeros(N, H, H, Cout, device=DEV, dtype=torch.bfloat16)
    wd = torch.zeros(C, 9 * Cout, device=DEV)
    wd16 = wd.to(torch.bfloat16)
    nb = dict(x=torch.zeros(N, H, H, C, device=DEV), mean=torch.zeros(N, C, device=DEV), rstd=torch.ones(N, C, device=DEV),
              gamma=torch.ones(C, device=DEV), beta=torch.zeros(C, device=DEV), c0=0)
    prev = K.PRECISION['value']
    K.set_conv_precision('bf16')
    try:
        assert K.conv_stats_ok(lib.CONV_DGRAD, geom, dx, dy, wd, w16=wd16, norm_bwd=dict(nb, act='relu'))
        assert not K.conv_stats_ok(lib.CONV_DGRAD, geom, dx, dy, wd, w16=wd16, norm_bwd=dict(nb, act='elu'))
    finally:
        K.PRECISION['value'] = prev


# ---------------------------------------------------------------------------------------------------------------------------------
# the stride-2 SAME convolution ('down') and its transpose ('deconv')
# ---------------------------------------------------------------------------------------------------------------------------------
def _layer(kind, W, b, hw):
    from video_prediction_amd.engine import ConvLayer, _TensorStore, same_pad_before
    st = _TensorStore({'k': W, 'b': b}, {'k': torch.zeros_like(W), 'b': torch.zeros_like(b)})
    k = W.shape[0]
    L = ConvLayer(st, 'k', 'b', kind, (k, k), (2, 2), (same_pad_before(k + 1, 2, hw[0]), same_pad_before(k + 1, 2, hw[1])))
    L.prep()
    return L


def _same_conv64(x, w, b):
    from oracle import ops
    return ops.conv2d(x, w, b, strides=(2, 2))


# N, hi-res H, W, channels at the hi-res side, channels at the lo-res side, k: the ladder of c2 (64 x 64, ngf 32) and one odd plane ratio
CONV_SHAPES = [(2, 64, 64, 16, 32, 5), (2, 32, 32, 32, 64, 3), (2, 16, 16, 64, 128, 3), (3, 16, 24, 8, 24, 3)]


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'N%d_%dx%d_%dto%d_k%d' % s)
def test_strided_conv_and_deconv_vs_fp64(shape, prec):
    """downsample conv2d (forward, data gradient, weight and bias gradient) and deconv2d with the same kernel read as [k, k, F, Cin]
    (forward = that data gradient, data gradient = that forward, weight gradient with the roles swapped) against fp64 -- on the bf16
    datapath against fp64 of the bf16-rounded operands (tests/bf16_exact.py: only the fp32 accumulation is left, so the fp32 bounds hold)."""
    N, H, Wd, Chi, Clo, k = shape
    g = torch.Generator().manual_seed(17)
    x = torch.randn(N, H, Wd, Chi, generator=g).to(DEV)                    # hi-res side
    yl = torch.randn(N, H // 2, Wd // 2, Clo, generator=g).to(DEV)         # lo-res side
    w = (0.1 * torch.randn(k, k, Chi, Clo, generator=g)).to(DEV)
    b_lo, b_hi = (0.1 * torch.randn(Clo, generator=g)).to(DEV), (0.1 * torch.randn(Chi, generator=g)).to(DEV)
    q = rne if prec == 'bf16' else (lambda t: t)
    tol = TOL_EXACT if prec == 'bf16' else TOL_OP
    wtol = wgrad_tol(N, 1, H // 2, Wd // 2)
    x64 = q(x).double().cpu().requires_grad_(True)
    w64 = q(w).double().cpu().requires_grad_(True)
    y64 = _same_conv64(x64, w64, b_lo.double().cpu())
    (y64 * q(yl).double().cpu()).sum().backward()
    prev = K.PRECISION['value']
    K.set_conv_precision(prec)
    try:
        res = []
        # conv2d, strides 2, SAME
        L = _layer('down', w, b_lo, (H, Wd))
        y = torch.empty(N, H // 2, Wd // 2, Clo, device=DEV)
        L.forward(x, y)
        res.append(('down/fwd', _rel(y, y64), tol))
        dx = torch.empty_like(x)
        L.backward_data(yl, dx, beta=0)
        res.append(('down/dgrad', _rel(dx, x64.grad), tol))
        L.backward_weights(x, yl)
        L.finish_weight_grad()
        res.append(('down/wgrad', _rel(L.dW, w64.grad), wtol))
        res.append(('down/bias_grad', _rel(L.dbias, yl.double().sum(dim=(0, 1, 2))), wtol))
        # deconv2d: kernel [k, k, F = Chi, Cin = Clo]
        D = _layer('deconv', w, b_hi, (H, Wd))
        up = torch.empty(N, H, Wd, Chi, device=DEV)
        D.forward(yl, up)
        res.append(('deconv/fwd', _rel(up, x64.grad + b_hi.double().cpu()), tol))
        dlo = torch.empty_like(yl)
        D.backward_data(x, dlo, beta=0)
        res.append(('deconv/dgrad', _rel(dlo, y64.detach() - b_lo.double().cpu()), tol))
        D.backward_weights(yl, x)
        D.finish_weight_grad()
        res.append(('deconv/wgrad', _rel(D.dW, w64.grad), wtol))
        res.append(('deconv/bias_grad', _rel(D.dbias, x.double().sum(dim=(0, 1, 2))), wtol))
        torch.cuda.synchronize()
    finally:
        K.PRECISION['value'] = prev
    _assert_ok([(('%s/' % prec) + n, e, t) for n, e, t in res])


def test_fold_embed_round_trip_and_adjoint_accumulates():
    for k, a, b in ((3, 8, 16), (5, 6, 4)):
        w = torch.randn(k, k, a, b, device=DEV)
        wf = torch.full((k + 1, k + 1, a, b), 7.0, device=DEV)
        K.fold_embed(w, wf, k)
        assert torch.equal(wf[1:, 1:], w) and float(wf[0].abs().max()) == 0.0 and float(wf[:, 0].abs().max()) == 0.0
        acc = torch.ones_like(w)
        K.fold_embed(wf, acc, k, adjoint=True)
        assert torch.equal(acc, w + 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: generator outputs and one train step (losses, every gradient, variables after Adam) against the extended oracle, with the
# bounds tests/gpu_model_checks.py applies to the default layers (check_generator_forward :111-139, check_train_step :193-232)
# ---------------------------------------------------------------------------------------------------------------------------------
SWITCHES = [('conv2d', dict(downsample_layer='conv2d')), ('deconv2d', dict(upsample_layer='deconv2d')), ('elu', dict(activation_layer='elu')),
            ('all_three', ALL3)]


@pytest.mark.parametrize('norm', ['instance', 'layer'])
@pytest.mark.parametrize('tag,over', SWITCHES, ids=[c[0] for c in SWITCHES])
def test_generator_and_train_step_vs_oracle(monkeypatch, tag, over, norm):
    OLC.install(monkeypatch)
    over = dict(over, norm_layer=norm)
    res = MC.check_generator_forward(nz=8, B=2, T=5, tag='gen_fwd_%s_%s' % (tag, norm), **over)
    res += MC.check_train_step(B=2, T=5, nz=8, steps=1, tag='train_%s_%s' % (tag, norm), **over)
    _assert_ok(res)


COMBOS = [('gru', dict(conv_rnn='gru')), ('ablation_rnn', dict(ablation_rnn=True)), ('untiled', dict(use_tile_concat=False)),
          ('where_add_input', dict(where_add='input')), ('where_add_middle', dict(where_add='middle')),
          ('layer_layer', dict(norm_layer='layer', conv_rnn_norm_layer='layer')), ('flow', dict(transformation='flow')),
          ('v2_names', dict(downsample_layer='conv_pool2d_v2', upsample_layer='upsample_conv2d_v2', activation_layer='relu'))]


# The untiled latent's train step runs without the discriminators, as the default layers' own parity row does (gpu_model_checks.py:437
# 'train_untiled_latent').  With them the video discriminator's first kernel gradient misses check_train_step's bound with the DEFAULT
# layers as much as with the new ones (measured in one run: excess 2.054 default layers, 2.051 all three; 0.05 with the tiled latent) -- a
# property of that configuration's discriminator step, which this feature does not touch.
NO_D = dict(video_sn_vae_gan_weight=0.0, video_sn_gan_weight=0.0, vae_gan_feature_cdist_weight=0.0)


@pytest.mark.parametrize('tag,over', COMBOS, ids=[c[0] for c in COMBOS])
def test_all_three_in_combination_vs_oracle(monkeypatch, tag, over):
    OLC.install(monkeypatch)
    over = dict(ALL3, **over)
    res = MC.check_generator_forward(nz=8, B=2, T=5, tag='gen_fwd_all3_' + tag, **over)
    res += MC.check_train_step(B=2, T=5, nz=8, steps=1, tag='train_all3_' + tag, **dict(over, **(NO_D if tag == 'untiled' else {})))
    _assert_ok(res)


def test_unknown_values_and_unbuildable_combinations_raise():
    from video_prediction_amd.models.savp_model import SAVPEngine
    for over, exc in ((dict(downsample_layer='max_pool'), ValueError), (dict(upsample_layer='nearest'), ValueError),
                      (dict(activation_layer='gelu'), ValueError),
                      (dict(ALL3, norm_layer='layer', use_tile_concat=False), NotImplementedError),
                      (dict(ALL3, conv_rnn='gru', conv_rnn_norm_layer='layer'), NotImplementedError)):
        hp = MC.make_hparams(context_frames=2, sequence_length=4, nz=8, **over)
        with pytest.raises(exc):
            SAVPEngine(hp, (64, 64, 3), 2, mode='train', seed=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 datapath, reproducibility, hipGraph replay
# ---------------------------------------------------------------------------------------------------------------------------------
def _c2_engine(graph, **over):
    """The c2-shaped step (B = 16, T = 30, the ours_savp recipe, bf16 datapath, shipped tuning table) with the given switches."""
    from video_prediction_amd import variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    case = MC.BENCH_CASES['c2']
    hp, _, images, noise = MC.recipe_case(**case)
    hp.override_from_dict(over)
    vals = V.init_variables(V.variable_specs(hp, (64, 64, 3), mode='train'), seed=4)
    K.set_conv_precision('bf16')
    K.enable_autotune(True)
    K.load_tuning(os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json'))
    eng = SAVPEngine(hp, (64, 64, 3), case['B'], mode='train', values=vals, device=DEV)
    eng.use_graph = graph
    eng.set_images(images.float().cuda(), time_major=True)
    return eng, noise


@pytest.mark.parametrize('norm', ['instance', 'layer'])
def test_c2_bf16_step_repeats_bit_identically_eager_and_replayed(norm):
    """As tests/test_gpu_soak.py for the default model, with the three switches: from one state, 3 eager repeats in one engine and 3
    replayed ones (after the eager and the capturing step) in another give the same bits in the generated frames, the losses, every
    variable, both Adam moments and the spectral-norm vectors -- so two runs agree, and replayed equals eager."""
    import gc
    from tests.test_gpu_soak import _bits, _restore, _state
    saved = dict(K.AUTOTUNE, cache=dict(K.AUTOTUNE['cache']))
    ref, bad = None, []
    try:
        for graph in (False, True):
            eng, noise = _c2_engine(graph, **dict(ALL3, norm_layer=norm))
            s0 = _state(eng)
            for rep in range(3 + (2 if graph else 0)):
                _restore(eng, s0)
                info = eng.train_step(noise)
                torch.cuda.synchronize()
                if graph and rep >= 1:
                    assert eng.graph is not None
                out = _state(eng)
                out['gen_images'] = eng.gen.gen.v.clone()
                out['losses'] = torch.stack([info['d_loss'].reshape(()).double(), info['g_loss'].reshape(()).double()]).clone()
                assert all(bool(torch.isfinite(v.float()).all()) for v in out.values())
                if ref is None:
                    ref = out
                else:
                    bad += [('replayed' if graph else 'eager', rep, k) for k in out if not torch.equal(_bits(out[k]), _bits(ref[k]))]
            del eng, s0
            gc.collect()
            torch.cuda.empty_cache()
        assert not bad, bad
    finally:
        K.set_conv_precision('f32')
        K.AUTOTUNE.update(enabled=saved['enabled'], cache=saved['cache'])


def _small_losses(monkeypatch, prec, **over):
    from video_prediction_amd.models.savp_model import SAVPEngine
    monkeypatch.setenv('SAVP_GRAPH', '0')
    prev = K.PRECISION['value']
    K.set_conv_precision(prec)
    try:
        hp = MC.make_hparams(context_frames=2, sequence_length=12, nz=8, lr=1e-3, beta1=0.5, l1_weight=100.0, kl_weight=1.0,
                             video_sn_gan_weight=0.1, video_sn_vae_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0, **over)
        eng = SAVPEngine(hp, (64, 64, 3), 2, mode='train', seed=4)
        g = torch.Generator().manual_seed(3)
        eng.set_images(torch.rand(12, 2, 64, 64, 3, generator=g).cuda(), time_major=True)
        info = eng.train_step()
        torch.cuda.synchronize()
        return float(info['d_loss']), float(info['g_loss'])
    finally:
        K.PRECISION['value'] = prev


@pytest.mark.parametrize('tag,over', SWITCHES, ids=[c[0] for c in SWITCHES])
def test_bf16_datapath_first_step_tracks_the_fp32_datapath(monkeypatch, tag, over):
    """Bounds of tests/test_gpu_layer_norm.py::test_bf16_datapath_train_steps_track_the_fp32_datapath (:283-285)."""
    d32, g32 = _small_losses(monkeypatch, 'f32', **over)
    d16, g16 = _small_losses(monkeypatch, 'bf16', **over)
    print(tag, (d32, g32), (d16, g16))
    assert np.isfinite(d16) and np.isfinite(g16)
    assert abs(g16 - g32) <= 2e-2 * abs(g32) and abs(d16 - d32) <= 5e-2 * max(1.0, abs(d32))


# ---------------------------------------------------------------------------------------------------------------------------------
# checkpoints and scripts
# ---------------------------------------------------------------------------------------------------------------------------------
def test_model_class_trains_generates_and_checkpoints_with_the_new_names(tmp_path):
    from video_prediction_amd.checkpoint import read_checkpoint
    from video_prediction_amd.models import get_model_class
    Model = get_model_class('savp')
    hp = dict(context_frames=2, sequence_length=5, nz=8, **ALL3)
    images = torch.rand(2, 5, 64, 64, 3).cuda()
    a = Model(mode='train', hparams_dict=hp)
    a.build_graph({'images': images})
    a.engine.set_images(images)
    for _ in range(2):
        info = a.engine.train_step()
        assert np.isfinite(float(info['g_loss']))
    a.save(str(tmp_path / 'model-2'))
    ck = read_checkpoint(str(tmp_path / 'model-2'))
    p = 'generator/rnn/savp_cell/'
    assert tuple(ck[p + 'h0/conv2d/kernel'].shape)[:2] == (5, 5) and tuple(ck[p + 'h1/conv2d/kernel'].shape)[:2] == (3, 3)
    assert tuple(ck[p + 'h3/deconv2d/kernel'].shape)[:3] == (3, 3, 64) and tuple(ck[p + 'h3/deconv2d/bias'].shape) == (64,)
    assert not any('conv_pool2d' in k or 'upsample_conv2d' in k for k in ck)
    b = Model(mode='test', hparams_dict=hp)
    b.build_graph({'images': images})
    b.restore(str(tmp_path))
    for n in b.engine.store.names():
        assert torch.equal(a.engine.store[n], b.engine.store[n]), n
    b.engine.set_images(images)
    gen = b.engine.generate(b.engine.default_noise())
    assert torch.isfinite(gen).all()


def test_train_and_generate_scripts_with_the_three_switches(tmp_path):
    out = str(tmp_path / 'run')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'train.py'), '--input_dir', 'none', '--dataset', 'synthetic',
                        '--model', 'savp', '--output_dir', out, '--progress_freq', '1', '--summary_freq', '2', '--eval_summary_freq', '0',
                        '--save_freq', '2', '--dataset_hparams', 'sequence_length=12',
                        '--model_hparams', 'batch_size=2,max_steps=2,downsample_layer=conv2d,upsample_layer=deconv2d,activation_layer=elu'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'progress  global step 2' in r.stdout and os.path.exists(os.path.join(out, 'model-2.index'))
    res = str(tmp_path / 'results')
    # no --model_hparams: the three switches come from the checkpoint's model_hparams.json
    g = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'generate.py'), '--input_dir', 'none', '--dataset', 'synthetic',
                        '--checkpoint', out, '--results_dir', res, '--batch_size', '2', '--num_samples', '2', '--num_stochastic_samples', '1',
                        '--dataset_hparams', 'sequence_length=12'], capture_output=True, text=True, timeout=600)
    assert g.returncode == 0, g.stdout[-2000:] + g.stderr[-2000:]
    pngs = [f for f in os.listdir(os.path.join(res, 'run')) if f.endswith('.png')]
    assert len(pngs) == 2 * 1 * 10

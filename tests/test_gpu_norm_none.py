"""norm_layer = 'none' on the HIP path: savp_plain_act_fwd / _bwd (csrc/plain_act.hip) against fp64 autograd of act(x + add), and the
generator, a train step, the bf16 datapath, determinism, hipGraph replay and the model class against the fp64 oracle (oracle/savp.py takes
norm_layer = 'none' as it stands).  The bounds are those of tests/test_gpu_layer_norm.py for the same quantities."""
import numpy as np
import pytest
import torch

from tests import gpu_model_checks as MC
from tests import oracle_layer_choices as OLC
from tests import oracle_layer_norm as OLN
from video_prediction_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    """norm_layer = 'none' is opt-in on the HIP path (SAVP_NORM_NONE=1 or the keyword norm_none=True); every engine below is built with it."""
    monkeypatch.setenv('SAVP_NORM_NONE', '1')


ACTS = [('none', 0.0), ('relu', 0.0), ('lrelu', 0.2), ('elu', 0.0)]


def _assert_ok(res):
    bad = [(n, e, t) for (n, e, t) in res if not (e <= t)]
    assert not bad, 'parity failures (name, err, tol): %r' % bad


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _act64(z, act, alpha):
    F = torch.nn.functional
    return {'none': lambda t: t, 'relu': torch.relu, 'lrelu': lambda t: F.leaky_relu(t, alpha), 'elu': F.elu}[act](z)


def _ref(x, add, dy, act, alpha):
    """fp64 autograd of y = act(x + add[:, None, None, :]): (y, dx, dadd)."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    a64 = add.detach().double().cpu().requires_grad_(True) if add is not None else None
    z = x64 if a64 is None else x64 + a64[:, None, None, :]
    y = _act64(z, act, alpha)
    (y * dy.detach().double().cpu()).sum().backward()
    return y.detach(), x64.grad, (a64.grad if a64 is not None else None)


def _inputs(N, H, W, C, seed, add=True):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, H, W, C, generator=g) * 1.5 + torch.randn(C, generator=g) * 0.5).to(DEV)
    a = (torch.randn(N, C, generator=g)).to(DEV) if add else None
    dy = torch.randn(N, H, W, C, generator=g).to(DEV)
    return x, a, dy


def _psum_err(psum, rdx):
    """Per (sample, channel) entry, against the size of what was summed (the sums cancel: relative to the sum itself would be ill-conditioned)."""
    N, C = psum.shape
    r = rdx.reshape(N, -1, C)
    return float(((psum.cpu() - r.sum(1)).abs() / r.abs().sum(1).clamp_min(1e-30)).max())


# (N, H, W, C): a single pixel; an odd plane with C no power of two; C % 4 != 0 (the scalar instantiation); several pixel chunks per plane;
# and, beyond the issue's list, the two widths at which a plane's columns no longer fit one workgroup (more than 256 float4 columns, more
# than 256 scalar columns: a second column block, its last one partly empty)
SHAPES = [(1, 1, 1, 8), (3, 5, 7, 24), (2, 3, 3, 5), (2, 8, 8, 128), (2, 16, 16, 96), (1, 2, 3, 1028), (2, 2, 2, 259)]


@pytest.mark.parametrize('with_add', [False, True], ids=['plain', 'add'])
@pytest.mark.parametrize('act,alpha', ACTS, ids=[a for a, _ in ACTS])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_plain_act_fwd_bwd_vs_fp64(shape, act, alpha, with_add):
    N, H, W, C = shape
    x, add, dy = _inputs(N, H, W, C, 3, with_add)
    y = torch.empty_like(x)
    K.plain_act_fwd(x, add, [y], act=act, alpha=alpha)
    dx = torch.empty_like(x)
    psum = torch.zeros(N, C, device=DEV, dtype=torch.float64)
    K.plain_act_bwd(x, add, [dy], dx, act=act, alpha=alpha, psum=psum)
    ry, rdx, radd = _ref(x, add, dy, act, alpha)
    ey, edx, eps_ = _rel(y, ry), _rel(dx, rdx), _psum_err(psum, rdx)
    print('plain_act %s %s add=%s: y %.2e dx %.2e psum %.2e' % (shape, act, with_add, ey, edx, eps_))
    assert ey < 2e-5 and edx < 5e-4 and eps_ < 1e-5
    if with_add:          # the rows of psum ARE the gradient of add
        assert float(((psum.cpu() - radd).abs() / rdx.reshape(N, -1, C).abs().sum(1).clamp_min(1e-30)).max()) < 1e-5
    # psum is an accumulator: a second call adds the same sums again
    K.plain_act_bwd(x, add, [dy], torch.empty_like(x), act=act, alpha=alpha, psum=psum)
    assert _psum_err(psum / 2, rdx) < 1e-5


@pytest.mark.parametrize('off', [8, 3], ids=['aligned_slice', 'unaligned_slice'])
def test_two_destinations_with_channel_ranges_one_bf16_one_a_slice_of_a_wider_buffer(off):
    """Destination 0: channels [0, 32) into channels [off, off + 32) of a 48-channel buffer whose other channels must stay untouched
    (off = 3: no 16-byte alignment, the scalar instantiation); destination 1: channels [32, 64) as bf16."""
    N, H, W, C = 3, 5, 7, 64
    x, add, dy = _inputs(N, H, W, C, 5)
    wide = torch.full((N, H, W, 48), -7.25, device=DEV)
    yb = torch.empty(N, H, W, 32, device=DEV, dtype=torch.bfloat16)
    K.plain_act_fwd(x, add, [wide[..., off:off + 32], yb], act='relu', out_ranges=[(0, 32), (32, 32)])
    ry, _, _ = _ref(x, add, dy, 'relu', 0.0)
    assert _rel(wide[..., off:off + 32], ry[..., 0:32]) < 2e-5 and _rel(yb.float(), ry[..., 32:]) < 8e-3
    assert bool((wide[..., :off] == -7.25).all()) and bool((wide[..., off + 32:] == -7.25).all())


def test_two_gradient_views_with_ranges_and_an_accumulated_dx():
    N, H, W, C = 3, 5, 7, 64
    x, add, dy = _inputs(N, H, W, C, 6)
    _, rdx, _ = _ref(x, add, dy, 'lrelu', 0.2)
    # two dys with ranges: views into two different buffers
    da = torch.zeros(N, H, W, 40, device=DEV)
    da[..., 8:40] = dy[..., 0:32]
    db = dy[..., 32:].contiguous()
    dx = torch.empty_like(x)
    K.plain_act_bwd(x, add, [da[..., 8:40], db], dx, act='lrelu', alpha=0.2, dy_ranges=[(0, 32), (32, 32)])
    assert _rel(dx, rdx) < 5e-4
    # two overlapping gradients are summed
    dx2 = torch.empty_like(x)
    K.plain_act_bwd(x, add, [dy, dy], dx2, act='lrelu', alpha=0.2)
    assert _rel(dx2, 2 * rdx) < 5e-4
    # dx_beta = 1 adds to what dx holds; the column sums stay those of this call's gradient
    base = torch.randn(N, H, W, C, device=DEV)
    dx3 = base.clone()
    psum = torch.zeros(N, C, device=DEV, dtype=torch.float64)
    K.plain_act_bwd(x, add, [dy], dx3, act='lrelu', alpha=0.2, dx_beta=1, psum=psum)
    assert _rel(dx3 - base, rdx) < 5e-4 and _psum_err(psum, rdx) < 1e-5


@pytest.mark.parametrize('shape', [(2, 16, 16, 96), (2, 3, 3, 5)], ids=['vector', 'scalar'])
def test_bf16_dx_keeps_the_fp32_column_sums_and_a_second_run_gives_the_same_bits(shape):
    N, H, W, C = shape
    x, add, dy = _inputs(N, H, W, C, 7)
    _, rdx, _ = _ref(x, add, dy, 'relu', 0.0)
    dx32, dx16 = torch.empty_like(x), torch.empty(N, H, W, C, device=DEV, dtype=torch.bfloat16)
    p32, p16 = (torch.zeros(N, C, device=DEV, dtype=torch.float64) for _ in range(2))
    K.plain_act_bwd(x, add, [dy], dx32, act='relu', psum=p32)
    K.plain_act_bwd(x, add, [dy], dx16, act='relu', psum=p16)
    assert _rel(dx16.float(), rdx) < 8e-3 and _psum_err(p16, rdx) < 1e-5
    assert torch.equal(p16, p32)                 # taken before the rounding: the very sums of the fp32 run
    assert torch.equal(dx16, dx32.to(torch.bfloat16))
    # deterministic: a second run gives the same bits, outputs and sums alike
    y1, y2 = torch.empty_like(x), torch.empty_like(x)
    K.plain_act_fwd(x, add, [y1], act='elu')
    K.plain_act_fwd(x, add, [y2], act='elu')
    dxb, pb = torch.empty_like(x), torch.zeros(N, C, device=DEV, dtype=torch.float64)
    K.plain_act_bwd(x, add, [dy], dxb, act='relu', psum=pb)
    assert torch.equal(y1, y2) and torch.equal(dxb, dx32) and torch.equal(pb, p32)


def test_relu_gradient_is_zero_where_the_input_is_exactly_zero():
    N, H, W, C = 2, 4, 4, 8
    x, _, dy = _inputs(N, H, W, C, 8, add=False)
    x[:, ::2, :, ::3] = 0.0
    add = torch.zeros(N, C, device=DEV)
    add[1, 1] = 0.5
    x[1, 1, 1, 1] = -0.5                         # x + add == 0 exactly
    dx = torch.empty_like(x)
    K.plain_act_bwd(x, add, [dy], dx, act='relu')
    _, rdx, _ = _ref(x, add, dy, 'relu', 0.0)          # torch.relu: gradient 0 at 0
    zero = (x + add[:, None, None, :]) == 0
    assert int(zero.sum()) > 32 and bool((dx[zero] == 0).all()) and _rel(dx, rdx) < 5e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------
NN = dict(norm_layer='none')
CASES = [('alone', {}),
         ('cell_none', dict(conv_rnn_norm_layer='none')),
         ('gru', dict(conv_rnn='gru')),
         ('abl_rnn', dict(ablation_rnn=True)),
         ('flow', dict(transformation='flow')),
         ('prior', dict(learn_prior=True, use_e_rnn=True)),
         ('untiled', dict(use_tile_concat=False)),
         ('untiled_middle', dict(use_tile_concat=False, where_add='middle')),
         ('cell_layer', dict(conv_rnn_norm_layer='layer')),
         # tests/oracle_layer_choices.norm_act hands norm_layer = 'none' through unchanged (elu(h) with no norm in front)
         ('elu', dict(activation_layer='elu'))]


@pytest.mark.parametrize('tag,over', CASES, ids=[c[0] for c in CASES])
def test_generator_and_train_step_vs_oracle(monkeypatch, tag, over):
    if tag == 'cell_layer':
        OLN.install(monkeypatch)
    if tag == 'elu':
        OLC.install(monkeypatch)
    res = MC.check_generator_forward(nz=8, B=2, T=5, tag='gen_fwd_nn_' + tag, **NN, **over)
    res += MC.check_train_step(B=2, T=5, nz=8, steps=1, tag='train_nn_' + tag, **NN, **over)
    _assert_ok(res)


def test_kth_shape_generator_and_train_step_vs_oracle():
    res = MC.check_generator_forward(nz=8, B=2, T=5, C=1, tag='gen_fwd_nn_kth', **NN)
    res += MC.check_train_step(B=2, T=5, C=1, nz=8, steps=1, tag='train_nn_kth', **NN)
    _assert_ok(res)


def _engine_and_noise(mode='test', T=5, **over):
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = MC.make_hparams(context_frames=2, sequence_length=T, nz=8, clip_length=4, **NN, **over)
    eng = SAVPEngine(hp, (64, 64, 3), 2, mode=mode, seed=4)
    eng.set_images(MC.synth(hp, 2, 64, 64, 3, 0).float().to(DEV), time_major=True)
    return hp, eng


def test_the_untiled_latent_is_live():
    """use_tile_concat=False without a normaliser: dense(z) survives (an instance norm would cancel it, tests/test_untiled_latent_is_
    cancelled.py), so the frames depend on z and h0/dense/kernel has a gradient.  That the gradient is the oracle's, inside
    check_train_step's bound, is test_generator_and_train_step_vs_oracle[untiled]: its worst-over-all-variables figure covers this
    variable with the relative check, because a non-zero gradient here against a zero one there would fail the absolute one."""
    hp, eng = _engine_and_noise(use_tile_concat=False)
    eng.mode = 'train'
    eng.prep_generator_weights()
    noise = MC.make_noise(hp, 2, seed=1)
    g1 = eng.forward_generator(noise).clone()
    other = dict(noise, eps=noise['eps'] + 1.0, prior=noise['prior'] - 1.0)
    g2 = eng.forward_generator(other).clone()
    assert float((g1 - g2).abs().max()) > 1e-4
    g3 = eng.forward_generator(noise)
    assert torch.equal(g1, g3)
    hp, tr = _engine_and_noise(mode='train', use_tile_concat=False)
    info = tr.train_step(MC.make_noise(hp, 2, seed=100), return_grads=True)
    grads = info['g_grads']
    gmax = max(float(v.abs().max()) for v in grads.values())
    for name in ('generator/rnn/savp_cell/h0/dense/kernel', 'generator/rnn/savp_cell/h5/dense/kernel'):
        assert float(grads[name].abs().max()) > 1e-6 * gmax, (name, float(grads[name].abs().max()), gmax)


def test_bf16_datapath_ladder_bias_gradients_track_the_fp32_datapath():
    """One train step on the bf16 datapath against the SAME engine on the exact-fp32 datapath from identical variables, inputs and noise
    (as tests/gpu_model_checks.check_action_conditioned_bf16 runs the two).  On the bf16 datapath the ladder convolutions' output
    gradients are bf16 and their weight-gradient pass takes no bias gradient: it comes from savp_plain_act_bwd's float64 column sums.
    Bound: the bf16 arm's per-variable gradient gate there, 0.25 in relative L2 -- here without its absolute floor (a missing bias
    gradient, all zeros, is a relative error of 1)."""
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = MC.make_hparams(context_frames=2, sequence_length=5, clip_length=4, nz=8, lr=2e-4, beta1=0.5, beta2=0.999, l1_weight=100.0,
                         l2_weight=0.0, kl_weight=1.0, kl_anneal='none', video_sn_vae_gan_weight=0.1, video_sn_gan_weight=0.1,
                         vae_gan_feature_cdist_weight=10.0, gan_feature_cdist_weight=0.0, **NN)
    from video_prediction_amd import variables as V
    vals = V.init_variables(V.variable_specs(hp, (64, 64, 3), mode='train'), seed=4)
    rng = np.random.default_rng(9)
    for k in vals:
        if k.endswith('bias'):
            vals[k] = (0.1 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('kernel') and k.startswith('generator'):
            vals[k] = (vals[k] * 3).astype(np.float32)
    images = MC.synth(hp, 2, 64, 64, 3, 0).float().to(DEV)
    noise = MC.make_noise(hp, 2, seed=100)
    runs = {}
    for prec in ('f32', 'bf16'):
        K.set_conv_precision(prec)
        try:
            eng = SAVPEngine(hp, (64, 64, 3), 2, mode='train', values=vals, device=DEV)
            eng.set_images(images, time_major=True)
            runs[prec] = eng.train_step(noise, return_grads=True)
            torch.cuda.synchronize()
            if prec == 'bf16':          # the path under test is taken: bf16 output gradients at the ladder
                assert eng.gen.layers[0]['pre'].g.dtype == torch.bfloat16 and eng.gen.heads_pre.g.dtype == torch.bfloat16
        finally:
            K.set_conv_precision('f32')
    ref, got = runs['f32']['g_grads'], runs['bf16']['g_grads']
    assert np.isfinite(float(runs['bf16']['g_loss']))
    p = 'generator/rnn/savp_cell/'
    names = [p + 'h%d/%s/bias' % (i, 'conv_pool2d' if i < 3 else 'upsample_conv2d') for i in range(6)] + \
            [p + 'h6_masks/conv2d/bias', p + 'h6_scratch/conv2d/bias']
    errs = {n: MC._l2rel(got[n], ref[n]) for n in names}
    print('bf16 vs fp32 bias gradients (relative L2):', errs)
    assert all(float(ref[n].abs().max()) > 0 for n in names)
    assert max(errs.values()) <= 0.25, errs


# ---------------------------------------------------------------------------------------------------------------------------------
# determinism, hipGraph replay, model class
# ---------------------------------------------------------------------------------------------------------------------------------
def _engine(monkeypatch, graph, seed=4):
    from video_prediction_amd.models.savp_model import SAVPEngine
    monkeypatch.setenv('SAVP_GRAPH', '1' if graph else '0')
    hp = MC.make_hparams(context_frames=2, sequence_length=12, nz=8, lr=1e-3, beta1=0.5, l1_weight=100.0, kl_weight=1.0,
                         video_sn_gan_weight=0.1, video_sn_vae_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0, **NN)
    eng = SAVPEngine(hp, (64, 64, 3), 2, mode='train', seed=seed)
    g = torch.Generator().manual_seed(3)
    eng.set_images(torch.rand(12, 2, 64, 64, 3, generator=g).cuda(), time_major=True)
    return eng


def _run(eng, steps):
    out = []
    for _ in range(steps):
        info = eng.train_step()
        out.append((float(info['d_loss']), float(info['g_loss'])))
    torch.cuda.synchronize()
    return out


def _state(eng):
    st = {n: eng.store[n].clone() for n in eng.store.names()}
    for k, grp in eng.store.groups.items():
        st['adam_m/' + k], st['adam_v/' + k] = grp.m.clone(), grp.v.clone()
    return st


def test_two_engines_from_one_state_agree_after_three_steps(monkeypatch):
    runs = []
    for _ in range(2):
        eng = _engine(monkeypatch, False)
        runs.append((_run(eng, 3), _state(eng)))
        del eng
    (la, sa), (lb, sb) = runs
    assert la == lb, (la, lb)
    diff = [n for n in sa if not torch.equal(sa[n], sb[n])]
    assert not diff, diff


def test_hipgraph_replay_equals_eager(monkeypatch):
    ee = _engine(monkeypatch, False)
    le = _run(ee, 3)
    eg = _engine(monkeypatch, True)
    lg = _run(eg, 3)
    assert eg.graph is not None
    assert le == lg, (le, lg)
    se, sg = _state(ee), _state(eg)
    diff = [n for n in se if not torch.equal(se[n], sg[n])]
    assert not diff, diff


def test_model_class_trains_saves_restores_and_generates(monkeypatch, tmp_path):
    from video_prediction_amd.checkpoint import read_checkpoint
    from video_prediction_amd.models import get_model_class
    Model = get_model_class('savp')
    hps = 'norm_layer=none,context_frames=2,sequence_length=5,nz=8'
    images = torch.rand(2, 5, 64, 64, 3).cuda()
    monkeypatch.delenv('SAVP_NORM_NONE')          # here the keyword opts in, and without it the model refuses
    with pytest.raises(NotImplementedError, match="norm_layer='none'"):
        Model(mode='train', hparams=hps).build_graph({'images': images})
    a = Model(mode='train', hparams=hps, norm_none=True)
    a.build_graph({'images': images})
    a.engine.set_images(images)
    info = a.engine.train_step()
    assert np.isfinite(float(info['g_loss'])) and np.isfinite(float(info['d_loss']))
    a.save(str(tmp_path / 'model-1'))
    names = set(read_checkpoint(str(tmp_path / 'model-1')))
    assert 'generator/rnn/savp_cell/h0/conv_pool2d/bias' in names and 'generator/encoder/layer_2/conv2d/bias' in names
    assert 'generator/rnn/savp_cell/lstm_h0/basic_conv2dlstm_cell/state/gamma' in names          # the cell keeps its own norms
    assert not any('InstanceNorm' in k or 'LayerNorm' in k for k in names)
    gens = []
    for restore in (False, True):          # a test model on the trained variables themselves, and a fresh one restored from the file
        b = Model(mode='test', hparams=hps, norm_none=True)
        b.build_graph({'images': images}, share_with=None if restore else a)
        if restore:
            b.restore(str(tmp_path))
            for n in b.engine.store.names():
                assert torch.equal(a.engine.store[n], b.engine.store[n]), n
        b.engine.set_images(images)
        gens.append(b.engine.generate(b.engine.default_noise(torch.Generator().manual_seed(5))).clone())
    assert torch.isfinite(gens[0]).all() and torch.equal(gens[0], gens[1])

"""SAVPEngine.eval_losses on the GPU (pytest -m gpu): the forward-only losses of a batch -- what scripts/train.py logs for the validation
batch -- against the fp64 oracle, against the train step that shares their launches, and their invisibility to training."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import savp as OS
from oracle import train as OT
from tests import gpu_model_checks as GM
from video_prediction_amd import variables as V

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, T, H, W, C = 2, 5, 32, 32, 3
T_MODEL = 4                 # the model-class tests: the shapes of tests/test_gpu_summaries.py


def _case(cond=(0, 0), seed=0, **over):
    """The hyper-parameters, variables (with the perturbations) and inputs of gpu_model_checks.check_train_step at the smallest shapes that
    still take every branch: 32x32x3 frames, B = 2, context_frames = 2, nz = 4 -- and sequence_length = 5, clip_length = 4, one more than the
    4 / 3 of the model-class tests below: video_sn_discriminator (networks.py:72-108) halves the clip with a VALID 4-tap convolution after
    two that shorten it by one frame each, so neither the reference nor the fp64 oracle can build it on clips shorter than 4 frames."""
    hpd = dict(context_frames=2, sequence_length=T, clip_length=4, nz=4, lr=2e-4, beta1=0.5, beta2=0.999, l1_weight=100.0, l2_weight=0.0,
               kl_weight=1.0, kl_anneal='none', video_sn_vae_gan_weight=0.1, video_sn_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0,
               gan_feature_cdist_weight=0.0)
    hpd.update(over)
    hp = GM.make_hparams(**hpd)
    specs = V.variable_specs(hp, (H, W, C), mode='train', cond=cond)
    vals = V.init_variables(specs, seed=4)
    rng = np.random.default_rng(9)
    for k in vals:
        if k.endswith('gamma'):
            vals[k] = (1 + 0.2 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('beta') or k.endswith('bias'):
            vals[k] = (0.1 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('initial_state'):
            vals[k] = (0.3 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('kernel') and k.startswith('generator'):
            vals[k] = (vals[k] * (30 if 'state_pred' in k else 3)).astype(np.float32)
    images = GM.synth(hp, B, H, W, C, seed)
    ci = GM.synth_cond(hp, B, cond, seed)
    noise = GM.make_noise(hp, B, seed=100, sampling=True)
    return hp, vals, dict(ci, images=images), noise


def _engine(hp, vals, inputs64, cond=(0, 0), mode='train'):
    from video_prediction_amd.models.savp_model import SAVPEngine
    eng = SAVPEngine(hp, (H, W, C), B, mode=mode, values=vals, device=DEV, cond=cond)
    eng.set_images({k: v.float().to(DEV) for k, v in inputs64.items()}, time_major=True)
    return eng


def _oracle_losses(hp, vals, inputs, noise, step=0, dtype=torch.float64):
    """The reference's summary_op on a train-mode graph (base_model.py:434-446,704-712): ONE discriminator_fn call on the generator's
    outputs, with the pre-update clip draws and no u assignment; both loss functions read its outputs."""
    P = {k: torch.tensor(v, dtype=dtype) for k, v in vals.items()}
    inputs = {k: v.to(dtype) for k, v in inputs.items()}
    noise = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in noise.items()}
    root = OS.Scope(P)
    with torch.no_grad():
        outputs = OrderedDict(OS.generator_fn(root.sub('generator'), inputs, 'train', hp, noise))
        if V.uses_discriminator(hp):
            outputs.update(OS.discriminator_fn(root.sub('discriminator'), inputs, outputs, 'train', hp, noise['d_indices_pre'],
                                               sn_state=None))
        d_losses = OT.discriminator_loss_fn(hp, inputs, outputs)
        g_losses = OT.generator_loss_fn(hp, inputs, outputs, OT.kl_weight(hp, step))
    ref = {'d_losses': OrderedDict((k, float(l)) for k, (l, w) in d_losses.items()),
           'g_losses': OrderedDict((k, float(l)) for k, (l, w) in g_losses.items()),
           'g_loss': float(OT.total_loss(g_losses))}
    if d_losses:
        ref['d_loss'] = float(OT.total_loss(d_losses))
    return ref


ALL_D = dict(image_sn_gan_weight=0.1, image_sn_vae_gan_weight=0.1, video_sn_gan_weight=0.1, video_sn_vae_gan_weight=0.1,
             images_sn_gan_weight=0.1, images_sn_vae_gan_weight=0.1, gan_feature_l2_weight=1.0)
NO_D = dict(video_sn_gan_weight=0.0, video_sn_vae_gan_weight=0.0, vae_gan_feature_cdist_weight=0.0)
CASES = OrderedDict([
    ('a_defaults', ((0, 0), {})),
    ('b_all_discriminators_feature_l2', ((0, 0), ALL_D)),
    ('c_learn_prior', ((0, 0), dict(learn_prior=True))),
    ('d_nz0_no_discriminator', ((0, 0), dict(NO_D, nz=0, kl_weight=0.0))),
    ('e_flow_tv', ((0, 0), dict(transformation='flow', tv_weight=0.05))),
    ('f_cond_state', ((4, 3), dict(state_weight=1e-4))),
])


@functools.lru_cache(maxsize=None)
def _case_and_reference(name):
    """One case's inputs and its fp64 oracle losses, computed once for the tests that share them (nothing modifies them)."""
    cond, over = CASES[name]
    hp, vals, inputs, noise = _case(cond=cond, **over)
    return cond, hp, vals, inputs, noise, _oracle_losses(hp, vals, inputs, noise)


def _compare(info, ref, rel, tol_total, tol_term, tag):
    assert set(info['d_losses']) == set(ref['d_losses']), (sorted(info['d_losses']), sorted(ref['d_losses']))
    assert set(info['g_losses']) == set(ref['g_losses']), (sorted(info['g_losses']), sorted(ref['g_losses']))
    rows = []
    if 'd_loss' in ref:
        rows.append(('d_loss', rel(float(info['d_loss']), ref['d_loss']), tol_total))
    else:
        assert float(info['d_loss']) == 0.0 and not info['d_losses']
    rows.append(('g_loss', rel(float(info['g_loss']), ref['g_loss']), tol_total))
    for grp in ('d_losses', 'g_losses'):
        for nm, (l, w) in info[grp].items():
            rows.append((nm, rel(float(l), ref[grp][nm]), tol_term))
    for nm, e, tol in rows:
        print('%s/%s: error %.3e (gate %.1e)' % (tag, nm, e, tol))
    bad = [(nm, e, tol) for nm, e, tol in rows if not e <= tol]
    assert not bad, bad


@pytest.mark.parametrize('name', list(CASES))
def test_eval_losses_against_the_fp64_oracle(name):
    """Exact-fp32 datapath: the project's tolerances for first-step losses (gpu_model_checks.check_train_step): 1e-3 relative on d_loss /
    g_loss, 2e-3 on every term."""
    cond, hp, vals, inputs, noise, ref = _case_and_reference(name)
    eng = _engine(hp, vals, inputs, cond)
    info = eng.eval_losses(noise)
    torch.cuda.synchronize()
    if name.startswith('d_'):
        assert not info['d_losses'] and set(info['g_losses']) == {'gen_l1_loss'}
    if name.startswith('b_'):
        assert len(info['d_losses']) == 6 and sum(1 for k in info['g_losses'] if k.endswith('feature_l2_loss')) == 3
    term = {'c_': 'gen_kl_loss', 'e_': 'gen_tv_loss', 'f_': 'gen_state_loss'}.get(name[:2])
    assert term is None or term in info['g_losses']
    _compare(info, ref, lambda got, want: abs(got - want) / max(abs(want), 1e-30), 1e-3, 2e-3, name)


def test_eval_losses_bf16_datapath_against_the_fp64_oracle():
    """The bench's datapath (conv operands rounded to bf16, fp32 accumulate) on the default case: every figure within 2e-2 of
    max(|ref|, 0.05), the loss yardstick of gpu_model_checks.check_train_recipe_shapes."""
    from video_prediction_amd import kernels as K
    cond, hp, vals, inputs, noise, ref = _case_and_reference('a_defaults')
    K.set_conv_precision('bf16')
    try:
        eng = _engine(hp, vals, inputs, cond)
        info = eng.eval_losses(noise)
        torch.cuda.synchronize()
    finally:
        K.set_conv_precision('f32')
    _compare(info, ref, lambda got, want: abs(got - want) / max(abs(want), 0.05), 2e-2, 2e-2, 'a_defaults/bf16')


def _bits(x):
    return np.asarray(torch.as_tensor(x).detach().float().cpu()).tobytes()


def test_eval_losses_and_the_eager_step_share_their_pre_update_terms_bit_for_bit():
    """From one state and the same noise, eval_losses() and then an eager train_step(): the terms the step takes from the same launches
    before any update are the same bits: discrim_*, gen_l1 / gen_l2, gen_kl, gen_state.  Left out by name: gen_tv_loss (the step sums it
    inside BPTT, last time step first, eval_losses first step first) and the gen_*_gan / *_feature_* terms (the step takes them from a
    second discriminator pass, against the UPDATED discriminator and with the post-update clip draws)."""
    cond = (4, 3)
    hp, vals, inputs, noise = _case(cond=cond, state_weight=1e-4, l2_weight=1.0)
    eng = _engine(hp, vals, inputs, cond)
    ev = eng.eval_losses(noise)
    ev2 = eng.eval_losses(noise)                    # same batch, noise and state: the same bits
    st = eng.train_step(noise)
    torch.cuda.synchronize()
    assert eng.graph is None                        # the first step is eager
    shared = [k for k in ev['g_losses'] if k in ('gen_l1_loss', 'gen_l2_loss', 'gen_kl_loss', 'gen_state_loss')]
    assert len(shared) == 4 and len(ev['d_losses']) == 2 and all(k.startswith('discrim_') for k in ev['d_losses'])
    for grp, names in (('d_losses', list(ev['d_losses'])), ('g_losses', shared)):
        for k in names:
            assert _bits(ev[grp][k][0]) == _bits(st[grp][k][0]), (k, float(ev[grp][k][0]), float(st[grp][k][0]))
            assert ev[grp][k][1] == st[grp][k][1]
    assert _bits(ev['d_loss']) == _bits(st['d_loss'])
    for grp in ('d_losses', 'g_losses'):
        assert list(ev[grp]) == list(ev2[grp]) == list(st[grp])
        for k in ev[grp]:
            assert _bits(ev[grp][k][0]) == _bits(ev2[grp][k][0]), k
    assert _bits(ev['g_loss']) == _bits(ev2['g_loss']) and _bits(ev['d_loss']) == _bits(ev2['d_loss'])


def test_a_test_mode_engine_has_no_losses():
    hp, vals, inputs, noise = _case()
    test_vals = {k: v for k, v in vals.items() if k in V.variable_specs(hp, (H, W, C), mode='test')}
    eng = _engine(hp, test_vals, inputs, mode='test')
    with pytest.raises(RuntimeError, match='train'):
        eng.eval_losses(noise)


def _trained_model(train):
    """The model of test_summary_passes_leave_the_training_state_untouched, plus what gives the pass something to disturb: two image
    discriminators (a second optimiser, spectral-norm vectors, clip draws), a feature loss and a KL term."""
    from video_prediction_amd.models import get_model_class
    hp = dict(context_frames=2, sequence_length=T_MODEL, nz=4, clip_length=3, batch_size=B, image_sn_gan_weight=0.1,
              images_sn_vae_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0, kl_weight=1.0, kl_anneal='none')
    m = get_model_class('savp')(mode='train', hparams_dict=hp, eval_num_samples=2)
    m.build_graph(train)
    for _ in range(3):                              # one eager step, the capture, one replay
        info = m.train_step(train)
    return m, info


def _state(eng):
    G_ = eng.store.groups
    s = {'aux.p': G_['aux'].p.clone(), 'images': eng.images_tm.clone()}
    for grp in ('g', 'd'):
        s[grp + '.p'], s[grp + '.m'], s[grp + '.v'] = G_[grp].p.clone(), G_[grp].m.clone(), G_[grp].v.clone()
    return s, (eng.step, G_['g'].t, G_['d'].t), eng.default_noise()


def _assert_same_state(a, b):
    (s0, c0, n0), (s1, c1, n1) = a, b
    assert c0 == c1
    for k in s0:
        assert torch.equal(s0[k].view(torch.int32), s1[k].view(torch.int32)), k
    assert set(n0) == set(n1)
    for k in n0:
        a_, b_ = n0[k], n1[k]
        if isinstance(a_, dict):
            assert all(torch.equal(a_[j][i], b_[j][i]) for j in a_ for i in (0, 1)), k
        else:
            assert torch.equal(a_, b_), k


def test_validation_losses_leave_the_training_state_untouched():
    """The comparison of test_gpu_summaries.test_summary_passes_leave_the_training_state_untouched applied to eval_losses() and to
    scalar_summary_fn(val, losses=True): variables, both moments of both optimisers, u, the counters and the next step's draws are the same
    bits, the step stays captured, and the next train_step equals, bit for bit, that of a twin model that never ran the pass."""
    g = torch.Generator().manual_seed(9)
    train = {'images': torch.rand(B, T_MODEL, 32, 32, 3, generator=g).to(DEV)}
    val = {'images': torch.rand(B, T_MODEL, 32, 32, 3, generator=g).to(DEV)}
    m, _ = _trained_model(train)
    twin, _ = _trained_model(train)
    eng = m.engine
    torch.cuda.synchronize()
    assert all(torch.equal(a.p.view(torch.int32), b.p.view(torch.int32))
               for a, b in ((eng.store.groups[k], twin.engine.store.groups[k]) for k in ('g', 'd', 'aux')))     # the twin IS a twin
    before = _state(eng)
    info = eng.eval_losses()
    out = m.scalar_summary_fn(val, losses=True)
    assert {'g_loss', 'd_loss', 'loss', 'gen_l1_loss', 'gen_kl_loss', 'psnr', 'ssim'} <= set(out)
    assert set(info['g_losses']) | set(info['d_losses']) <= set(out) and len(info['d_losses']) == 2
    assert not {'g_loss', 'd_loss', 'loss'} & set(m.scalar_summary_fn(val))        # without losses=True: today's entries
    m.inputs = train
    eng.set_images(train)
    torch.cuda.synchronize()
    _assert_same_state(before, _state(eng))
    assert eng.graph is not None                    # the step stays captured; the next one replays
    got, want = m.train_step(train), twin.train_step(train)
    torch.cuda.synchronize()
    for grp in ('d_losses', 'g_losses'):
        assert list(got[grp]) == list(want[grp])
        for k in got[grp]:
            assert _bits(got[grp][k][0]) == _bits(want[grp][k][0]), k
    for k in ('g', 'd', 'aux'):
        a, b = eng.store.groups[k], twin.engine.store.groups[k]
        for name in ('p', 'm', 'v'):
            assert torch.equal(getattr(a, name).view(torch.int32), getattr(b, name).view(torch.int32)), (k, name)

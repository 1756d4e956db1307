"""last_frames > 1 on the HIP path (savp_model.py:281,349,406-407,529-549,926-965): the multi-source transformation entries against fp64
restatements, the generator and a train step against the fp64 oracle with the multi-frame cell (tests/oracle_last_frames.py), bit-exact
repeats, dilation_rate as the no-op it is on SAVPCell, and the refusals at the kernels' limits."""
import numpy as np
import pytest
import torch

import oracle.savp as OS
from tests import oracle_last_frames as OLF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _assert_ok(res):
    bad = [(n, e, t) for (n, e, t) in res if not (e <= t)]
    assert not bad, 'parity failures (name, err, tol): %r' % bad


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
N, H, W = 2, 20, 24          # partial 16 x 16 tiles on both axes
SLOT0 = 4                    # the transformed images sit at channel 4 of a wider row, like the mask conv's input buffer


def _sources(L, C, seed):
    """L source images as channel slices [..., 0:C] of time-major 8-channel buffers (the first conv's input buffer), steps t - L + 1 ..."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.rand(L, N, H, W, 8, generator=g).to(DEV)
    return [buf[j][..., 0:C] for j in range(L)]


def _slot(nk, C, seed):
    """[N, H, W, nk * C] view at channel SLOT0 of a row of SLOT0 + nk * C + 4 channels."""
    g = torch.Generator().manual_seed(seed)
    row = torch.randn(N, H, W, SLOT0 + nk * C + 4, generator=g).to(DEV)
    return row[..., SLOT0:SLOT0 + nk * C]


def _stack(outs, C):
    """list of nk [N, H, W, C] -> [N, H, W, nk * C] with channel k * C + c."""
    return torch.stack(outs, dim=3).reshape(N, H, W, -1)


def _ref(tf, imgs, params, dout, L, nti, kh=5, kw=5):
    """fp64 forward / backward on the CPU through the multi-frame oracle's list branches: (out, d imgs, d params)."""
    imgs64 = [x.detach().double().cpu().requires_grad_(True) for x in imgs]
    p64 = params.detach().double().cpu().requires_grad_(True)
    nk = L * nti
    if tf == 'cdna':
        outs = OLF.apply_cdna_multi(imgs64, p64.reshape(N, kh, kw, nk))
    elif tf == 'dna':
        k = p64.reshape(N, H, W, kh, kw, nk) + torch.as_tensor(OS.identity_kernel((kh, kw)))[None, None, None, :, :, None]
        k = torch.relu(k - OS.RELU_SHIFT) + OS.RELU_SHIFT
        k = k / k.sum(dim=(3, 4), keepdim=True)
        outs = OLF.apply_dna_multi(imgs64, k)
    else:
        outs = OLF.apply_flows_multi(imgs64, p64.reshape(N, H, W, 2, nk))
    out = _stack(outs, imgs[0].shape[-1])
    (out * dout.detach().double().cpu()).sum().backward()
    return out.detach(), [x.grad for x in imgs64], p64.grad


def _params(tf, nk, seed, kh=5, kw=5):
    g = torch.Generator().manual_seed(seed)
    if tf == 'cdna':                      # normalised kernels [N, kh * kw, nk]
        k = torch.rand(N, kh * kw, nk, generator=g) + 0.05
        return (k / k.sum(dim=1, keepdim=True)).to(DEV)
    if tf == 'dna':                       # raw conv output [N, H, W, kh * kw * nk]
        return (0.3 * torch.randn(N, H, W, kh * kw * nk, generator=g)).to(DEV)
    return (2.5 * torch.randn(N, H, W, 2 * nk, generator=g)).to(DEV)          # flows, x components then y


def _run(tf, imgs, params, out, dout, dimgs, betas, nti, kh=5, kw=5):
    """The multi-source entry: forward into out, backward with the given gradient destinations.  Returns the parameter gradient."""
    from video_prediction_amd import kernels as K
    L = len(imgs)
    nk = L * nti
    if tf == 'cdna':
        K.cdna_apply_multi_fwd(imgs, params, out, kh, kw, nti)
        dk = torch.empty(N, kh * kw, nk, device=DEV, dtype=torch.float64)
        K.cdna_apply_multi_bwd(imgs, params, dout, dimgs, dk, kh, kw, nti, betas)
        return dk
    if tf == 'dna':
        kern = torch.empty_like(params)
        K.dna_apply_multi_fwd(imgs, params, kern, out, kh, kw, nti)
        draw = torch.empty_like(params)
        K.dna_apply_multi_bwd(imgs, params, kern, dout, draw, dimgs, kh, kw, nti, betas)
        return draw
    K.image_warp_multi_fwd(imgs, params, out, nti)
    dfl = torch.empty_like(params)
    K.image_warp_multi_bwd(imgs, params, dout, dfl, dimgs, nti, betas)
    return dfl


_TF_NTI = [('cdna', 4), ('cdna', 3), ('dna', 2), ('flow', 2)]
# every transformation at 5 x 5 over L x C, then the general (any-size) kernels at an odd and an even size, L = 2, C = 3
_MULTI = [pytest.param(tf, nti, C, L, 5, 5, id='%s-%d-%d-%d' % (tf, nti, C, L)) for L in (1, 2, 3) for C in (1, 3) for tf, nti in _TF_NTI] + \
         [pytest.param(tf, nti, 3, 2, kh, kw, id='%s-%d-3-2-k%dx%d' % (tf, nti, kh, kw))
          for kh, kw in ((3, 3), (4, 4)) for tf, nti in _TF_NTI[:3]]


@pytest.mark.parametrize('tf,nti,C,L,kh,kw', _MULTI)
def test_multi_source_transformations_vs_fp64(tf, nti, C, L, kh, kw):
    """Forward and backward of the multi-source entries on strided views against fp64: every source's image gradient (overwritten for
    some, accumulated onto what the destination held for others, not wanted for one when L > 1) and the gradient of all L * nti kernel /
    flow columns.  cdna nti = 4 runs the LDS-tiled kernels at 5 x 5, nti = 3 and every other kernel size the general ones."""
    nk = L * nti
    seed = 100 * L + 10 * C + nti
    imgs = _sources(L, C, seed)
    params = _params(tf, nk, seed + 1, kh, kw)
    out = _slot(nk, C, seed + 2)
    dout = _slot(nk, C, seed + 3)
    row_before = out._base.clone() if out._base is not None else None
    # gradient destinations: strided views too; source 0 unwanted when L > 1; beta 1 on odd sources (added to what was there)
    dbuf = torch.randn(L, N, H, W, C + 2, device=DEV)
    prior = dbuf.clone()
    dimgs = [None if (L > 1 and j == 0) else dbuf[j][..., 1:1 + C] for j in range(L)]
    betas = [j % 2 for j in range(L)]
    dpar = _run(tf, imgs, params, out, dout, dimgs, betas, nti, kh, kw)
    torch.cuda.synchronize()
    ref_out, ref_dimgs, ref_dpar = _ref(tf, imgs, params, dout, L, nti, kh, kw)
    res = [('out', _rel(out, ref_out), 1e-5), ('dparams', _rel(dpar, ref_dpar.reshape(dpar.shape)), 1e-4)]
    for j in range(L):
        if dimgs[j] is None:
            assert torch.equal(dbuf[j], prior[j]), 'source %d: an unwanted gradient was written' % j
            continue
        want = ref_dimgs[j] + (prior[j][..., 1:1 + C].double().cpu() if betas[j] else 0.0)
        res.append(('dimg%d' % j, _rel(dimgs[j], want), 1e-4))
        # channels around the view stay as they were
        assert torch.equal(dbuf[j][..., 0], prior[j][..., 0]) and torch.equal(dbuf[j][..., 1 + C:], prior[j][..., 1 + C:])
    if row_before is not None:            # the forward writes its slot and nothing else of the row
        row = out._base
        assert torch.equal(row[..., :SLOT0], row_before[..., :SLOT0]) and torch.equal(row[..., SLOT0 + nk * C:], row_before[..., SLOT0 + nk * C:])
    _assert_ok(res)


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('tf,nti', [('cdna', 4), ('cdna', 3), ('dna', 2), ('flow', 2)])
def test_one_source_multi_entry_is_the_single_source_entry_bit_for_bit(tf, nti, C):
    from video_prediction_amd import kernels as K
    seed = 7 + C + nti
    img = _sources(1, C, seed)[0]
    params = _params(tf, nti, seed + 1)
    dout = _slot(nti, C, seed + 3)
    outs, grads, dimgs = [], [], []
    for multi in (False, True):
        out = _slot(nti, C, seed + 2)
        dimg = torch.full((N, H, W, C), 0.5, device=DEV)
        if tf == 'cdna':
            dk = torch.empty(N, 25, nti, device=DEV, dtype=torch.float64)
            if multi:
                K.cdna_apply_multi_fwd([img], params, out, 5, 5, nti)
                K.cdna_apply_multi_bwd([img], params, dout, [dimg], dk, 5, 5, nti, 1)
            else:
                K.cdna_apply_fwd(img, params, out, 5, 5, nti)
                K.cdna_apply_bwd(img, params, dout, dimg, dk, 5, 5, nti, dimg_beta=1)
            g = dk
        elif tf == 'dna':
            kern, g = torch.empty_like(params), torch.empty_like(params)
            if multi:
                K.dna_apply_multi_fwd([img], params, kern, out, 5, 5, nti)
                K.dna_apply_multi_bwd([img], params, kern, dout, g, [dimg], 5, 5, nti, 1)
            else:
                K.dna_apply_fwd(img, params, kern, out, 5, 5, nti)
                K.dna_apply_bwd(img, params, kern, dout, g, dimg, 5, 5, nti, dimg_beta=1)
        else:
            g = torch.empty_like(params)
            if multi:
                K.image_warp_multi_fwd([img], params, out, nti)
                K.image_warp_multi_bwd([img], params, dout, g, [dimg], nti, 0)
            else:
                K.image_warp_fwd(img, params, out, nti)
                K.image_warp_bwd(img, params, dout, g, dimg, nti)
        torch.cuda.synchronize()
        outs.append(out.clone())
        grads.append(g.clone())
        dimgs.append(dimg.clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert torch.equal(_bits(grads[0]), _bits(grads[1]))
    if tf == 'flow':                      # scatter with float atomics: the arrival order may differ between two launches
        assert _rel(dimgs[1], dimgs[0]) <= 1e-6
    else:
        assert torch.equal(_bits(dimgs[0]), _bits(dimgs[1]))


def test_multi_source_entries_refuse_what_the_kernels_cannot_take():
    from video_prediction_amd import kernels as K
    imgs = _sources(2, 3, 1)
    with pytest.raises(RuntimeError):                                  # 9 CDNA kernels per source > MAXK = 8
        K.cdna_apply_multi_fwd(imgs, _params('cdna', 18, 2), _slot(18, 3, 3), 5, 5, 9)
    with pytest.raises(ValueError):                                    # 5 sources > SAVP_MAX_SOURCES
        K.cdna_apply_multi_fwd(_sources(5, 3, 1), _params('cdna', 20, 2), _slot(20, 3, 3), 5, 5, 4)
    c5 = torch.rand(N, H, W, 5, device=DEV)
    with pytest.raises(RuntimeError):                                  # C = 5 > MAXC
        K.dna_apply_multi_fwd([c5, c5], _params('dna', 2, 2), torch.empty(N, H, W, 50, device=DEV), torch.empty(N, H, W, 10, device=DEV), 5, 5, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------
def _generator_forward(transformation, L, nz=8, B=2, T=7, Hm=64, Wm=64, C=3, seed=0, **over):
    """tests/gpu_model_checks.check_generator_forward for any number of CDNA kernels: generated frames, masks, mask argmax, kernels."""
    from tests import gpu_model_checks as G
    from video_prediction_amd import variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = G.make_hparams(context_frames=2, sequence_length=T, nz=nz, schedule_sampling='inverse_sigmoid', last_frames=L,
                        transformation=transformation, **over)
    vals = V.init_variables(V.variable_specs(hp, (Hm, Wm, C), mode='test'), seed=4)
    rng = np.random.default_rng(9)
    for k in vals:
        if k.endswith('gamma'):
            vals[k] = (1 + 0.2 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('beta') or k.endswith('bias'):
            vals[k] = (0.1 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('kernel'):
            vals[k] = (vals[k] * 3).astype(np.float32)
    images = G.synth(hp, B, Hm, Wm, C, seed)
    noise = G.make_noise(hp, B, sampling=True)
    P = {k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()}
    with torch.no_grad():
        ref = OS.generator_fn(OS.Scope(P).sub('generator'), {'images': images}, 'train', hp, noise)
    eng = SAVPEngine(hp, (Hm, Wm, C), B, mode='test', values=vals, device=DEV)
    eng.mode = 'train'
    eng.set_images(images.float().to(DEV), time_major=True)
    eng.prep_generator_weights()
    gen = eng.forward_generator(noise, collect_masks=True)
    torch.cuda.synchronize()
    tag = 'gen_fwd_%s_L%d' % (transformation, L)
    g = eng.gen
    lo = B if nz else 0
    out = [(tag + '/gen_images', G.rel(gen[:, lo:], ref['gen_images']), 1e-3)]
    masks = g.masks.reshape(g.T1, g.N, Hm, Wm, 1, g.M)
    out.append((tag + '/masks', G.rel(masks[:, lo:], ref['masks']), 1e-3))
    m_ref = ref['masks'].squeeze(-2)
    top2 = m_ref.topk(2, dim=-1).values
    safe = (top2[..., 0] - top2[..., 1]) > 1e-5
    mism = (masks[:, lo:].squeeze(-2).argmax(-1).cpu() != m_ref.argmax(-1)) & safe
    out.append((tag + '/mask_argmax_mismatch_frac', float(mism.sum()) / float(safe.sum()), 0.0))
    out.append((tag + '/transformed_images', G.rel(eng.gen.maskin.v[:, lo:, ..., hp.ngf:hp.ngf + g.nk * C].reshape(g.T1, B, Hm, Wm, g.nk, C)
                                                   .transpose(-1, -2), ref['transformed_images'][..., :g.nk]), 1e-3))
    if transformation == 'cdna':
        kern = g.cdna_kern.v.reshape(g.T1, g.N, hp.kernel_size[0], hp.kernel_size[1], g.nk)[:, lo:]
        out.append((tag + '/cdna_kernels', G.rel(kern, ref['_kernels']), 1e-3))
    if nz:
        out.append((tag + '/gen_images_enc', G.rel(gen[:, :B], ref['gen_images_enc']), 1e-3))
    return out


@pytest.mark.parametrize('transformation,L,nti', [('cdna', 2, 4), ('dna', 2, 4), ('flow', 2, 4), ('cdna', 3, 3)])
def test_generator_forward_with_last_frames_vs_oracle(monkeypatch, transformation, L, nti):
    """Scheduled sampling on (nz = 8, T = 7): the older sources are ground truth for some samples and generated frames for others.
    (CDNA at L = 3 with 3 kernels per frame: 4 would need a 300-column kernel head, refused below.)"""
    OLF.install(monkeypatch)
    _assert_ok(_generator_forward(transformation, L, num_transformed_images=nti))


@pytest.mark.parametrize('transformation', ['cdna', 'dna', 'flow'])
def test_train_step_with_last_frames_vs_oracle(monkeypatch, transformation):
    """Losses, every variable's gradient and the Adam update against the fp64 oracle: a generated frame's gradient arrives from the
    two steps that read it (BPTT over the per-step image-gradient accumulators)."""
    from tests import gpu_model_checks as G
    OLF.install(monkeypatch)
    over = dict(tv_weight=0.05) if transformation == 'flow' else {}
    _assert_ok(G.check_train_step(B=2, T=6, nz=8, steps=1, tag='train_%s_L2' % transformation, last_frames=2,
                                  transformation=transformation, **over))


def _keep_tuning_state():
    from video_prediction_amd import kernels as K
    return dict(K.AUTOTUNE, cache=dict(K.AUTOTUNE['cache']))


def _restore_tuning_state(saved):
    from video_prediction_amd import kernels as K
    K.set_conv_precision('f32')
    K.AUTOTUNE.update(enabled=saved['enabled'], cache=saved['cache'])


def _small_engine(graph, **over):
    """Seeded engine on the bf16 datapath (shipped tuning table, live tuning of the shapes it lacks), B = 2, T = 8, 64 x 64."""
    import os
    from tests import gpu_model_checks as G
    from video_prediction_amd import kernels as K
    from video_prediction_amd import variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = G.make_hparams(context_frames=2, sequence_length=8, clip_length=4, nz=8, lr=2e-4, beta1=0.5, l1_weight=100.0, kl_weight=1.0,
                        kl_anneal='none', video_sn_gan_weight=0.1, video_sn_vae_gan_weight=0.1, vae_gan_feature_cdist_weight=10.0,
                        schedule_sampling='inverse_sigmoid', **over)
    K.set_conv_precision('bf16')
    K.enable_autotune(True)
    K.load_tuning(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'video_prediction_amd', 'tuning_gfx950_bf16.json'))
    vals = V.init_variables(V.variable_specs(hp, (64, 64, 3), mode='train'), seed=4)
    eng = SAVPEngine(hp, (64, 64, 3), 2, mode='train', values=vals, device=DEV)
    eng.use_graph = graph
    eng.set_images(G.synth(hp, 2, 64, 64, 3, 0).float().to(DEV), time_major=True)
    return eng, G.make_noise(hp, 2, seed=5, sampling=True)


def _step_outputs(eng, info):
    G_ = eng.store.groups
    out = {'gen_images': eng.gen.gen.v.clone(),
           'losses': torch.stack([info['d_loss'].reshape(()).double(), info['g_loss'].reshape(()).double()] +
                                 [l.reshape(()).double() for l, w in info['g_losses'].values()])}
    for g in ('g', 'd'):
        out[g + '.p'], out[g + '.m'], out[g + '.v'] = G_[g].p.clone(), G_[g].m.clone(), G_[g].v.clone()
    return out


def _differences(a, b):
    return [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]


def test_last_frames_train_step_repeats_bit_identically_eager_and_replayed():
    """L = 2 cdna: a train step from the same state gives bit-identical frames, losses, variables and Adam moments, launched one by
    one twice and replayed from the captured hipGraph."""
    from tests.test_gpu_soak import _restore, _state
    saved = _keep_tuning_state()
    try:
        eng, noise = _small_engine(False, last_frames=2)
        s0 = _state(eng)
        eng.train_step(noise)                      # first use: live tuning of the shapes the table lacks
        runs = []
        for _ in range(2):
            _restore(eng, s0)
            info = eng.train_step(noise)
            torch.cuda.synchronize()
            runs.append(_step_outputs(eng, info))
        assert not _differences(runs[0], runs[1]), _differences(runs[0], runs[1])
        assert all(bool(torch.isfinite(v.float()).all()) for v in runs[0].values())
        del eng
        eng, noise = _small_engine(True, last_frames=2)
        for rep in range(3):                       # eager, capture + replay, replay
            _restore(eng, s0)
            info = eng.train_step(noise)
            torch.cuda.synchronize()
            if rep >= 1:
                assert eng.graph is not None
            d = _differences(_step_outputs(eng, info), runs[0])
            assert not d, (rep, d)
    finally:
        _restore_tuning_state(saved)


def test_dilation_rate_changes_nothing_on_savp():
    """dilation_rate never reaches apply_cdna_kernels / apply_dna_kernels on SAVPCell (savp_model.py:939-944): (2, 2) generates the same
    frames and gradients as (1, 1), bit for bit."""
    saved = _keep_tuning_state()
    try:
        got = []
        for dil in ((1, 1), (2, 2)):
            eng, noise = _small_engine(False, last_frames=2, dilation_rate=dil)
            eng.train_step(noise)                  # first use: live tuning
            info = eng.train_step(noise, return_grads=True)
            torch.cuda.synchronize()
            got.append(dict({'gen_images': eng.gen.gen.v.clone()}, **{'g/' + k: v for k, v in info['g_grads'].items()},
                            **{'d/' + k: v for k, v in info['d_grads'].items()}))
            del eng
        assert set(got[0]) == set(got[1])
        assert not _differences(got[0], got[1]), _differences(got[0], got[1])[:10]
    finally:
        _restore_tuning_state(saved)


@pytest.mark.parametrize('over,match', [(dict(last_frames=4, transformation='dna'), 'at most 16'),  # 16 + 2 + 1 = 19 masks
                                        (dict(last_frames=3), 'at most 256'),                      # 25 x 12 CDNA kernel columns
                                        (dict(last_frames=5, num_transformed_images=1), 'at most 4 source frames'),
                                        (dict(last_frames=2, num_transformed_images=9, first_image_background=False,
                                              prev_image_background=False, generate_scratch_image=False), 'at most 8 CDNA kernels')])
def test_last_frames_beyond_the_kernel_limits_is_refused(over, match):
    from tests import gpu_model_checks as G
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = G.make_hparams(context_frames=2, sequence_length=6, nz=8, **over)
    with pytest.raises(NotImplementedError, match=match):
        SAVPEngine(hp, (64, 64, 3), 2, mode='train', seed=4, device=DEV)

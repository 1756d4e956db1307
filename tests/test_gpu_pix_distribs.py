"""inputs['pix_distribs'] on the HIP path: the one-launch recurrence (csrc/pix_distribs.hip) against the float64 restatement
(tests/oracle_pix_distribs.py) on identical fp32 inputs, exact delta transport, bit-equal repeats, the model's outputs against the hooked
oracle, and the dataset's splat kernel against numpy.

Op-level tolerance (profiles/pix_distribs.md): err = max over the (step, sample, designated pixel) maps of max |kernel - float64| / max(map).
Measured worst case over the op-level cases below on MI355X: 3.31e-7 (flow, 128 x 128, last_frames 2, sources in global memory; the
fourteen cases lie between 2.30e-7 and 3.31e-7); OP_GATE is four times that.  Every
case also has to stay below its a-priori worst case (nk * kh * kw + M + log2(H * W) + 4) * T1 * 2^-24 (one rounding per product and per
addition of a map element per step: the taps of the nk transformations -- four bilinear corners for a flow --, the M slots of the composite,
the tree sum of the normalisation, and the softmax, the division and the weight products; errors are carried through the T1 steps)."""
import math

import numpy as np
import pytest
import torch

import oracle.savp as OS
from oracle import tfrecord as R
from tests import oracle_last_frames as OLF
from tests import oracle_pix_distribs as OP

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, T1, CF = 3, 5, 2
OP_GATE = 4 * 3.31e-7

BACKGROUNDS = [dict(),                                                                       # previous image, first image, scratch
               dict(prev_image_background=False, generate_scratch_image=False),              # first image only
               dict(last_image_background=True, last_context_image_background=True),
               dict(context_images_background=True),
               dict(first_image_background=False)]


def _hp(tf, L, nti, **over):
    from tests import gpu_model_checks as G
    return G.make_hparams(context_frames=CF, sequence_length=T1 + 1, transformation=tf, last_frames=L, num_transformed_images=nti, **over)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _gt_rows(n=N):
    """Ground truth for the context steps, then rows that mix ground-truth and generated samples."""
    rows = [[1] * n, [1] * n, [1, 0, 1], [0, 0, 1], [0, 1, 0]]
    return torch.tensor([r[:n] for r in rows], dtype=torch.int32)


def _case_inputs(tf, L, nti, H, W, P, seed, n=N, strided=True, ks=(5, 5)):
    """fp32 inputs on the device as the unroll keeps them: pix_in as a channel slice of a wider buffer, logits in a row padded to a
    multiple of four, flows in a padded row; random positive kernels, flows and logits."""
    g = torch.Generator().manual_seed(seed)
    nk, taps = L * nti, ks[0] * ks[1]
    pix = torch.rand(T1 + 1, n, H, W, P, generator=g) + 0.01
    pix = pix / pix.sum(dim=(2, 3), keepdim=True)
    if strided:
        buf = torch.zeros(T1 + 1, n, H, W, P + 3)
        buf[..., 1:1 + P] = pix
        pix_dev = buf.to(DEV)[..., 1:1 + P]
    else:
        pix_dev = pix.to(DEV)
    if tf == 'cdna':
        k = torch.rand(T1, n, taps, nk, generator=g) + 0.02
        tfp = k / k.sum(dim=2, keepdim=True)
    elif tf == 'dna':
        k = torch.rand(T1, n, H, W, taps, nk, generator=g) + 0.02
        tfp = (k / k.sum(dim=4, keepdim=True)).reshape(T1, n, H, W, taps * nk)
    else:
        tfp = torch.zeros(T1, n, H, W, (2 * nk + 3) // 4 * 4)
        tfp[..., :2 * nk] = 2.0 * torch.randn(T1, n, H, W, 2 * nk, generator=g)
    return pix_dev, tfp.to(DEV), g


def _oracle(hp, pix_dev, gt, tfp, masks64, H, W):
    nk = hp.last_frames * hp.num_transformed_images
    n = pix_dev.shape[1]
    pix64 = pix_dev.detach().double().cpu()
    t64 = tfp.detach().double().cpu()
    kernels = flows = None
    kh, kw = hp.kernel_size
    if hp.transformation == 'cdna':
        kernels = t64.reshape(T1, n, kh, kw, nk)
    elif hp.transformation == 'dna':
        kernels = t64.reshape(T1, n, H, W, kh, kw, nk)
    else:
        flows = t64[..., :2 * nk].reshape(T1, n, H, W, 2, nk)
    return OP.recurrence(pix64, gt.bool(), hp, masks64, kernels=kernels, flows=flows)


def _map_err(got, ref):
    """max over the [T1, N, P] maps of max |got - ref| / max(ref map)."""
    got, ref = got.detach().double().cpu(), ref.double()
    num = (got - ref).abs().amax(dim=(2, 3))
    return float((num / ref.amax(dim=(2, 3))).max())


def _a_priori(tf, nk, M, H, W, ks=(5, 5)):
    taps = 4 if tf == 'flow' else ks[0] * ks[1]
    return (nk * taps + M + math.log2(H * W) + 4) * T1 * 2.0 ** -24


def _run_case(tf, L, nti, H, W, P, bg, transformed, force_global, seed, expect_resident=None, ks=(5, 5)):
    from video_prediction_amd import kernels as K
    hp = _hp(tf, L, nti, kernel_size=ks, **bg)
    names = OP.slot_names(hp)
    M, nk = len(names), L * nti
    pix_dev, tfp, g = _case_inputs(tf, L, nti, H, W, P, seed, ks=ks)
    logits = torch.zeros(T1, N, H, W, (M + 3) // 4 * 4)
    logits[..., :M] = 2.0 * torch.randn(T1, N, H, W, M, generator=g)
    logits = logits.to(DEV)
    gt = _gt_rows().to(DEV)
    from video_prediction_amd import lib
    kinds = {'transformed': lib.PIX_SLOT_TRANSFORMED, 'current': lib.PIX_SLOT_CURRENT, 'fixed': lib.PIX_SLOT_FIXED,
             'last_context': lib.PIX_SLOT_LAST_CONTEXT}
    slots = [(kinds[k], a) for k, a in names]
    gen = torch.empty(T1, N, H, W, P, device=DEV)
    tr = torch.empty(T1, N, H, W, P, M, device=DEV) if transformed else None
    resident = K.pix_distribs_fwd(pix_dev, gt, tf, tfp, logits, gen, slots, L, nti, CF, ks[0], ks[1], transformed=tr, force_global=force_global)
    gen2 = torch.empty_like(gen)
    K.pix_distribs_fwd(pix_dev, gt, tf, tfp, logits, gen2, slots, L, nti, CF, ks[0], ks[1], force_global=force_global)
    torch.cuda.synchronize()
    assert resident == (not force_global if expect_resident is None else expect_resident)
    masks64 = torch.softmax(logits[..., :M].double().cpu(), dim=-1)
    ref_gen, ref_tr = _oracle(hp, pix_dev, gt.cpu(), tfp, masks64, H, W)
    err = _map_err(gen, ref_gen)
    bound = _a_priori(tf, nk, M, H, W, ks)
    sums = gen.double().sum(dim=(2, 3))
    print('pix_distribs op %s k%dx%d L=%d nti=%d %dx%d P=%d M=%d %s: err %.3e  a-priori %.3e  gate %.3e  max |sum - 1| %.3e'
          % (tf, ks[0], ks[1], L, nti, H, W, P, M, 'lds' if resident else 'global', err, bound, OP_GATE, float((sums - 1).abs().max())))
    assert torch.equal(_bits(gen), _bits(gen2)), 'two launches differ'
    assert float((sums - 1).abs().max()) <= 1e-5
    if transformed:
        tr_err = float((tr.double().cpu() - ref_tr).abs().max() / ref_tr.abs().max())
        assert tr_err <= OP_GATE, tr_err
    assert err < bound, (err, bound)
    assert err <= OP_GATE, (err, OP_GATE)
    return err


_GRID = [(tf, L, hw) for tf in ('cdna', 'dna', 'flow') for L in (1, 2) for hw in ((8, 8), (12, 16))]


@pytest.mark.parametrize('i', range(len(_GRID)), ids=['%s-L%d-%dx%d' % (tf, L, hw[0], hw[1]) for tf, L, hw in _GRID])
def test_recurrence_vs_float64(i):
    """cdna / dna / flow x last_frames {1, 2} x {8 x 8, 12 x 16}: P is 1 or 3 at either size, the background options rotate so that each
    appears, transformed_pix_distribs is asked for in half of the cases, and every third case takes its sources from global memory."""
    tf, L, (H, W) = _GRID[i]
    _run_case(tf, L, 4 if L == 1 else 2, H, W, P=(1, 3)[(i + i // 2) % 2], bg=BACKGROUNDS[i % len(BACKGROUNDS)],
              transformed=(i + i // 4) % 2 == 1, force_global=i % 3 == 0, seed=40 + i)


_SIZES = [(tf, ks, fg) for tf in ('cdna', 'dna') for ks in ((3, 3), (4, 4)) for fg in (False, True)]


@pytest.mark.parametrize('tf,ks,force_global', _SIZES, ids=['%s-k%dx%d-%s' % (tf, ks[0], ks[1], 'global' if fg else 'lds') for tf, ks, fg in _SIZES])
def test_recurrence_at_another_kernel_size_vs_float64(tf, ks, force_global):
    """kernel_size (3, 3) and (4, 4) on 8 x 8: the any-window loop of the kernel (the unrolled one is 5 x 5 only), an even size with its
    unequal pads, sources in LDS and in global memory.  Same gate and a-priori bound (with the window's own tap count) as at 5 x 5."""
    _run_case(tf, 2, 2, 8, 8, P=3, bg=BACKGROUNDS[0], transformed=True, force_global=force_global, seed=70 + ks[0], ks=ks)


def test_recurrence_64x64_with_four_sources_is_lds_resident():
    """Four source maps and the new one at 64 x 64: 80 KB of LDS, beyond the 64 KB a kernel gets without the dynamic-LDS attribute."""
    _run_case('cdna', 4, 2, 64, 64, P=1, bg=dict(), transformed=False, force_global=False, seed=7, expect_resident=True)


def test_recurrence_128x128_with_two_sources_reads_global_memory():
    """Three 64 KB maps do not fit: the sources are the pix_in / gen rows, a workgroup barrier between a step's stores and the next loads."""
    _run_case('flow', 2, 2, 128, 128, P=1, bg=dict(), transformed=True, force_global=False, seed=8, expect_resident=False)


@pytest.mark.parametrize('force_global', [False, True])
@pytest.mark.parametrize('tf', ['cdna', 'flow'])
def test_delta_transport_is_exact(tf, force_global):
    """A delta under one-hot CDNA taps / integer flows in the interior, one-hot masks from logits 0 / -2000 (exp(-2000) is 0 in fp32 and in the oracle's fp64): every
    map holds exactly 1.0 at the oracle's position and 0 elsewhere."""
    from video_prediction_amd import kernels as K
    from video_prediction_amd import lib
    H, W, P, nti = 12, 16, 2, 2
    hp = _hp(tf, 1, nti)
    names = OP.slot_names(hp)
    M = len(names)
    pix = torch.zeros(T1 + 1, N, H, W, P)
    pix[:, :, 3, 9, 0] = 1.0
    pix[:, :, 6, 8, 1] = 1.0
    if tf == 'cdna':
        tfp = torch.zeros(T1, N, 25, nti)
        tfp[:, :, 1 * 5 + 3, 0] = 1.0                 # tap (1, 3): reads (y - 1, x + 1), the delta moves down and to the left
        tfp[:, :, 2 * 5 + 2, 1] = 1.0
    else:
        tfp = torch.zeros(T1, N, H, W, 4)
        tfp[..., 0], tfp[..., 2] = 1.0, -1.0          # transformation 0: (fx, fy) = (1, -1), the same move
    logits = torch.full((T1, N, H, W, 8), -2000.0)
    logits[..., 0] = 0.0
    gt = _gt_rows()
    kinds = {'transformed': lib.PIX_SLOT_TRANSFORMED, 'current': lib.PIX_SLOT_CURRENT, 'fixed': lib.PIX_SLOT_FIXED}
    gen = torch.empty(T1, N, H, W, P, device=DEV)
    K.pix_distribs_fwd(pix.to(DEV), gt.to(DEV), tf, tfp.to(DEV), logits.to(DEV), gen, [(kinds[k], a) for k, a in names], 1, nti, CF, 5, 5,
                       force_global=force_global)
    torch.cuda.synchronize()
    masks64 = torch.softmax(logits[..., :M].double(), dim=-1)
    ref, _ = _oracle(hp, pix, gt, tfp, masks64, H, W)
    assert torch.equal(gen.double().cpu(), ref)
    assert float(ref.max()) == 1.0 and int((ref != 0).sum()) == T1 * N * P
    # sample 1 (ground truth at steps 0, 1 and 4): one move of (+1, -1) from the recorded (3, 9), two more from its own predictions, then
    # the recorded position again; sample 0 (ground truth at steps 0, 1 and 2) keeps predicting from step 3 on
    assert [tuple(int(v) for v in torch.nonzero(ref[t, 1, :, :, 0])[0]) for t in range(T1)] == [(4, 8), (4, 8), (5, 7), (6, 6), (4, 8)]
    assert [tuple(int(v) for v in torch.nonzero(ref[t, 0, :, :, 0])[0]) for t in range(T1)] == [(4, 8), (4, 8), (4, 8), (5, 7), (6, 6)]


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: 32 x 32, B = 2, T = 6, context 2, nz = 8
# ---------------------------------------------------------------------------------------------------------------------------------
B, T, HM, P_MODEL = 2, 6, 32, 2


def _model_setup(transformation, L, nti, seed=0):
    from tests import gpu_model_checks as G
    from video_prediction_amd import variables as V
    hp = G.make_hparams(context_frames=2, sequence_length=T, nz=8, schedule_sampling='inverse_sigmoid', last_frames=L,
                        transformation=transformation, num_transformed_images=nti)
    vals = V.init_variables(V.variable_specs(hp, (HM, HM, 3), mode='test'), seed=4)
    rng = np.random.default_rng(9)
    for k in vals:
        if k.endswith('gamma'):
            vals[k] = (1 + 0.2 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('beta') or k.endswith('bias'):
            vals[k] = (0.1 * rng.standard_normal(vals[k].shape)).astype(np.float32)
        elif k.endswith('kernel'):
            vals[k] = (vals[k] * 3).astype(np.float32)
    images = G.synth(hp, B, HM, HM, 3, seed)
    g = torch.Generator().manual_seed(11)
    pix = torch.rand(T, B, HM, HM, P_MODEL, generator=g, dtype=torch.float64) ** 8 + 1e-3          # peaked maps
    pix = (pix / pix.sum(dim=(2, 3), keepdim=True)).float().double()                              # fp32-representable
    return hp, vals, images, pix, G.make_noise(hp, B, sampling=True)


@pytest.mark.parametrize('transformation,L,nti', [('cdna', 1, 4), ('flow', 1, 4), ('dna', 1, 4), ('cdna', 2, 4)])
def test_generator_fn_pix_outputs_vs_hooked_oracle(monkeypatch, transformation, L, nti):
    """generator_fn with an engine built for P = 2 on the exact-fp32 datapath: gen_pix_distribs / transformed_pix_distribs of both unrolls
    against the oracle's cell with the pix_distribs hook, at the tolerance tests/gpu_model_checks.py applies to gen_images there (1e-3 of
    the reference's maximum); scheduled sampling on, so generated maps feed back for some samples."""
    from tests import gpu_model_checks as G
    from video_prediction_amd.models import savp_model as M
    hp, vals, images, pix, noise = _model_setup(transformation, L, nti)
    if L > 1:
        OLF.install(monkeypatch)
    OP.install(monkeypatch, pix)
    Pv = {k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()}
    with torch.no_grad():
        ref = OS.generator_fn(OS.Scope(Pv).sub('generator'), {'images': images}, 'train', hp, noise)
    eng = M.SAVPEngine(hp, (HM, HM, 3), B, mode='test', values=vals, device=DEV, pix_distribs=P_MODEL)
    eng.mode = 'train'                               # honour the injected scheduled-sampling mask like mode='train' does
    out = M.generator_fn({'images': images.float().to(DEV), 'pix_distribs': pix.float().to(DEV)}, 'train', hp, engine=eng, noise=noise)
    torch.cuda.synchronize()
    res = []
    for k in ('gen_images', 'gen_pix_distribs', 'transformed_pix_distribs'):
        for sfx in ('', '_enc'):
            assert tuple(out[k + sfx].shape) == tuple(ref[k + sfx].shape), (k + sfx, out[k + sfx].shape, ref[k + sfx].shape)
            res.append((k + sfx, G.rel(out[k + sfx], ref[k + sfx]), 1e-3))
    print('pix_distribs model %s L=%d: %s' % (transformation, L, ', '.join('%s %.2e' % (n, e) for n, e, _ in res)))
    bad = [(n, e, t) for n, e, t in res if not e <= t]
    assert not bad, bad
    sums = out['gen_pix_distribs'].double().sum(dim=(2, 3))
    assert float((sums - 1).abs().max()) <= 1e-5


def _model(pix_distribs, datapath='f32'):
    from video_prediction_amd.models import get_model_class
    hp, vals, images, pix, noise = _model_setup('cdna', 1, 4)
    model = get_model_class('savp')(mode='test', hparams_dict=dict(context_frames=2, sequence_length=T, nz=8), pix_distribs=pix_distribs)
    inputs = {'images': images.float().to(DEV).transpose(0, 1)}
    if pix_distribs:
        inputs['pix_distribs'] = pix.float().to(DEV).transpose(0, 1)
    model.build_graph(inputs, values=vals, device=DEV)
    return model, inputs, noise


def test_generate_returns_batch_major_maps_and_leaves_the_images_alone():
    """model.generate(): gen_pix_distribs(_enc) [B, T-1, H, W, P]; called three times (eager, captured, replayed) the maps repeat bit for
    bit; a model built without the opt-in has none of the keys, and its gen_images are those of the P = 2 model, bit for bit."""
    from video_prediction_amd.models import savp_model as M
    model, inputs, noise = _model(True)
    assert model.engine.P == P_MODEL
    runs = []
    for _ in range(3):
        out = model.generate(inputs, noise=noise)
        torch.cuda.synchronize()
        runs.append({k: out[k].clone() for k in ('gen_images', 'gen_images_enc', 'gen_pix_distribs', 'gen_pix_distribs_enc')})
    for k, v in runs[0].items():
        assert tuple(v.shape) == (B, T - 1, HM, HM, P_MODEL if 'pix' in k else 3), (k, v.shape)
        assert bool(torch.isfinite(v).all())
        for r in runs[1:]:
            assert torch.equal(_bits(r[k]), _bits(v)), k
    assert float((runs[0]['gen_pix_distribs'].double().sum(dim=(2, 3)) - 1).abs().max()) <= 1e-5
    with pytest.raises(KeyError):
        model.generate({'images': inputs['images']}, noise=noise)          # built with the key: a later batch without it
    plain, plain_inputs, _ = _model(False)
    assert plain.engine.P == 0
    out = plain.generate(plain_inputs, noise=noise)
    torch.cuda.synchronize()
    assert not [k for k in out if 'pix' in k]
    assert not [k for k in M.generator_fn({'images': plain_inputs['images'].transpose(0, 1)}, 'test', plain.hparams, engine=plain.engine,
                                          noise=noise) if 'pix' in k]
    out = plain.generate(plain_inputs, noise=noise)
    torch.cuda.synchronize()
    for k in ('gen_images', 'gen_images_enc'):
        assert torch.equal(_bits(out[k]), _bits(runs[0][k])), k
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        plain.generate(inputs, noise=noise)                                 # a key given to a model built without it


def test_bf16_datapath_maps_are_finite_and_sum_to_one():
    from video_prediction_amd import kernels as K
    K.set_conv_precision('bf16')
    try:
        model, inputs, noise = _model(True)
        out = model.generate(inputs, noise=noise)
        torch.cuda.synchronize()
        for k in ('gen_pix_distribs', 'gen_pix_distribs_enc'):
            assert bool(torch.isfinite(out[k]).all()), k
            assert float((out[k].double().sum(dim=(2, 3)) - 1).abs().max()) <= 1e-5, k
    finally:
        K.set_conv_precision('f32')


# ---------------------------------------------------------------------------------------------------------------------------------
# dataset
# ---------------------------------------------------------------------------------------------------------------------------------
def _positions(i, t):
    """(y, x) of two designated pixels on multiples of 1/8 (every weight is exact in fp32): an interior track, and a second one that
    sits on the right-hand edge, leaves the frame and comes back."""
    second = [(5.0, HM - 0.5), (HM - 1.0, HM - 1.0), (-3.0, 4.0), (HM + 2.5, 7.0), (7.125, 0.0), (31.5, 31.5)][t]
    return [4.0 + i + t * 0.625, 9.5 + t * 1.125, second[0], second[1]]


def test_dataset_pix_distribs_equal_numpy_and_feed_generate(tmp_path):
    from video_prediction_amd.datasets import SoftmotionVideoDataset
    from video_prediction_amd.models import get_model_class
    d = tmp_path / 'val'
    d.mkdir()
    rng = np.random.default_rng(0)
    exs = []
    for i in range(B):
        feats = {}
        for t in range(T):
            feats['%d/image_aux1/encoded' % t] = rng.integers(0, 256, (HM, HM, 3), dtype=np.uint8).tobytes()
            feats['%d/object_pos' % t] = _positions(i, t)
        exs.append(R.encode_example(feats))
    R.write_records(str(d / 'traj_0_to_1.tfrecords'), exs)
    hpd = dict(sequence_length=T, context_frames=2)
    assert 'pix_distribs' not in next(SoftmotionVideoDataset(str(d), mode='val', num_epochs=1, hparams_dict=hpd, pix_distribs=False)
                                      .make_batch(B, device=DEV))
    ds = SoftmotionVideoDataset(str(d), mode='val', num_epochs=1, hparams_dict=hpd, pix_distribs=True)
    batch = next(ds.make_batch(B, device=DEV))
    torch.cuda.synchronize()
    assert tuple(batch['pix_distribs'].shape) == (B, T, HM, HM, 2)
    want = np.stack([OP.pix_distribs_of(np.array([_positions(i, t) for t in range(T)], np.float32), HM, HM) for i in range(B)])
    assert np.array_equal(batch['pix_distribs'].cpu().numpy(), want)
    assert float(want[0, 2, :, :, 1].sum()) == 0.0 and float(want[0, 0, :, :, 1].sum()) == 1.0       # out of frame / wrapped on the edge
    model = get_model_class('savp')(mode='test', hparams_dict=dict(context_frames=2, sequence_length=T, nz=8), pix_distribs=True)
    model.build_graph(batch, device=DEV)
    out = model.generate()
    torch.cuda.synchronize()
    assert tuple(out['gen_pix_distribs'].shape) == (B, T - 1, HM, HM, 2) and tuple(out['gen_images'].shape) == (B, T - 1, HM, HM, 3)
    first = out['gen_pix_distribs'][..., 0].double()
    assert bool(torch.isfinite(first).all()) and float((first.sum(dim=(2, 3)) - 1).abs().max()) <= 1e-5

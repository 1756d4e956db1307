"""hparams.kernel_size other than (5, 5) on the HIP path: the CDNA / DNA kernels against a float64 statement of the transformation
(tests/kernel_size_refs.py) at odd, even and non-square sizes, the flow warp on flows built by hand, the generator and a train step
against the oracle, and the refusal of a SYMMETRIC pad larger than the image (tests/test_kernel_size_refusals.py has it host-side).  Rows and tolerances:
tests/gpu_checks_kernel_sizes.py."""
import pytest
import torch

from tests.kernel_size_refs import CDNA_CASES, DNA_IMAGES, DNA_SIZES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _assert_ok(res):
    bad = [(n, e, t) for (n, e, t) in res if not (e <= t)]
    assert not bad, 'parity failures (name, err, tol): %r' % bad


def _cases():
    from tests import gpu_checks_kernel_sizes as GK
    return GK


def _cdna_id(c):
    return 'k%dx%d-K%d-C%d-%dx%dx%d' % c


@pytest.mark.parametrize('case', CDNA_CASES, ids=_cdna_id)
def test_cdna_kernels_and_apply_vs_fp64(case):
    """(kh, kw, K, C, N, H, W): normalised kernels, the output in a channel slice of a wider row, image / kernel / raw gradients with the
    output gradient contiguous and as an aligned slice, the kernel-gradient buffer NaN beforehand."""
    _assert_ok(_cases().check_cdna(*case))


@pytest.mark.parametrize('case', [c for c in CDNA_CASES if c[0] % 2 == 0 or c[1] % 2 == 0], ids=_cdna_id)
def test_cdna_identity_at_an_even_side_is_the_mean_of_the_centre_taps(case):
    _assert_ok(_cases().check_even_identity(*case))


@pytest.mark.parametrize('kh,kw', DNA_SIZES)
def test_dna_apply_vs_fp64(kh, kw):
    """K in {2, 4} x C in {1, 3} on 8 x 12 (two samples) and 19 x 35 (three blocks, ragged tail); 7 x 7 also on 3 x 4, the height equal to
    the pad."""
    GK = _cases()
    res = []
    for (N, H, W) in DNA_IMAGES + ([(1, 3, 4)] if (kh, kw) == (7, 7) else []):
        for Kk in (2, 4):
            for C in (1, 3):
                res += GK.check_dna(kh, kw, Kk, C, N, H, W, seed=8 + Kk + C)
    _assert_ok(res)


@pytest.mark.parametrize('N,H,W,C,Kk', [(2, 7, 9, 3, 2), (1, 19, 35, 1, 4)])
def test_flow_warp_on_flows_built_by_hand_vs_fp64(N, H, W, C, Kk):
    _assert_ok(_cases().check_warp(N, H, W, C, Kk))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: they return before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kh,kw,H,W', [(5, 5, 1, 8), (7, 7, 2, 8), (5, 5, 8, 1), (7, 7, 8, 2), (4, 4, 1, 8), (0, 5, 8, 8), (5, 0, 8, 8),
                                       (-3, 3, 8, 8)])
def test_a_pad_larger_than_the_image_and_an_empty_kernel_are_refused(kh, kw, H, W):
    """tf.pad SYMMETRIC refuses a pad larger than the image: max(pt, kh - 1 - pt) <= H, likewise for the width.  Every single- and
    multi-source CDNA / DNA entry returns SAVP_EINVAL for it; the buffers are sized for a 7 x 7 kernel whatever is asked for."""
    from video_prediction_amd import kernels as K
    N, C, Kk, taps = 1, 3, 2, 49
    img = torch.rand(N, H, W, C, device=DEV)
    out = torch.zeros(N, H, W, 2 * Kk * C, device=DEV)
    dimg = torch.zeros(N, H, W, C, device=DEV)
    kern = torch.full((N, taps, 2 * Kk), 1.0 / taps, device=DEV)
    dk = torch.zeros(N, taps, 2 * Kk, device=DEV, dtype=torch.float64)
    raw = torch.zeros(N, H, W, taps * 2 * Kk, device=DEV)
    kn, draw = torch.zeros_like(raw), torch.zeros_like(raw)
    calls = [lambda: K.cdna_apply_fwd(img, kern, out, kh, kw, Kk),
             lambda: K.cdna_apply_bwd(img, kern, out, dimg, dk, kh, kw, Kk),
             lambda: K.cdna_apply_multi_fwd([img, img], kern, out, kh, kw, Kk),
             lambda: K.cdna_apply_multi_bwd([img, img], kern, out, [dimg, None], dk, kh, kw, Kk),
             lambda: K.dna_apply_fwd(img, raw, kn, out, kh, kw, Kk),
             lambda: K.dna_apply_bwd(img, raw, kn, out, draw, dimg, kh, kw, Kk),
             lambda: K.dna_apply_multi_fwd([img, img], raw, kn, out, kh, kw, Kk),
             lambda: K.dna_apply_multi_bwd([img, img], raw, kn, out, draw, [dimg, None], kh, kw, Kk)]
    for call in calls:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(dimg.abs().max()) == 0.0 and float(draw.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------
MODEL_CASES = [('cdna', (3, 3)), ('cdna', (4, 4)), ('dna', (3, 3))]


@pytest.mark.parametrize('transformation,ks', MODEL_CASES, ids=['%s-%dx%d' % (tf, ks[0], ks[1]) for tf, ks in MODEL_CASES])
def test_generator_forward_at_another_kernel_size_vs_oracle(transformation, ks):
    from tests import gpu_model_checks as G
    _assert_ok(G.check_generator_forward(nz=8, B=1, T=4, tag='gen_fwd_%s_k%dx%d' % (transformation, ks[0], ks[1]),
                                         transformation=transformation, kernel_size=ks))


@pytest.mark.parametrize('transformation,ks', MODEL_CASES, ids=['%s-%dx%d' % (tf, ks[0], ks[1]) for tf, ks in MODEL_CASES])
def test_train_step_at_another_kernel_size_vs_oracle(transformation, ks):
    from tests import gpu_model_checks as G
    _assert_ok(G.check_train_step(B=1, T=4, nz=8, steps=1, tag='train_%s_k%dx%d' % (transformation, ks[0], ks[1]),
                                  transformation=transformation, kernel_size=ks, video_sn_vae_gan_weight=0.0, video_sn_gan_weight=0.0,
                                  vae_gan_feature_cdist_weight=0.0))

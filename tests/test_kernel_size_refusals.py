"""The pixel-transformation entries refuse, on the host and before any launch, a SYMMETRIC pad larger than the image and a kernel
without taps: tf.pad refuses max(pad before, pad after) > size, and the kernels' mirror (sym / symi / pd_sym) reflects once only, so
such a call would read outside the image.  Every other field of the argument structs is valid, the pointers are never followed.
The model refuses a kernel_size the kernels cannot take when it is built."""
import ctypes

import pytest

# (kh, kw, H, W)
REFUSED = [(5, 5, 1, 8), (7, 7, 2, 8), (5, 5, 8, 1), (7, 7, 8, 2), (4, 4, 1, 8), (4, 4, 8, 1), (2, 2, 0, 8), (0, 5, 8, 8), (5, 0, 8, 8),
           (-3, 3, 8, 8), (-3, -3, 8, 8)]
PTR = 0x100000


def _view(lib, sp):
    v = lib.SavpView()
    v.p, v.sn, v.sp = PTR, 64 * sp, sp
    return v


def _fill(lib, a, kh, kw, H, W, multi):
    a.N, a.H, a.W, a.C, a.K, a.kh, a.kw = 1, H, W, 3, 2, kh, kw
    a.kern, a.out, a.dout = PTR, _view(lib, 12), _view(lib, 12)
    if multi:
        a.nsrc = 2
        for j in range(2):
            a.img[j], a.dimg[j] = _view(lib, 3), _view(lib, 3)
    else:
        a.img, a.dimg = _view(lib, 3), _view(lib, 3)
    return a


@pytest.mark.parametrize('kh,kw,H,W', REFUSED)
def test_cdna_and_dna_entries_refuse_the_shape(hip_lib, kh, kw, H, W):
    from video_prediction_amd import lib
    for multi in (False, True):
        a = _fill(lib, lib.SavpCdnaMultiArgs() if multi else lib.SavpCdnaArgs(), kh, kw, H, W, multi)
        a.dkern = PTR
        fwd, bwd = (hip_lib.savp_cdna_apply_multi_fwd, hip_lib.savp_cdna_apply_multi_bwd) if multi else \
                   (hip_lib.savp_cdna_apply_fwd, hip_lib.savp_cdna_apply_bwd)
        assert fwd(None, ctypes.byref(a)) == -1 and bwd(None, ctypes.byref(a)) == -1, ('cdna', multi)
        d = _fill(lib, lib.SavpDnaMultiArgs() if multi else lib.SavpDnaArgs(), kh, kw, H, W, multi)
        d.raw = d.draw = PTR
        fwd, bwd = (hip_lib.savp_dna_apply_multi_fwd, hip_lib.savp_dna_apply_multi_bwd) if multi else \
                   (hip_lib.savp_dna_apply_fwd, hip_lib.savp_dna_apply_bwd)
        assert fwd(None, ctypes.byref(d)) == -1 and bwd(None, ctypes.byref(d)) == -1, ('dna', multi)


@pytest.mark.parametrize('kh,kw,H,W', [c for c in REFUSED if c[2] > 0])
@pytest.mark.parametrize('tf', ['cdna', 'dna'])
def test_pix_distribs_entry_refuses_the_shape(hip_lib, tf, kh, kw, H, W):
    from tests.test_pix_distribs_host import _args
    from video_prediction_amd import lib
    a = _args(lib, H, W, 1, tf=lib.PIX_TF[tf], kh=kh, kw=kw)
    assert hip_lib.savp_pix_distribs_fwd(None, ctypes.byref(a)) == -1


@pytest.mark.parametrize('over,exc,match', [(dict(kernel_size=[8, 8]), NotImplementedError, 'at most 49 taps'),
                                            (dict(kernel_size=[8, 8], transformation='dna'), NotImplementedError, 'at most 49 taps'),
                                            (dict(kernel_size=[0, 5]), ValueError, 'at least 1'),
                                            (dict(kernel_size=[5, -1], transformation='dna'), ValueError, 'at least 1')])
def test_an_unsupported_kernel_size_is_refused_when_the_model_is_built(over, exc, match):
    """kernel_size = [8, 8] has 64 taps: 64 x 1 x 4 = 256 head columns pass the dense kernel's limit, the transformation kernels stop at
    49.  The refusal comes from the constructor, before it sizes a variable or touches the device, not from the first forward."""
    from tests import gpu_model_checks as G
    from video_prediction_amd.models.savp_model import SAVPEngine
    hp = G.make_hparams(context_frames=2, sequence_length=4, nz=8, **over)
    with pytest.raises(exc, match=match):
        SAVPEngine(hp, (64, 64, 3), 1, mode='train', seed=4)

"""The inputs of tests/test_gpu_ssim_large.py are judged here, on the fp64 oracle alone (no GPU): a window row or column that the strip
kernel dropped, counted twice or misplaced must move a frame's SSIM by much more than the tolerance the GPU tests allow."""
import pytest
import torch

from tests import ssim_large_cases as SC

K = 11                  # the SSIM window
MARGIN = 10.0           # a left-out row / column must show at this many times the GPU tolerance


def _band_means(a, b, axis):
    """[n_windows, T, B]: the oracle on every 11-row (axis -3) or 11-column (axis -2) band = the mean of that window row / column."""
    from oracle import metrics as OM
    n = a.shape[axis] - K + 1
    sa = torch.stack([a.narrow(axis, k, K) for k in range(n)])
    sb = torch.stack([b.narrow(axis, k, K) for k in range(n)])
    return OM.ssim(sa, sb)


@pytest.mark.parametrize('shape', SC.SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_every_window_row_and_column_matters(shape):
    H, W, C = shape
    worst = {-3: None, -2: None}
    for axis in (-3, -2):
        shift = []                                       # per profile [n_windows, T, B]: relative change of the frame's SSIM without window k
        for profile in SC.PROFILES:
            a, b = SC.frames(H, W, C, profile)
            full = SC.reference(H, W, C, profile)
            assert float(full.min()) >= 0.3 and float(full.max()) <= 0.45, (profile, full)
            bands = _band_means(a, b, axis)
            n = bands.shape[0]
            assert float((bands.mean(0) - full).abs().max()) <= 1e-12, (axis, profile)
            without = (full * n - bands) / (n - 1)
            shift.append((without - full).abs() / full)
        best = torch.stack(shift).max(0).values          # the profile that shows window k best, per frame
        worst[axis] = float(best.min()) / SC.SSIM_RTOL
        print('%dx%dx%d axis %d: smallest shift %.1f x tolerance' % (H, W, C, axis, worst[axis]))
        assert worst[axis] >= MARGIN, (axis, worst[axis])

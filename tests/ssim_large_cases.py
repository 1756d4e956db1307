"""Inputs for the SSIM tests of planes that metrics.hip walks in strips (more than 8192 pixels); importable without a GPU.

Uniform noise is useless for these: every window then has nearly the same SSIM, and a strip row that is dropped, counted twice or read from
the wrong place does not move the frame's mean.  Here the noise that separates the two frames grows across the frame in one of three
profiles, so that every window row and every window column carries a share of the mean that the GPU tolerance can see
(tests/test_ssim_large_inputs.py asserts exactly that, on the fp64 oracle alone)."""
import functools

import torch

T, B = 1, 2
PROFILES = ('rise', 'fall', 'bump')
# (H, W, C): the smallest shapes at which the strip code can go wrong
SHAPES = (
    (91, 91, 3),        # just above the 8192-pixel cap; odd; the last strip is partial
    (128, 128, 1),
    (128, 128, 3),
    (72, 120, 3),
    (120, 72, 1),
    (400, 24, 1),       # many strips
    (24, 400, 3),       # one short strip, wide rows
)
SSIM_RTOL = 2e-5        # frame_ssim against the fp64 oracle (tests/gpu_checks.py check_metrics)


def _profile(name, y, x):
    rise = 0.5 * y + 0.5 * x
    if name == 'rise':
        return rise
    if name == 'fall':
        return 1.0 - rise
    if name == 'bump':
        return 16.0 * y * (1.0 - y) * x * (1.0 - x)
    raise ValueError(name)


@functools.lru_cache(maxsize=None)
def frames(H, W, C, profile):
    """(a, b): float64 [T, B, H, W, C] in [0, 1]; a is smooth with a little noise, b = a + noise of amplitude 0.4 u^2."""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + C + 7919 * PROFILES.index(profile))
    y = torch.linspace(0, 1, H, dtype=torch.float64).reshape(1, 1, H, 1, 1)
    x = torch.linspace(0, 1, W, dtype=torch.float64).reshape(1, 1, 1, W, 1)
    shape = (T, B, H, W, C)
    a = (0.5 + 0.25 * torch.sin(6 * y + 1) * torch.cos(5 * x) + 0.1 * torch.rand(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    u = _profile(profile, y, x)
    b = (a + 0.4 * u * u * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return a, b


@functools.lru_cache(maxsize=None)
def reference(H, W, C, profile):
    """oracle.metrics.ssim of frames(...): float64 [T, B].  Computed once and shared; do not modify."""
    from oracle import metrics as OM
    a, b = frames(H, W, C, profile)
    return OM.ssim(a, b)

"""tests/kernel_size_refs.py (loops over taps with an explicit mirror) against oracle.savp (pad2d 'SAME' / 'SYMMETRIC', then a VALID
depthwise convolution or patch products): two independent statements of the reference's padding rule for any kernel size have to agree
before a HIP kernel is compared with either."""
import numpy as np
import pytest
import torch

import oracle.savp as OS
from tests import kernel_size_refs as KR

SIZES = [(1, 1), (2, 2), (3, 3), (4, 4), (3, 5), (4, 3), (5, 5), (6, 6), (7, 7)]
N, H, W, C, K = 2, 7, 9, 3, 2


def _max_abs(a, b):
    return float((a - b).abs().max())


@pytest.mark.parametrize('kh,kw', SIZES)
def test_identity_kernel_matches_the_oracle(kh, kw):
    ident = KR.identity(kh, kw)
    assert _max_abs(ident, torch.as_tensor(OS.identity_kernel((kh, kw)))) <= 1e-12
    assert abs(float(ident.sum()) - 1.0) <= 1e-15
    assert int((ident != 0).sum()) == (1 if kh % 2 else 2) * (1 if kw % 2 else 2)


@pytest.mark.parametrize('kh,kw', SIZES)
def test_cdna_reference_matches_the_oracle(kh, kw):
    rng = np.random.default_rng(100 * kh + kw)
    img = torch.tensor(rng.random((N, H, W, C)), requires_grad=True)
    raw = torch.tensor(0.3 * rng.standard_normal((N, kh, kw, K)), requires_grad=True)
    dout = torch.tensor(rng.standard_normal((N, H, W, K * C)))
    kern = KR.normalise(raw)
    out = KR.apply_kernels(img, kern)
    (out * dout).sum().backward()
    got = out.detach(), img.grad.clone(), raw.grad.clone()
    img.grad = raw.grad = None
    k2 = raw + torch.as_tensor(OS.identity_kernel((kh, kw)))[None, :, :, None]
    k2 = torch.relu(k2 - OS.RELU_SHIFT) + OS.RELU_SHIFT
    k2 = k2 / k2.sum(dim=(1, 2), keepdim=True)
    ref = torch.cat(OS.apply_cdna_kernels(img, k2), dim=-1)
    (ref * dout).sum().backward()
    assert _max_abs(kern.detach(), k2.detach()) <= 1e-12
    assert _max_abs(got[0], ref.detach()) <= 1e-12
    assert _max_abs(got[1], img.grad) <= 1e-12 * max(1.0, float(img.grad.abs().max()))
    assert _max_abs(got[2], raw.grad) <= 1e-12 * max(1.0, float(raw.grad.abs().max()))


@pytest.mark.parametrize('kh,kw', SIZES)
def test_dna_reference_matches_the_oracle(kh, kw):
    rng = np.random.default_rng(200 * kh + kw)
    img = torch.tensor(rng.random((N, H, W, C)), requires_grad=True)
    raw = torch.tensor(0.3 * rng.standard_normal((N, H, W, kh, kw, K)), requires_grad=True)
    dout = torch.tensor(rng.standard_normal((N, H, W, K * C)))
    kern = KR.normalise(raw)
    out = KR.apply_kernels(img, kern)
    (out * dout).sum().backward()
    got = out.detach(), img.grad.clone(), raw.grad.clone()
    img.grad = raw.grad = None
    k2 = raw + torch.as_tensor(OS.identity_kernel((kh, kw)))[None, None, None, :, :, None]
    k2 = torch.relu(k2 - OS.RELU_SHIFT) + OS.RELU_SHIFT
    k2 = k2 / k2.sum(dim=(3, 4), keepdim=True)
    ref = torch.cat(OS.apply_dna_kernels(img, k2), dim=-1)
    (ref * dout).sum().backward()
    assert _max_abs(kern.detach(), k2.detach()) <= 1e-12
    assert _max_abs(got[0], ref.detach()) <= 1e-12
    assert _max_abs(got[1], img.grad) <= 1e-12 * max(1.0, float(img.grad.abs().max()))
    assert _max_abs(got[2], raw.grad) <= 1e-12 * max(1.0, float(raw.grad.abs().max()))


@pytest.mark.parametrize('kh,kw', [(2, 2), (4, 4), (4, 3), (3, 4), (6, 6)])
def test_an_even_identity_kernel_averages_the_centre_taps(kh, kw):
    """The pad before an even side is one short of the pad after it, so the two centre taps read rows y and y + 1, never y - 1."""
    rng = np.random.default_rng(kh + 10 * kw)
    img = torch.tensor(rng.random((N, H, W, C)))
    out = KR.apply_kernels(img, KR.identity(kh, kw)[None, :, :, None].expand(N, kh, kw, 1))
    assert _max_abs(out, KR.centre_mean(img, kh, kw)) <= 1e-15
    want = img.clone()
    if kh % 2 == 0:
        want = 0.5 * (want + torch.cat([want[:, 1:], want[:, -1:]], dim=1))
    if kw % 2 == 0:
        want = 0.5 * (want + torch.cat([want[:, :, 1:], want[:, :, -1:]], dim=2))
    assert _max_abs(out, want) <= 1e-15


def test_the_mirror_is_single_and_refuses_a_pad_beyond_the_image():
    assert [KR.mirror(q, 3) for q in range(-3, 6)] == [2, 1, 0, 0, 1, 2, 2, 1, 0]
    assert KR.pads(4) == (1, 2) and KR.pads(7) == (3, 3) and KR.pads(1) == (0, 0)
    for q, n in ((-4, 3), (6, 3), (-2, 1)):
        with pytest.raises(ValueError):
            KR.mirror(q, n)
    with pytest.raises(ValueError):                    # H = 2 under a 7 x 7 kernel: pad 3
        KR.apply_kernels(torch.zeros(1, 2, 8, 1, dtype=torch.float64), torch.zeros(1, 7, 7, 1, dtype=torch.float64))

"""GPU parity checks of the pixel transformations at kernel sizes other than 5 x 5 (hparams.kernel_size is live: models/savp_cell.py
hands kh, kw to every entry below), and of the flow warp on flows built by hand.

The CDNA / DNA rows compare against tests/kernel_size_refs.py, a float64 statement of the transformation written from its definition
(tests/test_kernel_size_reference.py holds it against oracle.savp on the CPU); the flow rows against oracle.savp.apply_flows.  The
reference sees the float32-rounded inputs the kernels see.  Each check returns (name, err, tol) rows like tests/gpu_checks.py: err is
rel_err, or an absolute figure where the reference value is exactly zero (those rows say so in their names).  Tolerances are the ones the
5 x 5 checks use: TOL_OP for values and normalised kernels, 5e-5 for gradients.

What reaches which branch (csrc/cdna_composite.hip, csrc/warp_dna.hip):
  general cdna_apply_fwd / bwd_img / bwd_kern kernels   every CDNA_CASES row (kh, kw != 5, H or W < 3, or C in (2, 4))
  49 accumulators of cdna_apply_bwd_kern_kernel, all live  7 x 7 rows; 1 .. 16 live at the other sizes
  even-side identity (0.5 / 0.5 centre)                 4 x 4, 2 x 2, 4 x 3 rows and check_even_identity
  unequal pads before / after in the gather-form dimg   4 x 4, 2 x 2, 4 x 3 (pt 1, pb 2 / pt 0, pb 1), CDNA and DNA
  image no larger than its pad                          7 x 7 on 3 x 4 (pad 3 on a height of 3)
"""
import numpy as np
import torch

from oracle import savp as OS
from tests import kernel_size_refs as KR
from tests.bf16_exact import rel_err
from tests.gpu_checks import DEV, TOL_OP, dev
from video_prediction_amd import kernels as K

TOL_GRAD = 5e-5


def f32(a):
    """float64 tensor holding float32-representable values: what the kernel receives, exactly."""
    return torch.as_tensor(np.asarray(a), dtype=torch.float64).float().double()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float('nan'), device=DEV, dtype=dtype)


def _aligned_slice(dout, off=32):
    """dout [N, H, W, KC] as a 16-byte aligned channel slice of a wider row (row width a multiple of 4, junk around the slice)."""
    N, H, W, KC = dout.shape
    wide = torch.full((N, H, W, off + 4 * ((KC + 3) // 4) + 4), 3.0, device=DEV)
    wide[..., off:off + KC] = dev(dout)
    return wide[..., off:off + KC]


def check_cdna(kh, kw, Kk, C, N, H, W, seed=5):
    """savp_cdna_kernels_fwd/bwd and savp_cdna_apply_fwd/bwd called as check_cdna_composite calls them."""
    rng = np.random.default_rng(seed)
    out, taps, KC = [], kh * kw, Kk * C
    raw = f32(0.3 * rng.standard_normal((N, kh, kw, Kk))).requires_grad_(True)
    img = f32(rng.random((N, H, W, C))).requires_grad_(True)
    kern = KR.normalise(raw)
    kern.retain_grad()
    ref_out = KR.apply_kernels(img, kern)
    dout = f32(rng.standard_normal(tuple(ref_out.shape)))
    (ref_out * dout).sum().backward()
    tag = 'cdna_k%dx%d_K%d_C%d_%dx%dx%d' % (kh, kw, Kk, C, N, H, W)
    rawd = dev(raw).reshape(N, taps * Kk)
    kd = _nan(N, taps, Kk)
    K.cdna_kernels_fwd(rawd, kd, kh, kw, Kk)
    imgd = dev(img)
    row = torch.full((N, H, W, 32 + KC + 4), 7.0, device=DEV)          # the output is a channel slice of a wider row
    ov = row[..., 32:32 + KC]
    K.cdna_apply_fwd(imgd, kd, ov, kh, kw, Kk)
    out.append((tag + '/row_outside_the_slot_abs', float((row[..., :32] - 7.0).abs().max() + (row[..., 32 + KC:] - 7.0).abs().max()), 0.0))
    if taps == 1:          # exact: k / k is 1, 0 + pixel * 1 is the pixel
        out.append((tag + '/kernels_minus_one_abs', float((kd - 1.0).abs().max()), 0.0))
        same = torch.equal(ov.contiguous().view(torch.int32), torch.cat([imgd] * Kk, dim=-1).view(torch.int32))
        out.append((tag + '/apply_differs_from_the_image_bits', 0.0 if same else 1.0, 0.0))
    out.append((tag + '/kernels', rel_err(kd.reshape(N, kh, kw, Kk), kern), TOL_OP))
    out.append((tag + '/apply', rel_err(ov, ref_out), TOL_OP))
    for name, dview in (('', dev(dout)), ('_aligned_slice', _aligned_slice(dout))):
        dimg = _nan(N, H, W, C)
        dk = _nan(N, taps, Kk, dtype=torch.float64)
        K.cdna_apply_bwd(imgd, kd, dview, dimg, dk, kh, kw, Kk)
        out.append((tag + '/dimg' + name, rel_err(dimg, img.grad), TOL_GRAD))
        out.append((tag + '/dkern' + name, rel_err(dk.reshape(N, kh, kw, Kk), kern.grad), TOL_GRAD))
        draw = _nan(N, taps * Kk)
        K.cdna_kernels_bwd(rawd, dk, draw, kh, kw, Kk)
        if taps == 1:      # d(k / k) is 0 whatever dkern holds: the reference value is exactly zero
            out.append((tag + '/draw_abs' + name, float(draw.abs().max()), 0.0))
        else:
            out.append((tag + '/draw' + name, rel_err(draw.reshape(N, kh, kw, Kk), raw.grad), TOL_GRAD))
    torch.cuda.synchronize()
    return out


def check_even_identity(kh, kw, Kk, C, N, H, W, seed=6):
    """The identity property the model relies on at an even side: a zero dense output gives the mean of the 2 or 4 centre taps of the
    mirrored image (rows y, y + 1: the pad before an even side is the shorter one)."""
    rng = np.random.default_rng(seed)
    img = f32(rng.random((N, H, W, C)))
    taps = kh * kw
    kd = _nan(N, taps, Kk)
    K.cdna_kernels_fwd(torch.zeros(N, taps * Kk, device=DEV), kd, kh, kw, Kk)
    ov = _nan(N, H, W, Kk * C)
    K.cdna_apply_fwd(dev(img), kd, ov, kh, kw, Kk)
    torch.cuda.synchronize()
    ref = KR.apply_kernels(img, KR.normalise(torch.zeros(N, kh, kw, Kk, dtype=torch.float64)))
    mean = torch.cat([KR.centre_mean(img, kh, kw)] * Kk, dim=-1)
    tag = 'cdna_identity_k%dx%d_C%d_%dx%d' % (kh, kw, C, H, W)
    # the reference itself: (taps - 2 or 4) taps of 1e-12 next to the centre's 0.25 or 0.5
    return [(tag + '/reference_vs_centre_mean', rel_err(ref, mean), 1e-10),
            (tag + '/vs_reference', rel_err(ov, ref), TOL_OP),
            (tag + '/vs_centre_mean', rel_err(ov, mean), TOL_OP)]


def check_dna(kh, kw, Kk, C, N, H, W, seed=8):
    """savp_dna_apply_fwd/bwd: normalised kernels, output, raw-kernel gradient and image gradient (overwritten, then added to a destination
    that holds something)."""
    rng = np.random.default_rng(seed)
    out, taps = [], kh * kw
    raw = f32(0.3 * rng.standard_normal((N, H, W, kh, kw, Kk))).requires_grad_(True)
    img = f32(rng.random((N, H, W, C))).requires_grad_(True)
    kern = KR.normalise(raw)
    kern.retain_grad()
    ref = KR.apply_kernels(img, kern)
    dout = f32(rng.standard_normal(tuple(ref.shape)))
    (ref * dout).sum().backward()
    tag = 'dna_k%dx%d_K%d_C%d_%dx%dx%d' % (kh, kw, Kk, C, N, H, W)
    rawd = dev(raw).reshape(N, H, W, taps * Kk)
    imgd = dev(img)
    kd = _nan(*rawd.shape)
    row = torch.full((N, H, W, 8 + Kk * C + 3), 7.0, device=DEV)
    od = row[..., 8:8 + Kk * C]
    K.dna_apply_fwd(imgd, rawd, kd, od, kh, kw, Kk)
    out.append((tag + '/row_outside_the_slot_abs', float((row[..., :8] - 7.0).abs().max() + (row[..., 8 + Kk * C:] - 7.0).abs().max()), 0.0))
    out.append((tag + '/fwd', rel_err(od, ref), TOL_OP))
    out.append((tag + '/kern', rel_err(kd.reshape(N, H, W, kh, kw, Kk), kern), TOL_OP))
    draw, dimg = _nan(*rawd.shape), _nan(N, H, W, C)
    K.dna_apply_bwd(imgd, rawd, kd, dev(dout), draw, dimg, kh, kw, Kk)
    prior = f32(rng.standard_normal((N, H, W, C)))
    draw2, dimg2 = _nan(*rawd.shape), dev(prior)
    K.dna_apply_bwd(imgd, rawd, kd, _aligned_slice(dout, off=8), draw2, dimg2, kh, kw, Kk, dimg_beta=1)
    for name, dr in (('', draw), ('_beta1', draw2)):
        if taps == 1:      # the reference value is exactly zero: judged against the gradient that enters the normalisation
            out.append((tag + '/draw_abs_over_max_dkern' + name, float(dr.abs().max()) / float(kern.grad.abs().max()), TOL_GRAD))
        else:
            out.append((tag + '/draw' + name, rel_err(dr.reshape(N, H, W, kh, kw, Kk), raw.grad), TOL_GRAD))
    out.append((tag + '/dimg', rel_err(dimg, img.grad), TOL_GRAD))
    out.append((tag + '/dimg_beta1', rel_err(dimg2, img.grad + prior), TOL_GRAD))
    torch.cuda.synchronize()
    return out


# (fx, fy) of the hand-built regions of check_warp; W and H stand for the image's own size
def _special_flows(H, W):
    integral = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (2, -2), (-2, 2), (2, 1), (-1, -2)]
    e = 1e-3
    near = [(-e, 1 - e), (1 - e, -e), (-e, -e), (1 - e, 1 - e)]          # floor on either side of an integer
    clamp = [(sx * (W + 3), sy * (H + 3)) for sx in (1, -1) for sy in (1, -1)]
    huge = [(sx * 1e6, sy * 1e6) for sx in (1, -1) for sy in (1, -1)]
    mixed = [(1e6, 0.25), (-0.75, -1e6)]
    return integral + near + clamp + huge + mixed, len(integral) + len(near), len(integral) + len(near) + len(clamp) + len(huge)


def check_warp(N, H, W, C, Kk, seed=9):
    """savp_image_warp_fwd/bwd against oracle.savp.apply_flows on float64 copies of the float32 flows.  The flow field is built by hand:
    exactly integral flows, flows a hair below an integer, flows that clamp all four corners onto one corner pixel (+-(W + 3), +-(H + 3)
    and +-1e6: the flow gradient there is exactly zero and the image gradient lands on that corner), and 2.5 * N(0, 1) elsewhere."""
    rng = np.random.default_rng(seed)
    out = []
    special, one_pixel_lo, one_pixel_hi = _special_flows(H, W)
    flows = 2.5 * rng.standard_normal((N, H, W, 2, Kk))
    region = np.full((N, H, W, Kk), -1)
    for n in range(N):
        for k in range(Kk):
            for p in range(H * W):
                r = (7 * p + 5 * k + 3 * n) % 40
                if r < len(special):
                    flows[n, p // W, p % W, :, k] = special[r]
                    region[n, p // W, p % W, k] = r
    assert all((region == r).any() for r in range(len(special))), 'a hand-built region is missing'
    flows = f32(flows).requires_grad_(True)
    img = f32(rng.random((N, H, W, C))).requires_grad_(True)
    ref = torch.cat(OS.apply_flows(img, flows), dim=-1)
    dout = f32(rng.standard_normal(tuple(ref.shape)))
    (ref * dout).sum().backward()
    tag = 'warp_by_hand_%dx%dx%dx%d_K%d' % (N, H, W, C, Kk)
    fl = dev(flows).reshape(N, H, W, 2 * Kk)
    imgd = dev(img)
    big = torch.full((N, H, W, 8 + Kk * C), 7.0, device=DEV)
    K.image_warp_fwd(imgd, fl, big[..., 8:], Kk)
    out.append((tag + '/row_outside_the_slot_abs', float((big[..., :8] - 7.0).abs().max()), 0.0))
    out.append((tag + '/fwd', rel_err(big[..., 8:], ref), TOL_OP))
    dfl, dimg = _nan(N, H, W, 2 * Kk), _nan(N, H, W, C)
    K.image_warp_bwd(imgd, fl, dev(dout), dfl, dimg, Kk)
    dfl = dfl.reshape(N, H, W, 2, Kk)
    out.append((tag + '/dflows', rel_err(dfl, flows.grad), TOL_GRAD))
    out.append((tag + '/dimg', rel_err(dimg, img.grad), TOL_GRAD))
    # all four corners on one pixel: the four gathers are one value, so the flow gradient is exactly zero (reference and kernel)
    one = torch.as_tensor((region >= one_pixel_lo) & (region < one_pixel_hi))
    one2 = one[:, :, :, None, :].expand(N, H, W, 2, Kk)
    out.append((tag + '/dflows_one_pixel_reference_abs', float(flows.grad[one2].abs().max()), 1e-12))      # float64 round-off at most
    out.append((tag + '/dflows_one_pixel_abs', float(dfl.cpu()[one2].abs().max()), 0.0))
    # ... and the image gradient of those outputs alone lands on the four corner pixels of the image and nowhere else
    img.grad = None
    dmask = dout * one[..., None].expand(N, H, W, Kk, C).reshape(N, H, W, Kk * C).double()
    (torch.cat(OS.apply_flows(img, flows.detach()), dim=-1) * dmask).sum().backward()
    dfl2, dimg2 = _nan(N, H, W, 2 * Kk), _nan(N, H, W, C)
    K.image_warp_bwd(imgd, fl, dev(dmask), dfl2, dimg2, Kk)
    corner = torch.zeros(N, H, W, C, dtype=torch.bool)
    for y in (0, H - 1):
        for x in (0, W - 1):
            corner[:, y, x] = True
    out.append((tag + '/dimg_one_pixel_off_the_corners_reference_abs', float(img.grad[~corner].abs().max()), 0.0))
    out.append((tag + '/dimg_one_pixel_off_the_corners_abs', float(dimg2.cpu()[~corner].abs().max()), 0.0))
    out.append((tag + '/dimg_one_pixel_corners', rel_err(dimg2.cpu()[corner], img.grad[corner]), TOL_GRAD))
    torch.cuda.synchronize()
    return out

"""CPU self-test of the bf16-exact bounds (tests/bf16_exact.py) the GPU parity checks hold the bf16 datapath to.

Emulated "kernels" in torch: a bf16-operand / fp32-accumulate convolution (FPROP / DGRAD / WGRAD), a 4-way split-K fold and a
statistics epilogue.  The bounds must accept each correct emulation and reject each precision-class mutation of it -- a truncating
fp32 -> bf16 conversion, one image's last 8 output channels scaled by (1 - 2^-8), split-K partial slices stored as bf16, statistics
summed from bf16-rounded outputs, a truncated bf16 destination -- every one of which passes the old 1e-2 rule against the fp64
result of the unrounded operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.bf16_exact import TOL_EXACT, RNE_MISMATCH, bf16_apart, bf16_bracket, bf16_ulps_apart, rel_err, rne, wgrad_tol, window

OLD_TOL = 1e-2
# (N, H, W, Cx, Cy, k): the 8x8 / 16x16 / 32x32 ConvLSTM gate convolutions (smaller batches) and a 64x64 3x3 head
SHAPES = [(2, 8, 8, 264, 128, 5), (2, 16, 16, 136, 64, 5), (1, 32, 32, 72, 32, 5), (2, 64, 64, 32, 32, 3)]


def trunc(t):
    """fp32 -> bf16 by dropping the low 16 bits (round toward zero): the mutation of the RNE conversion."""
    return (t.float().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def _data(shape, seed):
    N, H, W, Cx, Cy, k = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cx, H, W, generator=g)
    w = torch.randn(Cy, Cx, k, k, generator=g) * 0.05
    dy = torch.randn(N, Cy, H, W, generator=g)
    return x, w, dy, k // 2


def _fprop(x, w, pad, cast):
    """The kernel under emulation: operands through `cast`, fp32 products and sums."""
    return F.conv2d(cast(x).float(), cast(w).float(), padding=pad)


def _dgrad(dy, w, x_shape, pad, cast):
    return torch.nn.grad.conv2d_input(x_shape, cast(w).float(), cast(dy).float(), padding=pad)


def _wgrad(x, dy, w_shape, pad, cast):
    return torch.nn.grad.conv2d_weight(cast(x).float(), w_shape, cast(dy).float(), padding=pad)


def _scale_block(y):
    """One image's last 8 output channels scaled by (1 - 2^-8): a small systematic error on one tile of the destination."""
    y = y.clone()
    y[-1, -8:] *= 1.0 - 2.0 ** -8
    return y


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_c%d' % (s[1], s[2], s[3]))
def test_fprop_bound_accepts_rne_and_rejects_precision_bugs(shape):
    x, w, _, pad = _data(shape, 1)
    ref_old = F.conv2d(x.double(), w.double(), padding=pad)                  # today's reference: unrounded operands
    ref = F.conv2d(rne(x).double(), rne(w).double(), padding=pad)            # the exact row's reference
    good = _fprop(x, w, pad, rne)
    assert rel_err(good, ref) <= TOL_EXACT
    for bad in (_fprop(x, w, pad, trunc), _scale_block(good)):
        assert rel_err(bad, ref_old) <= OLD_TOL                               # the old rule lets it through ...
        assert rel_err(bad, ref) > TOL_EXACT                                  # ... the exact row does not


@pytest.mark.parametrize('shape', SHAPES[:2], ids=lambda s: '%dx%d_c%d' % (s[1], s[2], s[3]))
def test_dgrad_and_wgrad_bounds(shape):
    x, w, dy, pad = _data(shape, 2)
    N, H, W = shape[:3]
    ref_dx = torch.nn.grad.conv2d_input(x.shape, rne(w).double(), rne(dy).double(), padding=pad)
    ref_dw = torch.nn.grad.conv2d_weight(rne(x).double(), w.shape, rne(dy).double(), padding=pad)
    old_dx = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), padding=pad)
    old_dw = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), padding=pad)
    wtol = wgrad_tol(N, 1, H, W)
    assert rel_err(_dgrad(dy, w, x.shape, pad, rne), ref_dx) <= TOL_EXACT
    assert rel_err(_wgrad(x, dy, w.shape, pad, rne), ref_dw) <= wtol
    for bad in (_dgrad(dy, w, x.shape, pad, trunc), _scale_block(_dgrad(dy, w, x.shape, pad, rne))):
        assert rel_err(bad, old_dx) <= OLD_TOL
        assert rel_err(bad, ref_dx) > TOL_EXACT
    bad_dw = _wgrad(x, dy, w.shape, pad, trunc)
    assert rel_err(bad_dw, old_dw) <= OLD_TOL
    assert rel_err(bad_dw, ref_dw) > wtol


def test_wgrad_bound_formula():
    assert wgrad_tol(1, 1, 64, 64) == TOL_EXACT
    assert wgrad_tol(32, 1, 64, 64) == pytest.approx(TOL_EXACT * 2 ** 0.5)


def _split_k_fold(x, w, pad, splits, part_cast):
    """FPROP with the reduction (input channels) cut into `splits` slices, each slice's fp32 partial result through `part_cast`
    (the scratch), then added in split order in fp32."""
    xs, ws = torch.chunk(rne(x).float(), splits, dim=1), torch.chunk(rne(w).float(), splits, dim=1)
    out = torch.zeros(1)
    for a, b in zip(xs, ws):
        out = out + part_cast(F.conv2d(a, b, padding=pad)).float()
    return out


def test_split_k_fold_bound():
    x, w, _, pad = _data(SHAPES[0], 3)                                        # K = 25 x 264 = 6600
    ref_old = F.conv2d(x.double(), w.double(), padding=pad)
    ref = F.conv2d(rne(x).double(), rne(w).double(), padding=pad)
    good = _split_k_fold(x, w, pad, 4, lambda t: t)
    bad = _split_k_fold(x, w, pad, 4, lambda t: t.to(torch.bfloat16))
    assert rel_err(good, ref) <= TOL_EXACT
    assert rel_err(bad, ref_old) <= OLD_TOL
    assert rel_err(bad, ref) > TOL_EXACT


def test_statistics_epilogue_bound():
    for shape in SHAPES[:3]:
        x, w, _, pad = _data(shape, 4)
        ref = F.conv2d(rne(x).double(), rne(w).double(), padding=pad)
        ref_old = F.conv2d(x.double(), w.double(), padding=pad)
        acc = _fprop(x, w, pad, rne)                                           # the fp32 accumulators
        for r, tol in ((ref, TOL_EXACT), (ref_old, OLD_TOL)):
            want = [r.sum(dim=(2, 3)), (r * r).sum(dim=(2, 3))]
            good = [acc.double().sum(dim=(2, 3)), (acc.double() ** 2).sum(dim=(2, 3))]
            y16 = acc.to(torch.bfloat16).double()                               # the mutation: sums of the bf16-rounded outputs
            bad = [y16.sum(dim=(2, 3)), (y16 * y16).sum(dim=(2, 3))]
            assert all(rel_err(g, t) <= tol for g, t in zip(good, want))
            if tol == TOL_EXACT:
                assert rel_err(bad[0], want[0]) > TOL_EXACT
            else:
                assert all(rel_err(b, t) <= OLD_TOL for b, t in zip(bad, want))


@pytest.mark.parametrize('shape', SHAPES[:3], ids=lambda s: '%dx%d_c%d' % (s[1], s[2], s[3]))
def test_bf16_destination_bracket(shape):
    x, w, _, pad = _data(shape, 5)
    ref = F.conv2d(rne(x).double(), rne(w).double(), padding=pad)
    acc = _fprop(x, w, pad, rne)
    n_out, frac = bf16_bracket(acc.to(torch.bfloat16), ref)                   # correct: RNE of the fp32 accumulators
    assert n_out == 0 and frac <= RNE_MISMATCH
    assert rel_err(trunc(acc), ref) <= 1e-2                                  # the old rule on a truncated destination: passes
    n_out, frac = bf16_bracket(trunc(acc).to(torch.bfloat16), ref)           # truncated: still in the bracket, but not RNE
    assert frac > RNE_MISMATCH
    n_out, frac = bf16_bracket(_fprop(x, w, pad, trunc).to(torch.bfloat16), ref)    # truncated operands: outside the bracket
    assert n_out > 0
    n_out, _ = bf16_bracket(_scale_block(acc).to(torch.bfloat16), ref)
    assert n_out > 0
    poisoned = acc.to(torch.bfloat16)
    poisoned.view(-1)[7] = float('nan')
    assert bf16_bracket(poisoned, ref)[0] == 1


def test_bracket_and_ulp_helpers_at_the_edges():
    b = torch.tensor([1.0, -1.0, 0.0, 2.0 ** -126, -2.5], dtype=torch.float64)
    c16 = b.to(torch.bfloat16)
    assert bf16_bracket(c16, b) == (0.0, 0.0)                                # exact values: only themselves
    up = (c16.float().view(torch.int32) + 0x10000).view(torch.float32).to(torch.bfloat16)
    assert bf16_bracket(up[:1], b[:1], atol=0.0)[0] == 1                      # 1 ulp off an exactly representable result
    two = (c16.float().view(torch.int32) + 0x20000).view(torch.float32).to(torch.bfloat16)
    assert bf16_bracket(two[:1], b[:1])[0] == 1                               # 2 ulps off: outside the window's bracket too
    mid = torch.tensor([1.0 + 2.0 ** -8], dtype=torch.float64)               # halfway between 1 and 1 + 2^-7 (the bf16 ulp at 1)
    for v in (1.0, 1.0 + 2.0 ** -7):
        assert bf16_bracket(torch.tensor([v]).to(torch.bfloat16), mid)[0] == 0
    assert bf16_bracket(torch.tensor([1.0 + 2.0 ** -6]).to(torch.bfloat16), mid)[0] == 1
    neg = torch.tensor([-1.0 - 2.0 ** -8 - 2.0 ** -12], dtype=torch.float64)   # just past the midpoint: rounds away from zero
    assert bf16_bracket(torch.tensor([-1.0 - 2.0 ** -7]).to(torch.bfloat16), neg) == (0.0, 0.0)
    assert bf16_bracket(torch.tensor([-1.0]).to(torch.bfloat16), neg) == (0.0, 1.0)
    assert bf16_ulps_apart(c16, c16) == 0.0
    assert bf16_ulps_apart(c16[:1], up[:1]) == 1.0
    assert bf16_ulps_apart(torch.tensor([0.0]).to(torch.bfloat16), torch.tensor([-0.0]).to(torch.bfloat16)) == 0.0
    assert bf16_ulps_apart(torch.tensor([float('nan')]).to(torch.bfloat16), c16[:1]) == float('inf')
    r = torch.tensor(np.array([1.0, 2.0], dtype=np.float32))
    assert torch.equal(rne(r), r) and rne(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20])).item() == 1.0 + 2.0 ** -7


def test_bracket_window_near_zero():
    """An element that cancels to ~0 rounds an fp32 sum whose own error (~1e-7 of the largest element) is many bf16 ulps of the
    element: the window (TOL_EXACT of max|ref|) admits that, and nothing beyond it."""
    ref = torch.tensor([1.0, 3.0e-7, -2.0e-9], dtype=torch.float64)
    acc = ref.float() + torch.tensor([0.0, 4.0e-7, 1.0e-7])                    # fp32 sums 1e-7 .. 4e-7 off, far below TOL_EXACT
    assert bf16_bracket(acc.to(torch.bfloat16), ref) == (0.0, 2.0 / 3.0)
    assert bf16_bracket(acc.to(torch.bfloat16), ref, atol=0.0)[0] == 2.0       # the bare bracket rejects a correct kernel
    far = ref.float() + torch.tensor([0.0, 3.0 * TOL_EXACT, 0.0])
    assert bf16_bracket(far.to(torch.bfloat16), ref)[0] == 1.0
    a, b = acc.to(torch.bfloat16), (ref.float() - torch.tensor([0.0, 4.0e-7, 1.0e-7])).to(torch.bfloat16)
    assert bf16_ulps_apart(a, b) > 1.0 and bf16_apart(a, b, 2 * window(ref)) == 0.0
    one_up = (a.float().view(torch.int32) + 0x10000).view(torch.float32).to(torch.bfloat16)
    two_up = (a.float().view(torch.int32) + 0x20000).view(torch.float32).to(torch.bfloat16)
    assert bf16_apart(a[:1], one_up[:1]) == 0.0 and bf16_apart(a[:1], two_up[:1], 2 * window(ref)) == 1.0

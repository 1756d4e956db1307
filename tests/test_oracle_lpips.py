"""CPU checks of the LPIPS restatement (tests/oracle_lpips.py) by identities and hand-computed cases that do not depend on it being right,
of the best-of-N fold with lpips / eval_diversity and the parallel path's chunk bookkeeping, of the weight loader and of the converter."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import oracle_lpips as OL  # noqa: E402


def _frames(seed, n=2, H=64, W=64, C=3):
    return np.random.default_rng(seed).random((n, H, W, C))


# ---------------------------------------------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tap_sizes_are_the_published_ones():
    from video_prediction_amd.lpips import tap_sizes
    w = OL.make_weights(1)
    for (H, W), want in (((64, 64), [(15, 15), (7, 7), (3, 3), (3, 3), (3, 3)]), ((128, 128), [(31, 31), (15, 15), (7, 7), (7, 7), (7, 7)]),
                         ((48, 64), [(11, 15), (5, 7), (2, 3), (2, 3), (2, 3)])):
        taps = OL.trunk(_frames(0, 1, H, W), w)
        assert [t.shape[1:3] for t in taps] == want
        assert [t.shape[3] for t in taps] == [64, 192, 384, 256, 256]
        assert tap_sizes(H, W) == want


def test_distance_identities():
    w = OL.make_weights(2)
    a, b = _frames(3), _frames(4)
    assert np.all(OL.distance(a, a, w) == 0.0)
    dab, dba = OL.distance(a, b, w), OL.distance(b, a, w)
    assert np.array_equal(dab, dba)
    assert np.all(dab > 0)
    assert np.allclose(OL.lpips_metric(a.reshape(1, 2, 64, 64, 3), b.reshape(1, 2, 64, 64, 3), w), -dab.reshape(1, 2), rtol=0, atol=0)


def test_grey_frame_equals_its_tiling():
    w = OL.make_weights(5)
    a, b = _frames(6, C=1), _frames(7, C=1)
    assert np.array_equal(OL.distance(a, b, w), OL.distance(np.tile(a, (1, 1, 1, 3)), np.tile(b, (1, 1, 1, 3)), w))


def test_zero_convolutions_with_positive_biases_give_zero():
    w = OL.make_weights(8)
    for l in range(1, 6):
        w['conv%d_w' % l][:] = 0
        w['conv%d_b' % l] = np.abs(w['conv%d_b' % l]) + 0.1
    assert np.all(OL.distance(_frames(9), _frames(10), w) == 0.0)


def _one_channel_weights(w1, b1, wl, bl, lins):
    w = OL.make_weights(0, channels=(1, 1, 1, 1, 1))
    for l in range(1, 6):
        w['conv%d_w' % l][:] = w1 if l == 1 else wl
        w['conv%d_b' % l][:] = b1 if l == 1 else bl
        w['lin%d' % l][:] = lins[l - 1]
    return w


def test_hand_computed_one_channel_case():
    """One channel per layer.  All-ones frame: every scaled input is u_c = (1 - shift_c) / scale_c > 0, so with a constant positive conv1
    weight tap 1 is w1 * (taps inside the image) * sum_c u_c + b1: 11 x 11 taps in the interior, 9 x 9 in the corner (pad 2).  All-zero
    frame: u_c < 0, tap 1 is 0 after the ReLU, and with bias -0.5 behind it every later tap is 0 too.  A single channel normalises to 1
    where it is positive and to 0 where it is 0, so d = sum_l lin_l * mean (1 - 0)^2 = sum_l lin_l -- up to the 1e-10 in the
    normalisation: f / (f + 1e-10) falls short of 1 by 1e-10 / f, and every positive tap here is above 1, so d is within 2e-10 * sum_l lin_l
    below the hand value."""
    w1, b1 = 0.0078125, 0.25                                            # exact in float32, the dtype of the weight arrays
    lins = (0.5, 0.25, 0.125, 0.0625, 0.03125)
    w = _one_channel_weights(w1, b1, 1.0, -0.5, lins)
    ones, zeros = np.ones((1, 64, 64, 3)), np.zeros((1, 64, 64, 3))
    su = sum((1.0 - s) / c for s, c in zip((-.030, -.088, -.188), (.458, .448, .450)))
    t1 = OL.stem(ones, w)
    assert t1.shape == (1, 15, 15, 1)
    assert abs(t1[0, 7, 7, 0] - (w1 * 121 * su + b1)) < 1e-12
    assert abs(t1[0, 0, 0, 0] - (w1 * 81 * su + b1)) < 1e-12
    assert abs(t1[0, 0, 7, 0] - (w1 * 99 * su + b1)) < 1e-12
    wz = _one_channel_weights(w1, -b1, 1.0, -0.5, lins)                 # negative bias: the all-zero frame dies in conv1
    assert np.all(OL.stem(zeros, wz) == 0.0)
    assert all(np.all(t == 0.0) for t in OL.trunk(zeros, wz))
    assert all(np.all(t > 0.0) for t in OL.trunk(ones, wz))
    d = OL.distance(ones, zeros, wz)
    assert 0 <= sum(lins) - float(d[0]) < 2e-10 * sum(lins)
    assert abs(float(OL.distance_torch_f32(ones, zeros, wz)[0]) - sum(lins)) < 1e-6


def test_conv1_pads_with_zeros_in_the_scaled_space():
    """A frame equal to the constant that the affine maps to 0 is indistinguishable from the padding: tap 1 is relu(bias) everywhere.
    An all-zero frame is not (it maps to (-1 - shift) / scale != 0): its border outputs differ from the interior ones, which they would
    not if the zeros were padded before the affine."""
    w = OL.make_weights(11)
    const = np.broadcast_to((1.0 + OL.SHIFT) / 2.0, (1, 64, 64, 3))
    t = OL.stem(const, w)
    assert np.allclose(t, np.maximum(w['conv1_b'].astype(np.float64), 0.0), rtol=0, atol=1e-12)
    z = OL.conv2d(OL.preprocess(np.zeros((1, 64, 64, 3))), w['conv1_w'], w['conv1_b'], 4, 2)
    assert np.allclose(z[0, 3:12, 3:12], z[0, 7, 7], rtol=0, atol=1e-12)          # the interior is uniform ...
    assert np.abs(z[0, 0, 0] - z[0, 7, 7]).max() > 1e-3                           # ... and the corner is something else
    assert not np.allclose(OL.stem(np.zeros((1, 64, 64, 3)), w), t)


def test_float32_twin_follows_the_float64_oracle():
    w = OL.make_weights(12)
    for H, W, C in ((64, 64, 3), (48, 64, 1)):
        a, b = _frames(13, 3, H, W, C), _frames(14, 3, H, W, C)
        d64, d32 = OL.distance(a.astype(np.float32), b.astype(np.float32), w), OL.distance_torch_f32(a, b, w)
        assert np.abs(d32 - d64).max() / np.abs(d64).max() < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# best-of-N with lpips and diversity
# ---------------------------------------------------------------------------------------------------------------------------------
def _best_of_n_case(S, nd, seed):
    F, T1, B, H, W, C = 2, 3, 2, 32, 32, 3
    rng = np.random.default_rng(seed)
    target = rng.random((F, B, H, W, C))
    samples = rng.random((S, T1, B, H, W, C))
    w = OL.make_weights(seed + 1)
    lp = lambda a, b: OL.lpips_metric(a, b, w)
    mse = lambda a, b: ((a - b) ** 2).mean(axis=(-3, -2, -1))
    outs, mets = OL.best_of_n(target, samples, [('mse', mse), ('lpips', lp)], lp, nd)
    per = np.stack([lp(target, samples[s, -F:]) for s in range(S)])          # [S, F, B]
    return F, B, samples, w, outs, mets, per


@pytest.mark.parametrize('S,nd', [(5, 3), (3, 10), (4, 3)])
def test_best_of_n_with_lpips_and_diversity(S, nd):
    """The literal fold against its closed form: the kept sample is the arg-extremum of the time-mean (first one on ties), the average is the
    mean, and eval_diversity is the sum of d(sample i-1, sample i) over 0 < i <= min(nd, S-1) divided by nd -- also when S - 1 < nd."""
    F, B, samples, w, outs, mets, per = _best_of_n_case(S, nd, 20 + S)
    means = per.mean(1)                                                       # [S, B]
    for b in range(B):
        hi, lo = int(np.argmax(means[:, b])), int(np.argmin(means[:, b]))
        assert np.array_equal(mets['eval_lpips/max'][:, b], per[hi, :, b]) and np.array_equal(mets['eval_lpips/min'][:, b], per[lo, :, b])
        assert np.array_equal(outs['eval_gen_images_lpips/max'][:, b], samples[hi, :, b])
        assert np.array_equal(outs['eval_gen_images_lpips/min'][:, b], samples[lo, :, b])
    assert np.allclose(mets['eval_lpips/avg'], per.mean(0), rtol=1e-13, atol=0)
    assert np.all(mets['eval_lpips/max'] <= 0)
    want = np.zeros((F, B))
    for i in range(1, min(nd, S - 1) + 1):
        want += -OL.lpips_metric(samples[i - 1, -F:], samples[i, -F:], w)
    assert np.allclose(mets['eval_diversity'], want / nd, rtol=1e-13, atol=0)
    assert np.all(mets['eval_diversity'] > 0)


@pytest.mark.parametrize('num_samples,S,nd', [(10, 4, 5), (10, 4, 10), (10, 4, 3), (3, 4, 10), (8, 4, 8), (9, 2, 4), (5, 1, 2), (100, 10, 10)])
def test_chunk_bookkeeping_adds_the_reference_pairs_in_order(num_samples, S, nd):
    """The parallel path's controls (savp_model.chunk_controls) through the device-side gate restated in oracle_lpips.chunked_diversity:
    exactly the pairs (i-1, i), 0 < i <= nd, i < num_samples, ascending -- across chunk boundaries, with a padded last chunk, and with
    fewer samples than nd."""
    from video_prediction_amd.models.savp_model import chunk_controls
    controls = chunk_controls(num_samples, S)
    assert sum(nv for nv, _ in controls) == num_samples and [b for _, b in controls] == list(range(0, num_samples, S))
    assert all(nv == S for nv, _ in controls[:-1]) and 1 <= controls[-1][0] <= S
    rng = np.random.default_rng(num_samples * 100 + S * 10 + nd)
    table = rng.random((num_samples, num_samples, 2, 3))
    div, pairs = OL.chunked_diversity(lambda i, j: table[i, j], controls, S, nd, 2, 3)
    want_pairs = [(i - 1, i) for i in range(1, num_samples) if i <= nd]
    assert pairs == want_pairs
    want = np.zeros((2, 3))
    for i, j in want_pairs:
        want = want + table[i, j]
    assert np.array_equal(div, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# loader and converter
# ---------------------------------------------------------------------------------------------------------------------------------
def test_loader_accepts_a_good_file_and_refuses_bad_ones(tmp_path):
    from video_prediction_amd import lpips as LP
    w = OL.make_weights(30)
    path = str(tmp_path / 'w.npz')
    np.savez(path, **w)
    got = LP.load_weights(path)
    assert sorted(got) == sorted(LP.expected_arrays()) and all(np.array_equal(got[k], w[k]) for k in w)

    def refused(arrays, word):
        p = str(tmp_path / 'bad.npz')
        np.savez(p, **arrays)
        with pytest.raises(ValueError, match=word):
            LP.load_weights(p)
    bad = dict(w)
    del bad['conv3_b']
    refused(bad, 'missing array conv3_b')
    refused(dict(w, conv6_w=np.zeros(3, np.float32)), 'unexpected array conv6_w')
    refused(dict(w, conv2_w=w['conv2_w'].transpose(0, 1, 3, 2)), 'conv2_w has shape')
    refused(dict(w, lin4=w['lin4'][:-1]), 'lin4 has shape')
    refused(dict(w, conv1_w=w['conv1_w'].astype(np.float64)), 'conv1_w is float64')
    neg = w['lin2'].copy()
    neg[5] = -1e-3
    refused(dict(w, lin2=neg), 'lin2 has negative entries')


def test_weight_path_comes_from_the_keyword_or_the_environment(monkeypatch):
    from video_prediction_amd import lpips as LP
    monkeypatch.delenv(LP.ENV_VAR, raising=False)
    assert LP.configured_path(None) is None and LP.configured_path('a.npz') == 'a.npz'
    monkeypatch.setenv(LP.ENV_VAR, 'env.npz')
    assert LP.configured_path(None) == 'env.npz' and LP.configured_path('a.npz') == 'a.npz'


def test_stem_weight_pack_layout():
    """[ky][kp][co][e] holds W[ky][kx][c][co] at kx * 3 + c = 2 kp + e, zeros behind the 33 real entries of a kernel row."""
    from video_prediction_amd import lpips as LP
    w = OL.make_weights(31)['conv1_w']
    p = LP.pack_stem_weights(w)
    assert p.shape == (11, 18, 64, 2) and p.dtype == np.float32
    for ky, kx, c, co in ((0, 0, 0, 0), (3, 10, 2, 63), (10, 5, 1, 17), (7, 0, 1, 40)):
        j = kx * 3 + c
        assert p[ky, j // 2, co, j % 2] == w[ky, kx, c, co]
    assert np.all(p[:, 16, :, 1] == 0) and np.all(p[:, 17] == 0)


def test_converter_round_trip(tmp_path):
    import torch
    from scripts import convert_lpips_weights as CV
    from video_prediction_amd import lpips as LP
    w = OL.make_weights(32)
    alex, lin = {}, {}
    for l, idx in enumerate((0, 3, 6, 8, 10), 1):
        alex['features.%d.weight' % idx] = torch.from_numpy(w['conv%d_w' % l].transpose(3, 2, 0, 1).copy())      # HWIO -> OIHW
        alex['features.%d.bias' % idx] = torch.from_numpy(w['conv%d_b' % l])
        lin['lin%d.model.1.weight' % (l - 1)] = torch.from_numpy(w['lin%d' % l]).view(1, -1, 1, 1)
    alex['classifier.1.weight'] = torch.zeros(4, 4)                          # the rest of the torchvision model is ignored
    pa, pl, out = str(tmp_path / 'alexnet-owt-test.pth'), str(tmp_path / 'alex.pth'), str(tmp_path / 'lpips.npz')
    torch.save(alex, pa)
    torch.save(lin, pl)
    CV.main(['--alexnet', pa, '--lin', pl, '--output', out])
    got = LP.load_weights(out)
    assert sorted(got) == sorted(w) and all(np.array_equal(got[k], w[k]) for k in w)
    del lin['lin3.model.1.weight']
    with pytest.raises(KeyError, match='lin3.model.1.weight'):
        CV.convert(alex, lin)


# ---------------------------------------------------------------------------------------------------------------------------------
# the stem kernel's index arithmetic (csrc/lpips.hip), replayed in numpy
# ---------------------------------------------------------------------------------------------------------------------------------
def _stem_by_the_kernels_indexing(frames, w):
    """lpips_stem_kernel's strips, LDS patch [rows_in][RS], A address (4 oy + ky) * RS + 12 ox + k and packed-weight address
    [ky][k / 2][co][k % 2], with float64 arithmetic: k runs over all 36 entries of a padded kernel row."""
    from video_prediction_amd import lpips as LP
    wp = LP.pack_stem_weights(w['conv1_w']).astype(np.float64)                # [11][18][64][2]
    N, H, W, C = frames.shape
    Ho, Wo = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    R = 1 if Wo >= 128 else 128 // Wo
    RS = (Wo - 1) * 12 + 36
    out = np.zeros((N, Ho, Wo, 64))
    for n in range(N):
        for oy0 in range(0, Ho, R):
            rows_out = min(R, Ho - oy0)
            rows_in = (rows_out - 1) * 4 + 11
            patch = np.zeros(rows_in * RS)
            for i in range(rows_in * RS):
                r, q = divmod(i, RS)
                xc, c = divmod(q, 3)
                iy, ix = oy0 * 4 - 2 + r, xc - 2
                if 0 <= iy < H and 0 <= ix < W:
                    patch[i] = ((2.0 * frames[n, iy, ix, c if C == 3 else 0] - 1.0) - OL.SHIFT[c]) / OL.SCALE[c]
            patch = patch.reshape(rows_in, RS)
            for m in range(rows_out * Wo):
                oyl, ox = divmod(m, Wo)
                acc = np.zeros(64)
                for ky in range(11):
                    a = patch[oyl * 4 + ky, ox * 12:ox * 12 + 36]                  # never past the row: RS = 12 (Wo - 1) + 36
                    assert a.shape == (36,)
                    for k in range(36):
                        acc += a[k] * wp[ky, k // 2, :, k % 2]
                out[n, oy0 + oyl, ox] = acc
    return np.maximum(out + w['conv1_b'], 0.0)


@pytest.mark.parametrize('shape', [(32, 32, 3), (24, 40, 1), (64, 64, 3)])
def test_stem_kernel_index_arithmetic(shape):
    H, W, C = shape
    w = OL.make_weights(40)
    frames = _frames(41, 1, H, W, C)
    got, ref = _stem_by_the_kernels_indexing(frames, w), OL.stem(frames, w)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()

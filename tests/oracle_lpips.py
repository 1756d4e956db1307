"""float64 numpy restatement of the LPIPS distance the reference evaluates (video_prediction/metrics.py:17-24 calls lpips_tf.lpips with its
defaults: net-lin, alex, version 0.1), a torch-CPU float32 twin of it, and a literal restatement of the reference's best-of-N fold with the
lpips metric and eval_diversity (base_model.py:176-226).  For the tests of csrc/lpips.hip and video_prediction_amd/lpips.py.

UNPINNED: neither lpips_tf's frozen graph nor the published weights are available to this project's tests.  This file is written from the
published architecture (the AlexNet `features` trunk of torchvision; the LPIPS v0.1 scaling layer, unit normalisation and 1x1 linear
heads), not from any code; tests/test_oracle_lpips.py checks it against identities and a hand-computed case that do not depend on this
restatement being right.

  1. a 1-channel frame is tiled to 3 channels (metrics.py:19-21); v in [0, 1] -> x = 2 v - 1 -> (x - shift_c) / scale_c with
     shift = (-.030, -.088, -.188), scale = (.458, .448, .450).  conv1's zero padding is applied AFTER this step.
  2. conv1 11x11 /4 pad 2 (3 -> 64), ReLU = tap 1; max-pool 3x3 /2 (no padding, floor); conv2 5x5 pad 2 (-> 192), ReLU = tap 2;
     max-pool 3x3 /2; conv3 3x3 pad 1 (-> 384), ReLU = tap 3; conv4 3x3 pad 1 (-> 256), ReLU = tap 4; conv5 3x3 pad 1 (-> 256), ReLU = tap 5.
     Cross-correlations with bias.
  3. d = sum_l mean_{h,w} sum_c lin_l[c] (fa_l / (|fa_l|_c + 1e-10) - fb_l / (|fb_l|_c + 1e-10))^2.
The reference's metric `lpips` is -d (larger = better); eval_diversity accumulates +d between successive samples.
"""
import numpy as np

SHIFT = np.array([-.030, -.088, -.188])
SCALE = np.array([.458, .448, .450])
CHANNELS = (64, 192, 384, 256, 256)
KERNELS = (11, 5, 3, 3, 3)
STRIDES = (4, 1, 1, 1, 1)
PADS = (2, 2, 1, 1, 1)
POOL_AFTER = (True, True, False, False, False)


def make_weights(seed=0, channels=CHANNELS):
    """Test weights from a seeded generator: He-scaled normal convolutions (ReLUs stay alive), small biases, lin uniform in [0, 1).
    channels: other widths serve the hand-computed cases (the product accepts the published widths only)."""
    rng = np.random.default_rng(seed)
    out, cin = {}, 3
    for l, (k, c) in enumerate(zip(KERNELS, channels), 1):
        out['conv%d_w' % l] = (rng.standard_normal((k, k, cin, c)) * np.sqrt(2.0 / (k * k * cin))).astype(np.float32)
        out['conv%d_b' % l] = (0.05 * rng.standard_normal(c)).astype(np.float32)
        out['lin%d' % l] = rng.random(c).astype(np.float32)
        cin = c
    return out


def preprocess(frames):
    """[..., H, W, 1 | 3] in [0, 1] -> the trunk's input [..., H, W, 3], float64."""
    v = np.asarray(frames, np.float64)
    if v.shape[-1] == 1:
        v = np.tile(v, (1,) * (v.ndim - 1) + (3,))
    return ((2.0 * v - 1.0) - SHIFT) / SCALE


def conv2d(x, w, b, stride, pad):
    """Cross-correlation of x [N, H, W, Ci] with w [kh, kw, Ci, Co] (HWIO), zero padding `pad` on every side, + b."""
    x = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    kh, kw = w.shape[:2]
    N, H, W, Ci = x.shape
    Ho, Wo = (H - kh) // stride + 1, (W - kw) // stride + 1
    out = np.zeros((N, Ho, Wo, w.shape[3]), x.dtype)
    for dy in range(kh):
        for dx in range(kw):
            patch = x[:, dy:dy + (Ho - 1) * stride + 1:stride, dx:dx + (Wo - 1) * stride + 1:stride]
            out += patch @ w[dy, dx].astype(x.dtype)
    return out + b.astype(x.dtype)


def maxpool3s2(x):
    N, H, W, C = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = np.full((N, Ho, Wo, C), -np.inf, x.dtype)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, x[:, dy:dy + 2 * (Ho - 1) + 1:2, dx:dx + 2 * (Wo - 1) + 1:2])
    return out


def stem(frames, weights):
    """Tap 1 of frames [N, H, W, 1 | 3]."""
    return np.maximum(conv2d(preprocess(frames), weights['conv1_w'], weights['conv1_b'], 4, 2), 0.0)


def trunk(frames, weights):
    """The five ReLU taps [N, h_l, w_l, C_l] (float64) of frames [N, H, W, 1 | 3] in [0, 1]."""
    x = preprocess(frames)
    taps = []
    for l in range(5):
        x = np.maximum(conv2d(x, weights['conv%d_w' % (l + 1)], weights['conv%d_b' % (l + 1)], STRIDES[l], PADS[l]), 0.0)
        taps.append(x)
        if POOL_AFTER[l]:
            x = maxpool3s2(x)
    return taps


def head(taps_a, taps_b, weights):
    """d [N] from two lists of taps."""
    d = 0.0
    for l, (fa, fb) in enumerate(zip(taps_a, taps_b), 1):
        na = fa / (np.sqrt((fa * fa).sum(-1, keepdims=True)) + 1e-10)
        nb = fb / (np.sqrt((fb * fb).sum(-1, keepdims=True)) + 1e-10)
        d = d + (((na - nb) ** 2) * weights['lin%d' % l].astype(fa.dtype)).sum(-1).mean(axis=(1, 2))
    return d


def distance(a, b, weights):
    """The LPIPS distance [N] (float64) between frames a and b [N, H, W, 1 | 3] in [0, 1]."""
    return head(trunk(a, weights), trunk(b, weights), weights)


def lpips_metric(a, b, weights):
    """metrics.py:17-24 on [..., H, W, C]: minus the distance, leading shape kept."""
    a, b = np.asarray(a), np.asarray(b)
    lead = a.shape[:-3]
    return -distance(a.reshape((-1,) + a.shape[-3:]), b.reshape((-1,) + b.shape[-3:]), weights).reshape(lead)


def distance_torch_f32(a, b, weights):
    """The float32 twin on torch CPU kernels (F.conv2d / F.max_pool2d): same arithmetic, torch's summation orders.  Returns float32 [N]."""
    import torch
    import torch.nn.functional as Fn

    def taps_of(v):
        x = torch.as_tensor(np.asarray(v, np.float32))
        if x.shape[-1] == 1:
            x = x.repeat(1, 1, 1, 3)
        x = ((2.0 * x - 1.0) - torch.tensor(SHIFT, dtype=torch.float32)) / torch.tensor(SCALE, dtype=torch.float32)
        x = x.permute(0, 3, 1, 2).contiguous()
        taps = []
        for l in range(5):
            w = torch.as_tensor(weights['conv%d_w' % (l + 1)]).permute(3, 2, 0, 1).contiguous()
            x = torch.relu(Fn.conv2d(x, w, torch.as_tensor(weights['conv%d_b' % (l + 1)]), stride=STRIDES[l], padding=PADS[l]))
            taps.append(x)
            if POOL_AFTER[l]:
                x = Fn.max_pool2d(x, 3, 2)
        return taps
    d = 0.0
    for l, (fa, fb) in enumerate(zip(taps_of(a), taps_of(b)), 1):
        na = fa / (fa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        nb = fb / (fb.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        lin = torch.as_tensor(weights['lin%d' % l]).view(1, -1, 1, 1)
        d = d + ((na - nb).pow(2) * lin).sum(1).mean(dim=(1, 2))
    return d.numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# best-of-N with lpips and diversity
# ---------------------------------------------------------------------------------------------------------------------------------
def best_of_n(target, samples, metric_fns, lpips_fn, num_samples_for_diversity, dtype=np.float64):
    """base_model.py:176-226 literally, sample after sample.  target [F, B, H, W, C] (future frames); samples [S, T1, B, H, W, C] (whole
    unrolls, the last F frames are the future); metric_fns: [(name, fn(target, pred) -> [F, B])], 'lpips' among them or not;
    lpips_fn(a, b) -> [F, B] (minus the distance).  Returns (eval_outputs, eval_metrics) without 'eval_images'."""
    S, T1, B = samples.shape[:3]
    F = target.shape[0]
    a = {}
    for name, _ in metric_fns:                                             # initializer (:203-213)
        a['eval_gen_images_%s/min' % name] = np.zeros(samples.shape[1:], dtype)
        a['eval_gen_images_%s/sum' % name] = np.zeros(samples.shape[1:], dtype)
        a['eval_gen_images_%s/max' % name] = np.zeros(samples.shape[1:], dtype)
        a['eval_%s/min' % name] = np.full((F, B), np.inf, dtype)
        a['eval_%s/sum' % name] = np.zeros((F, B), dtype)
        a['eval_%s/max' % name] = np.full((F, B), -np.inf, dtype)
    a['eval_diversity'] = np.zeros((F, B), dtype)
    a['eval_sample_ind'] = 0
    a['eval_pred_images_last'] = np.zeros((F,) + samples.shape[2:], dtype)

    def where_axis1(cond, x, y):
        c = cond.reshape((1, -1) + (1,) * (x.ndim - 2))
        return np.where(c, x, y)

    for s in range(S):                                                     # accum_gen_images_and_metrics_fn (:176-201)
        gen_images_sample = samples[s].astype(dtype)
        pred_images_sample = gen_images_sample[-F:]
        for name, fn in metric_fns:
            metric = np.asarray(fn(target, pred_images_sample), dtype)
            cond_min = metric.mean(0) < a['eval_%s/min' % name].mean(0)
            cond_max = metric.mean(0) > a['eval_%s/max' % name].mean(0)
            a['eval_%s/min' % name] = where_axis1(cond_min, metric, a['eval_%s/min' % name])
            a['eval_%s/sum' % name] = metric + a['eval_%s/sum' % name]
            a['eval_%s/max' % name] = where_axis1(cond_max, metric, a['eval_%s/max' % name])
            a['eval_gen_images_%s/min' % name] = where_axis1(cond_min, gen_images_sample, a['eval_gen_images_%s/min' % name])
            a['eval_gen_images_%s/sum' % name] = gen_images_sample + a['eval_gen_images_%s/sum' % name]
            a['eval_gen_images_%s/max' % name] = where_axis1(cond_max, gen_images_sample, a['eval_gen_images_%s/max' % name])
        if 0 < a['eval_sample_ind'] <= num_samples_for_diversity:
            a['eval_diversity'] = -np.asarray(lpips_fn(a['eval_pred_images_last'], pred_images_sample), dtype) + a['eval_diversity']
        a['eval_sample_ind'] = 1 + a['eval_sample_ind']
        a['eval_pred_images_last'] = pred_images_sample
    outs, mets = {}, {}
    for name, _ in metric_fns:                                             # (:219-226)
        outs['eval_gen_images_%s/min' % name] = a['eval_gen_images_%s/min' % name]
        outs['eval_gen_images_%s/avg' % name] = a['eval_gen_images_%s/sum' % name] / float(S)
        outs['eval_gen_images_%s/max' % name] = a['eval_gen_images_%s/max' % name]
        mets['eval_%s/min' % name] = a['eval_%s/min' % name]
        mets['eval_%s/avg' % name] = a['eval_%s/sum' % name] / float(S)
        mets['eval_%s/max' % name] = a['eval_%s/max' % name]
    mets['eval_diversity'] = a['eval_diversity'] / float(num_samples_for_diversity)
    return outs, mets


def chunked_diversity(pair_distance, controls, S, nd, F, B):
    """What the parallel path's launch sequence does with the {n_valid, base} words of one chunk after another (csrc/lpips.hip: the gate of
    savp_lpips_head and savp_lpips_diversity_add, and the taps kept from a chunk's last sample), in numpy: pair_distance(i, j) -> [F, B] is
    the distance between samples i and j.  Returns the sum before the division by nd, and the list of pairs that were added."""
    div = np.zeros((F, B))
    pairs = []
    kept = None                                       # global index of the sample whose taps the previous chunk copied aside
    for n_valid, base in controls:
        dv = {}
        for s in range(S):                            # the head launches: slot s is written only when the gate passes
            if s < n_valid and 0 < base + s <= nd:
                prev = kept if s == 0 else base + s - 1
                dv[s] = (prev, base + s)
        for s in range(n_valid):                      # savp_lpips_diversity_add, ascending
            if 0 < base + s <= nd:
                i, j = dv[s]
                div = div + pair_distance(i, j)
                pairs.append((i, j))
        kept = base + S - 1                           # slot S-1 of this chunk, valid or padding
    return div, pairs

"""LPIPS on the HIP path: the learned perceptual distance of the reference's metrics.py:17-24 (lpips_tf defaults: AlexNet trunk, linear
heads, version 0.1), computed by csrc/lpips.hip and savp_conv.

The network weights are not part of this repository; the user brings them as one .npz (scripts/convert_lpips_weights.py writes it from the
torchvision AlexNet state dict and the lpips package's v0.1 linear layers).  Parity with lpips_tf's frozen graph is unpinned: that graph
is an export of the same PyTorch weights, but it has never been run against this code.

    net = Lpips(load_weights(path), device)
    fa, fb = net.feature_set(n_frames, H, W), net.feature_set(n_frames, H, W)
    net.features(frames_a, fa); net.features(frames_b, fb)      # frames: [N0, N1, H, W, C] in [0, 1], C = 1 | 3
    net.distance(fa, fb, out, sign=-1.0)                        # out [n_frames]: -d, the reference's `lpips` metric
"""
import os

import numpy as np
import torch

from . import kernels as K
from . import lib

ENV_VAR = 'SAVP_LPIPS_WEIGHTS'
CHANNELS = (64, 192, 384, 256, 256)
KERNELS = (11, 5, 3, 3, 3)


def expected_arrays():
    """{name: shape} of the weight file: HWIO convolution weights, biases, the non-negative 1x1 `lin` weights of the five taps."""
    out, cin = {}, 3
    for l, (k, c) in enumerate(zip(KERNELS, CHANNELS), 1):
        out['conv%d_w' % l] = (k, k, cin, c)
        out['conv%d_b' % l] = (c,)
        out['lin%d' % l] = (c,)
        cin = c
    return out


def check_weights(arrays):
    """Refuse a missing, extra or mis-shaped array (naming it) and negative `lin` entries (LPIPS clamps them at training time: a negative
    entry means a wrong file).  Returns {name: float32 ndarray}."""
    want = expected_arrays()
    missing = sorted(set(want) - set(arrays))
    if missing:
        raise ValueError('LPIPS weights: missing array %s' % ', '.join(missing))
    extra = sorted(set(arrays) - set(want))
    if extra:
        raise ValueError('LPIPS weights: unexpected array %s' % ', '.join(extra))
    out = {}
    for name in sorted(want):
        v = np.asarray(arrays[name])
        if tuple(v.shape) != want[name]:
            raise ValueError('LPIPS weights: %s has shape %r, expected %r' % (name, tuple(v.shape), want[name]))
        if v.dtype != np.float32:
            raise ValueError('LPIPS weights: %s is %s, expected float32' % (name, v.dtype))
        if not np.all(np.isfinite(v)):
            raise ValueError('LPIPS weights: %s has non-finite entries' % name)
        if name.startswith('lin') and (v < 0).any():
            raise ValueError('LPIPS weights: %s has negative entries (not an LPIPS linear layer)' % name)
        out[name] = np.ascontiguousarray(v)
    return out


def load_weights(path):
    with np.load(path, allow_pickle=False) as f:
        return check_weights({k: f[k] for k in f.files})


def configured_path(explicit=None):
    """The weight file in force: the model-class keyword lpips_weights=, else the environment variable, else None (LPIPS off)."""
    return explicit or os.environ.get(ENV_VAR) or None


def pack_stem_weights(w):
    """conv1 HWIO [11, 11, 3, 64] -> [ky][kp = 18][co][2]: kernel rows of 33 (kx, c) values zero-padded to 36, consecutive pairs
    interleaved per output channel (include/savp_hip.h savp_lpips_stem)."""
    w = np.asarray(w, np.float32).reshape(11, 33, 64)
    rows = np.zeros((11, lib.LPIPS_STEM_KROW, 64), np.float32)
    rows[:, :33] = w
    return np.ascontiguousarray(rows.reshape(11, lib.LPIPS_STEM_KROW // 2, 2, 64).transpose(0, 1, 3, 2))


def tap_sizes(H, W):
    """[(h, w)] of the five taps."""
    h1, w1 = (H + 4 - 11) // 4 + 1, (W + 4 - 11) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    if min(h3, w3) < 1:
        raise ValueError('LPIPS: %dx%d frames are too small for the AlexNet trunk' % (H, W))
    return [(h1, w1), (h2, w2), (h3, w3), (h3, w3), (h3, w3)]


class FeatureSet(object):
    """The five ReLU taps of n frames: contiguous [n, h_l, w_l, C_l] tensors."""

    def __init__(self, n, H, W, device):
        self.n, self.H, self.W = int(n), int(H), int(W)
        self.taps = [torch.empty(self.n, h, w, c, device=device) for (h, w), c in zip(tap_sizes(H, W), CHANNELS)]


class Lpips(object):
    """Packed weights, per-shape workspaces and the launch sequences.  Always fp32: kernels.PRECISION does not apply to a metric."""

    def __init__(self, weights, device):
        w = check_weights(weights)
        self.device = dev = torch.device(device)
        self.stem_w = torch.from_numpy(pack_stem_weights(w['conv1_w'])).to(dev)
        self.bias = [torch.from_numpy(w['conv%d_b' % l]).to(dev) for l in range(1, 6)]
        self.lin = [torch.from_numpy(w['lin%d' % l]).to(dev) for l in range(1, 6)]
        self.wt = [None]
        for l in range(2, 6):                                        # savp_conv's FPROP operand WT[Cy][taps * Cx], packed once
            src = torch.from_numpy(w['conv%d_w' % l]).to(dev)
            wt = torch.empty(src.numel(), device=dev)
            K.pack_weights(src, wt=wt)
            self.wt.append(wt)
        torch.cuda.synchronize(dev)                                  # src tensors die here
        self._pool = {}

    def feature_set(self, n, H, W):
        return FeatureSet(n, H, W, self.device)

    def _pools(self, fs):
        key = (fs.n, fs.H, fs.W)
        if key not in self._pool:
            (_, _), (h2, w2), (h3, w3) = tap_sizes(fs.H, fs.W)[:3]
            self._pool[key] = (torch.empty(fs.n, h2, w2, CHANNELS[0], device=self.device),
                               torch.empty(fs.n, h3, w3, CHANNELS[1], device=self.device))
        return self._pool[key]

    def features(self, frames, fs):
        """frames [N0, N1, H, W, C] (contiguous frames; a time-major slice is fine) -> fs.taps; frame (i0, i1) is row i0 * N1 + i1."""
        N0, N1, H, W, C = frames.shape
        if N0 * N1 != fs.n or (H, W) != (fs.H, fs.W):
            raise ValueError('Lpips.features: frames %r do not fit the feature set (%d frames of %dx%d)' % (tuple(frames.shape), fs.n, fs.H, fs.W))
        t, (p1, p2) = fs.taps, self._pools(fs)
        K.lpips_stem(frames, self.stem_w, self.bias[0], t[0])
        K.lpips_maxpool3s2(t[0], p1)
        self._conv(2, p1, t[1])
        K.lpips_maxpool3s2(t[1], p2)
        self._conv(3, p2, t[2])
        self._conv(4, t[2], t[3])
        self._conv(5, t[3], t[4])
        return fs

    def _conv(self, l, x, y):
        k = KERNELS[l - 1]
        K.conv(lib.CONV_FPROP, K.ConvGeom((k, k), (1, 1), (k // 2, k // 2)), x, y, self.wt[l - 1], bias=self.bias[l - 1],
               act=lib.ACT_LRELU, alpha=0.0, precision=0)

    def distance(self, fa, fb, out, sign=1.0):
        """out[i] = sign * d(frame i of fa, frame i of fb); out: contiguous, fa.n elements."""
        K.lpips_head(fa.taps, fb.taps, self.lin, out, sign, 1, fa.n, fa.n, fb.n, fb.n, fa.n)

    def head(self, fa, fb, out, sign, **kw):
        """kernels.lpips_head with this network's `lin` weights (the engine's frame mappings)."""
        K.lpips_head(fa.taps, fb.taps, self.lin, out, sign, **kw)

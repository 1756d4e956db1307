#!/usr/bin/env python
"""Write the LPIPS weight file video_prediction_amd/lpips.py reads (host only; no GPU, no network).

    python scripts/convert_lpips_weights.py --alexnet alexnet-owt-*.pth --lin alex.pth --output lpips_alex_v0.1.npz
    SAVP_LPIPS_WEIGHTS=lpips_alex_v0.1.npz python scripts/evaluate.py ...

--alexnet: torchvision's AlexNet state dict, keys features.{0,3,6,8,10}.{weight,bias} (OIHW).
--lin:     the lpips package's v0.1 linear layers for `alex`, keys lin{0..4}.model.1.weight of shape [1, C, 1, 1].
The output holds conv{1..5}_w (HWIO), conv{1..5}_b and lin{1..5}, float32.  Parity with lpips_tf's frozen graph (what the reference
calls) is unpinned: that graph is an export of these same PyTorch weights, but it has not been run against this code.
"""
from __future__ import absolute_import, division, print_function

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FEATURE_INDICES = (0, 3, 6, 8, 10)       # the convolutions inside torchvision's alexnet.features


def _np(v):
    return np.asarray(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, dtype=np.float32)


def convert(alexnet_state, lin_state):
    """The two state dicts -> {name: float32 array} in the layout of video_prediction_amd.lpips.expected_arrays (checked)."""
    from video_prediction_amd.lpips import check_weights
    out = {}
    for l, idx in enumerate(FEATURE_INDICES, 1):
        for part in ('weight', 'bias'):
            key = 'features.%d.%s' % (idx, part)
            if key not in alexnet_state:
                raise KeyError('--alexnet: no %s (not a torchvision AlexNet state dict)' % key)
        out['conv%d_w' % l] = np.ascontiguousarray(_np(alexnet_state['features.%d.weight' % idx]).transpose(2, 3, 1, 0))     # OIHW -> HWIO
        out['conv%d_b' % l] = _np(alexnet_state['features.%d.bias' % idx])
        key = 'lin%d.model.1.weight' % (l - 1)
        if key not in lin_state:
            raise KeyError('--lin: no %s (not the lpips package\'s linear layers)' % key)
        lin = _np(lin_state[key])
        if lin.ndim != 4 or lin.shape[0] != 1 or lin.shape[2:] != (1, 1):
            raise ValueError('--lin: %s has shape %r, expected [1, C, 1, 1]' % (key, lin.shape))
        out['lin%d' % l] = np.ascontiguousarray(lin.reshape(-1))
    return check_weights(out)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--alexnet', required=True, help='torchvision AlexNet state dict (alexnet-owt-*.pth)')
    parser.add_argument('--lin', required=True, help="the lpips package's v0.1 linear layers (weights/v0.1/alex.pth)")
    parser.add_argument('--output', required=True, help='the .npz to write')
    args = parser.parse_args(argv)
    import torch
    arrays = convert(torch.load(args.alexnet, map_location='cpu'), torch.load(args.lin, map_location='cpu'))
    np.savez(args.output, **arrays)
    print('wrote %s: %s' % (args.output, ', '.join('%s%r' % (k, v.shape) for k, v in sorted(arrays.items()))))


if __name__ == '__main__':
    main()

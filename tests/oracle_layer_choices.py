"""The generator's other layer choices for the fp64 oracle: downsample_layer in (conv2d, conv_pool2d_v2), upsample_layer in (deconv2d,
upsample_conv2d_v2), activation_layer = elu (oracle/savp.py refuses them and stays as it is).

install(monkeypatch) replaces oracle.savp._norm_act, _downsample and _upsample; savp_cell_call looks the names up at call time, so
generator_fn and oracle.train.train_step then run the chosen layers.  With the three defaults every replacement hands over to the function it
replaced.  install() installs tests/oracle_layer_norm first (layer norm + ELU is a combination of its own), so call this one alone or last.

Reference semantics (video_prediction/ops.py, models/savp_model.py):
  * get_downsample_layer('conv2d') is ops.conv2d (:494-550), called with strides = (2, 2) and the default padding 'SAME' (savp_model.py:
    461-462): tf.nn.conv2d, variables <scope>/conv2d/{kernel [k, k, Cin, F], bias}.
  * get_upsample_layer('deconv2d') is ops.deconv2d (:553-589): tf.nn.conv2d_transpose with output 2H x 2W, 'SAME', variables
    <scope>/deconv2d/{kernel [k, k, F, Cin], bias} -- output channels before input channels.
  * conv_pool2d_v2 (:859-892): conv2d with strides 1, then pool2d(avg, pool = strides = (2, 2)), then the bias; variables under the scope
    'conv_pool2d'.  upsample_conv2d_v2 (:722-761): upsample2d_v2 (a 'VALID' conv2d_transpose of every channel with the bilinear kernel,
    :622-640), conv2d with 'FULL' padding, the crop of :746-751, then the bias; variables under 'upsample_conv2d'.
  * get_activation_layer('elu') is tf.nn.elu: z > 0 ? z : exp(z) - 1, applied after norm_layer at every site that applies relu by default
    (savp_model.py:464,478,500,513,526,538,565,628).  The encoders and discriminators do not read it.
"""
import numpy as np
import torch

import oracle.savp as OS
from oracle import ops
from tests import oracle_layer_norm as LN

_downsample_orig = OS._downsample
_upsample_orig = OS._upsample


def elu(z):
    """tf.nn.elu."""
    return torch.where(z > 0, z, torch.expm1(z))


def norm_act(vs, h, hp):
    """SAVPCell's norm_layer + activation_layer."""
    if hp.activation_layer == 'relu':
        return LN.norm_act(vs, h, hp)
    if hp.activation_layer != 'elu':
        raise ValueError('Invalid activation layer %s' % hp.activation_layer)
    if hp.norm_layer != 'none':
        h = LN.norm(vs, h, hp.norm_layer)
    return elu(h)


def deconv2d(inputs, kernel, bias=None, strides=(2, 2)):
    """ops.deconv2d with its bias (oracle.ops.deconv2d is the bias-free conv2d_transpose)."""
    out = ops.deconv2d(inputs, kernel, strides=strides, padding='SAME')
    if bias is not None:
        out = out + bias
    return out


def conv_pool2d_v2(inputs, kernel, bias=None, strides=(2, 2)):
    """ops.py:859-892."""
    if inputs.shape[1] % strides[0] or inputs.shape[2] % strides[1]:
        raise NotImplementedError("The height and width of the input should be an integer multiple of the respective stride.")
    out = ops.pool2d(ops.conv2d(inputs, kernel, strides=(1, 1)), pool_size=strides, strides=strides, pool_mode='avg')
    if bias is not None:
        out = out + bias
    return out


def upsample2d_v2(inputs, strides, padding='SAME'):
    """ops.py:622-640 (bilinear): every channel on its own through deconv2d with the single bilinear kernel [kh, kw, 1, 1]."""
    k = torch.as_tensor(ops.get_bilinear_kernel(strides).astype(np.float32), dtype=inputs.dtype)[:, :, None, None]
    n, h, w, c = inputs.shape
    x = inputs.permute(3, 0, 1, 2).reshape(c * n, h, w, 1)                 # tf.map_fn over the channels
    y = ops.deconv2d(x, k, strides=strides, padding=padding)
    return y.reshape(c, n, y.shape[1], y.shape[2]).permute(1, 2, 3, 0)


def upsample_conv2d_v2(inputs, kernel, bias=None, strides=(2, 2)):
    """ops.py:722-761."""
    ksize = tuple(kernel.shape[:2])
    up = upsample2d_v2(inputs, strides=strides, padding='VALID')
    out = ops.conv2d(up, kernel, strides=(1, 1), padding='FULL')
    same = ops.pad2d_paddings(inputs.shape[1:3], ksize, strides=(1, 1), padding='SAME')
    full = ops.pad2d_paddings(inputs.shape[1:3], ksize, strides=(1, 1), padding='FULL')
    top = (strides[0] - strides[0] % 2) // 2 + full[1][1] - same[1][1]
    left = (strides[1] - strides[1] % 2) // 2 + full[2][1] - same[2][1]
    out = out[:, top:top + strides[0] * inputs.shape[1], left:left + strides[1] * inputs.shape[2], :]
    if bias is not None:
        out = out + bias
    return out


def downsample(vs, h, hp, kernel_size):
    d = hp.downsample_layer
    if d == 'conv_pool2d':
        return _downsample_orig(vs, h, hp, kernel_size)
    if d == 'conv_pool2d_v2':
        return OS._maybe_tile_concat(conv_pool2d_v2, vs, 'conv_pool2d', h, strides=(2, 2))
    if d == 'conv2d':
        return OS._maybe_tile_concat(ops.conv2d, vs, 'conv2d', h, strides=(2, 2))
    raise ValueError('Invalid downsampling layer %s' % d)


def upsample(vs, h, hp):
    u = hp.upsample_layer
    if u == 'upsample_conv2d':
        return _upsample_orig(vs, h, hp)
    if u == 'upsample_conv2d_v2':
        return OS._maybe_tile_concat(upsample_conv2d_v2, vs, 'upsample_conv2d', h, strides=(2, 2))
    if u == 'deconv2d':
        return OS._maybe_tile_concat(deconv2d, vs, 'deconv2d', h, strides=(2, 2))
    raise ValueError('Invalid upsampling layer %s' % u)


def install(monkeypatch):
    LN.install(monkeypatch)
    monkeypatch.setattr(OS, '_norm_act', norm_act)
    monkeypatch.setattr(OS, '_downsample', downsample)
    monkeypatch.setattr(OS, '_upsample', upsample)

"""Layer normalisation for the fp64 oracle (oracle/savp.py refuses norm_layer / conv_rnn_norm_layer = 'layer' and stays as it is).

install(monkeypatch) replaces oracle.savp._norm_act, encoder and _conv_rnn; their callers (savp_cell_call, _conv_rnn_layer, posterior_fn,
prior_fn) look the names up at call time, so generator_fn and oracle.train.train_step then run the layer-normalised model.  With both
switches 'instance' (or 'none') every replacement hands over to the original function.

Reference semantics.  ops.get_norm_layer('layer') is tf.contrib.layers.layer_norm with its defaults (TF >= 1.9, ops.py:1062-1074):
begin_norm_axis = 1, begin_params_axis = -1, center = scale = True.  From memory of tensorflow/contrib/layers/python/layers/layers.py
(layer_norm, TF 1.9-1.15):

    norm_axes = list(range(begin_norm_axis, inputs_rank))                # (1, 2, 3) of NHWC: per sample over H, W and C
    params_shape = inputs_shape[begin_params_axis:]                      # [C]
    beta = ... initializer=init_ops.zeros_initializer()  ('beta')
    gamma = ... initializer=init_ops.ones_initializer()  ('gamma')
    mean, variance = nn.moments(inputs, norm_axes, keep_dims=True)       # biased variance
    variance_epsilon = 1e-12
    outputs = nn.batch_normalization(inputs, mean, variance, offset=beta, scale=gamma, variance_epsilon=variance_epsilon)

under the variable scope 'LayerNorm' (default_name of the layer_norm variable_scope).  The ConvLSTM cell with separate_norms=True
(rnn_ops.py:147-164, switched on by conv_rnn_norm_layer = 'layer' at savp_model.py:386-390) normalises i, j, f, o each on its own under the
scopes input / transform / forget / output, and new_c under 'state'; the cell's _norm creates <scope>/gamma and <scope>/beta (ones / zeros,
rnn_ops.py:102-112) and calls layer_norm(reuse=True, scope=scope), so those variables have no 'LayerNorm' level.
"""
import torch

import oracle.savp as OS
from oracle import ops, tf_ops

EPS_LN = 1e-12

_norm_act_orig = OS._norm_act
_encoder_orig = OS.encoder
_conv_rnn_orig = OS._conv_rnn


def layer_norm(x, gamma, beta, eps=EPS_LN):
    """tf.contrib.layers.layer_norm(x) with its defaults for x [N, ..., C]: statistics per sample over every other axis."""
    axes = tuple(range(1, x.dim()))
    mean = x.mean(dim=axes, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=axes, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * gamma + beta


def norm(vs, h, kind):
    """normalizer_fn(h) of the given kind, variables under vs/<InstanceNorm | LayerNorm>/."""
    if kind == 'layer':
        return layer_norm(h, vs['LayerNorm/gamma'], vs['LayerNorm/beta'])
    if kind == 'instance':
        return ops.fused_instance_norm(h, vs['InstanceNorm/gamma'], vs['InstanceNorm/beta'])
    raise NotImplementedError(kind)


def norm_act(vs, h, hp):
    """SAVPCell's norm_layer + activation_layer (savp_model.py:463-464, 499-500, 477, 512, 525, 537, 564, 627)."""
    if hp.norm_layer != 'layer':
        return _norm_act_orig(vs, h, hp)
    if hp.activation_layer != 'relu':
        raise NotImplementedError(hp.activation_layer)
    return torch.relu(norm(vs, h, 'layer'))


def encoder(vs, inputs, nef=64, n_layers=3, norm_layer='instance'):
    """networks.encoder (networks.py:12-32) with norm_layer = 'layer'."""
    if norm_layer != 'layer':
        return _encoder_orig(vs, inputs, nef=nef, n_layers=n_layers, norm_layer=norm_layer)
    paddings = [[0, 0], [1, 1], [1, 1], [0, 0]]
    s = vs.sub('layer_1')
    h = ops.conv2d(tf_ops.pad_constant(inputs, paddings), s['conv2d/kernel'], s['conv2d/bias'], strides=(2, 2), padding='VALID')
    h = ops.lrelu(h, 0.2)
    for i in range(1, n_layers):
        s = vs.sub('layer_%d' % (i + 1))
        h = ops.conv2d(tf_ops.pad_constant(h, paddings), s['conv2d/kernel'], s['conv2d/bias'], strides=(2, 2), padding='VALID')
        h = ops.lrelu(norm(s, h, 'layer'), 0.2)
    return h.mean(dim=(1, 2))


def conv_lstm_cell_separate(vs, inputs, state, filters, forget_bias=1.0):
    """BasicConv2DLSTMCell.call with normalizer_fn = layer_norm, separate_norms = True (rnn_ops.py:137-171)."""
    c, h = state
    vs = vs.sub('basic_conv2dlstm_cell')
    tile_concat = isinstance(inputs, (list, tuple))
    if tile_concat:
        inputs, inputs_non_spatial = inputs
    args = torch.cat([inputs, h], dim=-1)
    concat = tf_ops.conv2d(args, vs['kernel'], (1, 1), 'SAME')              # no bias: the cell has a normalizer (:122-125)
    if tile_concat:
        concat = concat + (inputs_non_spatial @ vs['weights'])[:, None, None, :]
    i, j, f, o = torch.chunk(concat, 4, dim=-1)                             # :150
    i = layer_norm(i, vs['input/gamma'], vs['input/beta'])                  # :151-155
    j = layer_norm(j, vs['transform/gamma'], vs['transform/beta'])
    f = layer_norm(f, vs['forget/gamma'], vs['forget/beta'])
    o = layer_norm(o, vs['output/gamma'], vs['output/beta'])
    new_c = c * torch.sigmoid(f + forget_bias) + torch.sigmoid(i) * torch.tanh(j)
    new_c = layer_norm(new_c, vs['state/gamma'], vs['state/beta'])          # :163-164
    new_h = torch.tanh(new_c) * torch.sigmoid(o)
    return new_h, (new_c, new_h)


def conv_rnn(vs, inputs, state, filters, hp):
    """SAVPCell._conv_rnn_func (savp_model.py:364-391) with conv_rnn_norm_layer = 'layer'."""
    if hp.conv_rnn_norm_layer != 'layer':
        return _conv_rnn_orig(vs, inputs, state, filters, hp)
    if hp.conv_rnn != 'lstm':
        raise NotImplementedError("conv_rnn_norm_layer='layer' with conv_rnn=%r" % hp.conv_rnn)
    if getattr(hp, 'ablation_conv_rnn_norm', False):                        # :380-384
        h, state = OS.conv_lstm_cell(vs, inputs, state, filters, False)
        return norm(vs, h, 'layer'), state
    return conv_lstm_cell_separate(vs, inputs, state, filters)


def install(monkeypatch):
    monkeypatch.setattr(OS, '_norm_act', norm_act)
    monkeypatch.setattr(OS, 'encoder', encoder)
    monkeypatch.setattr(OS, '_conv_rnn', conv_rnn)

"""The fp64 oracle for conv_rnn = 'gru' with conv_rnn_norm_layer = 'layer' inside the cell (no ablation): Conv2DGRUCell.call with
normalizer_fn = layer_norm and separate_norms = True (rnn_ops.py:234-267, switched on at savp_model.py:386-390).  tests/oracle_layer_norm.py
refuses 'layer' with a GRU and tests/oracle_gru_plain.py adds the ablation_conv_rnn_norm branch only; install() puts this one branch in
front of the latter and hands everything else over.

The cell's _norm (rnn_ops.py:203-212) creates <scope>/gamma and <scope>/beta itself and calls layer_norm(reuse=True, scope=scope), so the
variables are gates/reset/{gamma,beta}, gates/update/{gamma,beta} and candidate/state/{gamma,beta}, each [F], without a LayerNorm level."""
import torch

import oracle.savp as OS
from oracle import tf_ops
from tests import oracle_gru_plain as OGP
from tests.oracle_layer_norm import layer_norm


def conv_gru_cell_separate(vs, inputs, state, filters):
    """Conv2DGRUCell.call with normalizer_fn = layer_norm, separate_norms = True.  Keeps the quirk of oracle.savp.conv_gru_cell: the
    candidate convolution sees [x, h, r*h] (rnn_ops.py:242 rebinds `inputs`, :258 concatenates again)."""
    vs = vs.sub('conv2dgru_cell')
    tile_concat = isinstance(inputs, (list, tuple))
    if tile_concat:
        inputs, inputs_non_spatial = inputs
    g = vs.sub('gates')
    inputs = torch.cat([inputs, state], dim=-1)
    concat = tf_ops.conv2d(inputs, g['kernel'], (1, 1), 'SAME')                  # no bias: the cell has a normalizer (:220-223)
    if tile_concat:
        concat = concat + (inputs_non_spatial @ g['weights'])[:, None, None, :]
    r, u = torch.chunk(concat, 2, dim=-1)                                       # :246
    r = layer_norm(r, g['reset/gamma'], g['reset/beta'])                        # :247-249
    u = layer_norm(u, g['update/gamma'], g['update/beta'])
    r, u = torch.sigmoid(r), torch.sigmoid(u)
    cs = vs.sub('candidate')
    inputs = torch.cat([inputs, r * state], dim=-1)
    candidate = tf_ops.conv2d(inputs, cs['kernel'], (1, 1), 'SAME')
    if tile_concat:
        candidate = candidate + (inputs_non_spatial @ cs['weights'])[:, None, None, :]
    candidate = layer_norm(candidate, cs['state/gamma'], cs['state/beta'])      # :261-262
    c = torch.tanh(candidate)
    new_h = u * state + (1 - u) * c
    return new_h, new_h


def conv_rnn(vs, inputs, state, filters, hp):
    if (hp.conv_rnn == 'gru' and hp.conv_rnn_norm_layer == 'layer' and not getattr(hp, 'ablation_conv_rnn_norm', False)
            and not getattr(hp, 'ablation_rnn', False)):
        return conv_gru_cell_separate(vs, inputs, state, filters)
    return OGP.conv_rnn(vs, inputs, state, filters, hp)


def install(monkeypatch):
    OGP.install(monkeypatch)
    monkeypatch.setattr(OS, '_conv_rnn', conv_rnn)

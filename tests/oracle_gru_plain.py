"""The fp64 oracle for conv_rnn = 'gru' with ablation_conv_rnn_norm and conv_rnn_norm_layer = 'layer' (savp_model.py:380-384: the cell is
built without a normaliser, normalizer_fn(h) -- here a layer norm -- goes over the layer's output only).  tests/oracle_layer_norm.py refuses
'layer' with a GRU in its conv_rnn; install() puts this one branch in front of it and hands everything else over."""
import oracle.savp as OS
from tests import oracle_layer_norm as OLN


def conv_rnn(vs, inputs, state, filters, hp):
    if hp.conv_rnn == 'gru' and hp.conv_rnn_norm_layer == 'layer' and getattr(hp, 'ablation_conv_rnn_norm', False):
        h, state = OS.conv_gru_cell(vs, inputs, state, filters, False)
        return OLN.norm(vs, h, 'layer'), state
    return OLN.conv_rnn(vs, inputs, state, filters, hp)


def install(monkeypatch):
    OLN.install(monkeypatch)
    monkeypatch.setattr(OS, '_conv_rnn', conv_rnn)

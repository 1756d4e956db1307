"""CPU pins of the layer-norm oracle extension (tests/oracle_layer_norm.py), of the variable table for norm_layer / conv_rnn_norm_layer =
'layer', and of the combinations the HIP path refuses."""
import numpy as np
import pytest
import torch

import oracle.savp as OS
from oracle import ops
from tests import oracle_layer_norm as OLN
from video_prediction_amd import variables as V
from tests.gpu_model_checks import make_hparams
from video_prediction_amd.models.savp_cell import check_norm_layers


def _x(seed=0, shape=(3, 5, 6, 8)):
    g = torch.Generator().manual_seed(seed)
    # channel means that differ, so that the layer norm and the instance norm disagree
    return (torch.randn(*shape, generator=g) + torch.arange(shape[-1]) * 0.7).double()


def _gb(C, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.2 * torch.randn(C, generator=g)).double(), (0.1 * torch.randn(C, generator=g)).double()


def tf_layer_norm_literal(x, gamma, beta):
    """nn.moments over axes (1, 2, 3) with keep_dims, then nn.batch_normalization with variance_epsilon 1e-12, written out per sample."""
    out = torch.empty_like(x)
    for n in range(x.shape[0]):
        v = x[n]
        mean = v.sum() / v.numel()
        var = ((v - mean) ** 2).sum() / v.numel()
        inv = 1.0 / torch.sqrt(var + 1e-12)
        out[n] = v * (inv * gamma) + (beta - mean * inv * gamma)
    return out


def test_layer_norm_matches_the_tf_formula():
    x = _x()
    g, b = _gb(x.shape[-1])
    assert torch.allclose(OLN.layer_norm(x, g, b), tf_layer_norm_literal(x, g, b), rtol=1e-12, atol=1e-12)


def test_layer_norm_has_zero_mean_unit_variance_per_sample():
    x = _x(2)
    C = x.shape[-1]
    y = OLN.layer_norm(x, torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64))
    for n in range(x.shape[0]):
        assert abs(float(y[n].mean())) < 1e-12
        assert abs(float(y[n].var(unbiased=False)) - 1.0) < 1e-9
    # ... but not per channel (the channel means differ)
    assert float(y.mean(dim=(1, 2)).abs().max()) > 0.1


def test_layer_norm_differs_from_instance_norm():
    x = _x(3)
    g, b = _gb(x.shape[-1])
    assert float((OLN.layer_norm(x, g, b) - ops.fused_instance_norm(x, g, b)).abs().max()) > 0.1


def test_layer_norm_of_a_constant_plane_is_beta():
    x = torch.full((2, 4, 4, 8), 3.25, dtype=torch.float64)
    g, b = _gb(8)
    y = OLN.layer_norm(x, g, b)
    assert torch.isfinite(y).all()
    assert torch.equal(y, b.expand_as(y))


def _lstm_vars(F, cin, seed=5):
    g = torch.Generator().manual_seed(seed)
    p = {'basic_conv2dlstm_cell/kernel': 0.1 * torch.randn(5, 5, cin + F, 4 * F, generator=g).double()}
    for k, name in enumerate(('input', 'transform', 'forget', 'output', 'state')):
        gm, bt = _gb(F, seed=seed + 10 + k)
        p['basic_conv2dlstm_cell/%s/gamma' % name] = gm
        p['basic_conv2dlstm_cell/%s/beta' % name] = bt
    return p


def _lstm_inputs(F, cin, seed=6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 6, 6, cin, generator=g).double()
    c = torch.randn(2, 6, 6, F, generator=g).double()
    h = torch.randn(2, 6, 6, F, generator=g).double()
    return x, (c, h)


def _lstm_by_hand(p, x, state, eps=1e-12, split=True):
    """The cell restated with the gates split by hand and each normalised by an explicit per-sample (H, W, F) loop."""
    c, h = state
    from oracle import tf_ops
    z = tf_ops.conv2d(torch.cat([x, h], -1), p['basic_conv2dlstm_cell/kernel'], (1, 1), 'SAME')
    F = c.shape[-1]

    def ln(v, name):
        gm, bt = p['basic_conv2dlstm_cell/%s/gamma' % name], p['basic_conv2dlstm_cell/%s/beta' % name]
        out = torch.empty_like(v)
        for n in range(v.shape[0]):
            m = v[n].mean()
            out[n] = (v[n] - m) / torch.sqrt(((v[n] - m) ** 2).mean() + eps) * gm + bt
        return out

    if split:
        i, j, f, o = (ln(z[..., k * F:(k + 1) * F], nm) for k, nm in enumerate(('input', 'transform', 'forget', 'output')))
    else:                     # mutation: one norm over the concatenated gates
        gm = torch.cat([p['basic_conv2dlstm_cell/%s/gamma' % nm] for nm in ('input', 'transform', 'forget', 'output')])
        bt = torch.cat([p['basic_conv2dlstm_cell/%s/beta' % nm] for nm in ('input', 'transform', 'forget', 'output')])
        zz = OLN.layer_norm(z, gm, bt, eps)
        i, j, f, o = torch.chunk(zz, 4, dim=-1)
    nc = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    nc = ln(nc, 'state')
    return torch.tanh(nc) * torch.sigmoid(o), nc


def test_lstm_separate_norms_match_a_hand_split_restatement():
    F, cin = 4, 3
    p = _lstm_vars(F, cin)
    x, st = _lstm_inputs(F, cin)
    h, (nc, _) = OLN.conv_lstm_cell_separate(OS.Scope(p), x, st, F)
    hh, ncc = _lstm_by_hand(p, x, st)
    assert torch.allclose(h, hh, rtol=1e-10, atol=1e-12) and torch.allclose(nc, ncc, rtol=1e-10, atol=1e-12)


def test_named_mutations_fail_the_pins():
    x = _x(4)
    g, b = _gb(x.shape[-1])
    ref = tf_layer_norm_literal(x, g, b)
    # a wrong epsilon (the instance norm's) on a low-variance input
    xs = x * 1e-3
    assert float((OLN.layer_norm(xs, g, b, eps=1e-6) - tf_layer_norm_literal(xs, g, b)).abs().max()) > 1e-3
    # normalising over (H, W) only is the instance norm
    hw = (x - x.mean(dim=(1, 2), keepdim=True)) / torch.sqrt(x.var(dim=(1, 2), unbiased=False, keepdim=True) + 1e-12) * g + b
    assert float((hw - ref).abs().max()) > 0.1
    # one norm over the concatenated gates
    F, cin = 4, 3
    p = _lstm_vars(F, cin)
    x2, st = _lstm_inputs(F, cin)
    p['basic_conv2dlstm_cell/kernel'][..., 0:F] *= 5.0          # gate blocks of different scale, so that the mutation shows
    h, _ = OLN.conv_lstm_cell_separate(OS.Scope(p), x2, st, F)
    hm, _ = _lstm_by_hand(p, x2, st, split=False)
    assert float((h - hm).abs().max()) > 1e-3


def _hp(**over):
    d = dict(context_frames=2, sequence_length=5, nz=8)
    d.update(over)
    return make_hparams(**d)


def test_instance_switches_leave_the_oracle_unpatched(monkeypatch):
    hp = _hp()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 4, 8, generator=g).double()
    vs = OS.Scope({'InstanceNorm/gamma': torch.ones(8).double(), 'InstanceNorm/beta': torch.zeros(8).double()})
    want = OS._norm_act(vs, x, hp)
    OLN.install(monkeypatch)
    assert OS._norm_act is OLN.norm_act
    assert torch.equal(OS._norm_act(vs, x, hp), want)


def _cfgs():
    return [('layer', 'instance', {}), ('instance', 'layer', dict(ablation_conv_rnn_norm=True)),
            ('layer', 'layer', dict(ablation_conv_rnn_norm=True)), ('layer', 'layer', dict(ablation_rnn=True)),
            ('layer', 'instance', dict(learn_prior=True, use_e_rnn=True)), ('layer', 'instance', dict(transformation='flow')),
            ('layer', 'layer', {})]


@pytest.mark.parametrize('nl,cl,over', _cfgs())
def test_variable_table_holds_the_layer_norm_variables(nl, cl, over):
    hp = _hp(norm_layer=nl, conv_rnn_norm_layer=cl, **over)
    specs = V.variable_specs(hp, (64, 64, 3), mode='train')
    names = set(specs)
    ln = [k for k in names if '/LayerNorm/' in k]
    if nl == 'layer':
        for k in ('generator/rnn/savp_cell/h0/LayerNorm/gamma', 'generator/rnn/savp_cell/h0/LayerNorm/beta',
                  'generator/rnn/savp_cell/h6_masks/LayerNorm/gamma', 'generator/encoder/layer_2/LayerNorm/gamma'):
            assert k in names, k
        assert not any('InstanceNorm' in k for k in names if '/h0/' in k or 'encoder/layer_' in k)
        assert specs['generator/rnn/savp_cell/h0/LayerNorm/gamma'] == ((hp.ngf,), 'ones')
        assert specs['generator/rnn/savp_cell/h0/LayerNorm/beta'] == ((hp.ngf,), 'zeros')
    if cl == 'layer' and over.get('ablation_conv_rnn_norm'):
        assert 'generator/rnn/savp_cell/lstm_h0/LayerNorm/gamma' in names
    if cl == 'layer' and not over:
        s = 'generator/rnn/savp_cell/lstm_h0/basic_conv2dlstm_cell/'
        for name in ('input', 'transform', 'forget', 'output', 'state'):
            assert specs[s + name + '/gamma'] == ((hp.ngf,), 'ones') and specs[s + name + '/beta'] == ((hp.ngf,), 'zeros')
        assert s + 'input_transform_forget_output/gamma' not in names and s + 'bias' not in names
    assert ln or nl != 'layer'


@pytest.mark.parametrize('nl,cl,over', _cfgs())
def test_oracle_extension_reads_exactly_the_variable_table(monkeypatch, nl, cl, over):
    """generator_fn of the patched oracle on the table's variables: every LayerNorm variable is read, and nothing is missing."""
    OLN.install(monkeypatch)
    hp = _hp(norm_layer=nl, conv_rnn_norm_layer=cl, ngf=8, nef=8, **over)
    specs = V.variable_specs(hp, (32, 32, 3), mode='test')
    vals = V.init_variables(specs, seed=4)
    read = set()

    class Rec(dict):
        def __getitem__(self, k):
            read.add(k)
            return dict.__getitem__(self, k)

        def __contains__(self, k):
            return dict.__contains__(self, k)

    P = Rec({k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()})
    from tests.gpu_model_checks import synth, make_noise
    B = 2
    images = synth(hp, B, 32, 32, 3, 0)
    noise = make_noise(hp, B, sampling=True)
    OS.generator_fn(OS.Scope(P).sub('generator'), {'images': images}, 'test', hp, noise)
    ln = {k for k in specs if 'LayerNorm' in k}
    assert ln and ln <= read


@pytest.mark.parametrize('over,msg', [
    (dict(conv_rnn='gru', conv_rnn_norm_layer='layer'), "conv_rnn='gru'"),
    (dict(norm_layer='layer', use_tile_concat=False), 'use_tile_concat=False'),
    (dict(conv_rnn_norm_layer='layer', ablation_conv_rnn_norm=True, use_tile_concat=False), 'use_tile_concat=False'),
    (dict(norm_layer='batch'), "norm_layer='batch'"),
    (dict(conv_rnn_norm_layer='batch'), "conv_rnn_norm_layer='batch'"),
    (dict(norm_layer='none'), "norm_layer='none'"),
])
def test_refusals_name_the_combination(over, msg):
    with pytest.raises(NotImplementedError, match=msg.replace('(', r'\(')):
        check_norm_layers(_hp(**over))


@pytest.mark.parametrize('over', [dict(norm_layer='layer'), dict(conv_rnn_norm_layer='layer', ablation_conv_rnn_norm=True),
                                  dict(norm_layer='layer', conv_rnn_norm_layer='layer', ablation_conv_rnn_norm=True),
                                  dict(conv_rnn_norm_layer='layer'), dict(norm_layer='layer', conv_rnn_norm_layer='layer'), {}])
def test_supported_combinations_pass_the_check(over):
    check_norm_layers(_hp(**over))

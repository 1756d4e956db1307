"""norm_layer = 'none' (ops.get_norm_layer('none') = tf.identity) on the host side: the variable table against the oracle's variable set,
and what check_norm_layers accepts and refuses.  The value is opt-in (SAVP_NORM_NONE=1 or the keyword norm_none=True, like the layer-norm
GRU cell's ln_gru): without it the refusal that tests/test_oracle_layer_norm.py pins stays.  No device, no library."""
import numpy as np
import pytest
import torch

from oracle import savp as OS
from video_prediction_amd import variables as V
from video_prediction_amd.hparams import HParams
from video_prediction_amd.models import conv_rnn_cells as CC
from video_prediction_amd.models.hparam_defaults import savp_defaults
from video_prediction_amd.models.savp_cell import check_norm_layers


def _hp(**over):
    hp = HParams(**savp_defaults())
    hp.override_from_dict(over)
    return hp


CASES = {
    'default_cell': dict(),
    'gru': dict(conv_rnn='gru'),
    'ablation_rnn': dict(ablation_rnn=True),
    'untiled_latent': dict(use_tile_concat=False),
    'untiled_latent_ablation_rnn': dict(use_tile_concat=False, ablation_rnn=True),
    'learn_prior_e_rnn': dict(learn_prior=True, use_e_rnn=True, nef=8),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_variable_table_equals_the_oracles_variable_set(name):
    """As tests/test_variable_table_matches_oracle.py: the oracle's generator_fn runs on exactly the table's variables and reads every one
    of them -- no InstanceNorm / LayerNorm variable at a norm_layer site, the convolutions' biases and the untiled latent's dense
    kernels stay."""
    hp = _hp(context_frames=2, sequence_length=4, ngf=8, nz=4, norm_layer='none', **CASES[name])
    H = W = 64
    specs = V.variable_specs(hp, (H, W, 3), mode='test')
    p = 'generator/rnn/savp_cell/'
    sites = [p + 'h%d/' % i for i in range(6)] + [p + 'h6_masks/', p + 'h6_scratch/'] + ['generator/encoder/layer_%d/' % i for i in (1, 2, 3)]
    assert not [k for k in specs if any(k.startswith(s + n) for s in sites for n in ('InstanceNorm/', 'LayerNorm/'))]
    assert p + 'h0/conv_pool2d/bias' in specs and p + 'h6_masks/conv2d/bias' in specs and 'generator/encoder/layer_2/conv2d/bias' in specs
    assert ((p + 'h0/dense/kernel') in specs) == (not hp.use_tile_concat)
    vals = V.init_variables(specs, seed=3)
    rng = np.random.default_rng(11)
    P = {}
    for k, v in vals.items():
        v = np.asarray(v, dtype=np.float64)
        if float(np.abs(v).max()) == 0.0:                          # zero-initialised biases: make them matter
            v = 0.1 * rng.standard_normal(v.shape)
        P[k] = torch.tensor(v, requires_grad=True)
    B, T = 1, hp.sequence_length
    images = torch.tensor(rng.random((T, B, H, W, 3)))
    noise = {'eps': torch.tensor(rng.standard_normal((T - 1, B, hp.nz))),
             'prior': torch.tensor(rng.standard_normal((T - hp.context_frames, B, hp.nz)))}
    if hp.learn_prior:
        noise['prior_eps'] = torch.tensor(rng.standard_normal((T - 1, B, hp.nz)))
    out = OS.generator_fn(OS.Scope(P).sub('generator'), {'images': images}, 'train', hp, noise)
    total = 0.0
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point() and v.requires_grad:
            total = total + (v * torch.tensor(rng.standard_normal(tuple(v.shape)))).sum()
    names = [k for k in P if k.startswith('generator/')]
    grads = torch.autograd.grad(total, [P[k] for k in names], allow_unused=True)
    unread = [k for k, g in zip(names, grads) if g is None]
    assert not unread, (name, unread)
    assert all(torch.isfinite(g).all() for g in grads)


ACCEPTED = [dict(), dict(conv_rnn_norm_layer='none'), dict(conv_rnn_norm_layer='layer'), dict(conv_rnn='gru'),
            dict(conv_rnn='gru', conv_rnn_norm_layer='none'), dict(ablation_rnn=True), dict(ablation_conv_rnn_norm=True),
            dict(use_tile_concat=False), dict(use_tile_concat=False, where_add='middle'), dict(use_tile_concat=False, ablation_rnn=True),
            # a bare cell takes no untiled latent unless where_add = 'all' hands it one
            dict(use_tile_concat=False, where_add='input', conv_rnn_norm_layer='none'),
            dict(use_tile_concat=False, conv_rnn_norm_layer='none', nz=0)]


@pytest.mark.parametrize('over', ACCEPTED, ids=[','.join('%s=%s' % kv for kv in o.items()) or 'alone' for o in ACCEPTED])
def test_check_norm_layers_accepts_none(over):
    hp = _hp(norm_layer='none', **over)
    check_norm_layers(hp, norm_none=True)
    CC.cell_class(hp, zw=hp.nz, norm_none=True)


def test_the_opt_in_is_the_keyword_or_the_environment(monkeypatch):
    from video_prediction_amd.models.savp_cell import norm_none_opt_in
    hp = _hp(norm_layer='none')
    monkeypatch.delenv('SAVP_NORM_NONE', raising=False)
    assert not norm_none_opt_in() and norm_none_opt_in(True)
    for fn in (check_norm_layers, CC.cell_class):          # without it: refused, the value named
        for kw in ({}, dict(norm_none=False)):
            with pytest.raises(NotImplementedError, match="norm_layer='none'.*SAVP_NORM_NONE=1"):
                fn(hp, **kw)
    monkeypatch.setenv('SAVP_NORM_NONE', '1')
    assert norm_none_opt_in() and not norm_none_opt_in(False)
    check_norm_layers(hp)
    assert CC.cell_class(hp)[0] is CC.InstanceNormLSTM
    with pytest.raises(NotImplementedError, match="norm_layer='none'"):          # the keyword wins over the environment
        check_norm_layers(hp, norm_none=False)
    # nothing differs for any other model
    check_norm_layers(_hp())
    check_norm_layers(_hp(norm_layer='layer'), norm_none=True)


def test_batch_stays_refused_with_its_message():
    with pytest.raises(NotImplementedError) as e:
        check_norm_layers(_hp(norm_layer='batch'))
    assert str(e.value) == "norm_layer='batch': the HIP path covers 'instance' and 'layer'"
    with pytest.raises(NotImplementedError, match="conv_rnn_norm_layer='batch'"):
        check_norm_layers(_hp(norm_layer='none', conv_rnn_norm_layer='batch'), norm_none=True)


REFUSED = [
    # unchanged: a layer norm does not cancel the untiled latent
    (dict(norm_layer='none', conv_rnn_norm_layer='layer', use_tile_concat=False), 'the untiled latent is only cancelled by an instance norm'),
    (dict(norm_layer='layer', use_tile_concat=False), 'the untiled latent is only cancelled by an instance norm'),
    # unchanged: the bare GRU cell, whatever norm_layer is
    (dict(conv_rnn='gru', conv_rnn_norm_layer='none', use_tile_concat=False), "conv_rnn='gru' without a cell normaliser"),
    (dict(norm_layer='none', conv_rnn='gru', conv_rnn_norm_layer='none', use_tile_concat=False), "conv_rnn='gru' without a cell normaliser"),
    (dict(norm_layer='none', conv_rnn='gru', ablation_conv_rnn_norm=True, use_tile_concat=False), "conv_rnn='gru' without a cell normaliser"),
    # new: the bare ConvLSTM cell's gap must not be widened by a model without any normaliser
    (dict(norm_layer='none', conv_rnn_norm_layer='none', use_tile_concat=False), "norm_layer='none' with conv_rnn='lstm' without a cell normaliser"),
    (dict(norm_layer='none', ablation_conv_rnn_norm=True, use_tile_concat=False), "norm_layer='none' with conv_rnn='lstm' without a cell normaliser"),
]


@pytest.mark.parametrize('over,text', REFUSED, ids=[','.join('%s=%s' % kv for kv in o.items()) for o, _ in REFUSED])
def test_the_untiled_latent_refusals(over, text):
    for fn in (lambda hp: check_norm_layers(hp, norm_none=True), lambda hp: CC.cell_class(hp, zw=hp.nz, norm_none=True)):
        with pytest.raises(NotImplementedError, match=text):
            fn(_hp(**over))


def test_the_bare_lstm_gap_itself_stays_as_it_is():
    """norm_layer = 'instance' with the bare ConvLSTM cell and an untiled latent is the known gap of DESIGN.md section 7: still built."""
    hp = _hp(conv_rnn_norm_layer='none', use_tile_concat=False)
    check_norm_layers(hp)
    assert CC.cell_class(hp, zw=8)[0] is CC.BareLSTM
    # and without a latent or conditioning columns nothing is added anywhere
    assert CC.cell_class(_hp(norm_layer='none', conv_rnn_norm_layer='none', use_tile_concat=False), zw=0, norm_none=True)[0] is CC.BareLSTM

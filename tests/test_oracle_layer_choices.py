"""CPU pins of the layer-choice oracle extension (tests/oracle_layer_choices.py): downsample_layer in (conv2d, conv_pool2d_v2), upsample_layer
in (deconv2d, upsample_conv2d_v2), activation_layer = elu; of the variable table for them; and of the kernel embedding that the HIP path's
'down' / 'deconv' convolution kinds use (engine.ConvLayer).  Everything in fp64; identities hold to an absolute error of 1e-12, the bound
tests/test_oracle_tf_semantics.py puts on identities of the same kind."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle.savp as OS
from oracle import ops
from tests import oracle_layer_choices as OLC
from tests import oracle_layer_norm as OLN
from video_prediction_amd import variables as V
from video_prediction_amd.hparams import HParams
from video_prediction_amd.models.hparam_defaults import savp_defaults

TOL = 1e-12


def _rand(shape, seed):
    return torch.tensor(np.random.default_rng(seed).standard_normal(shape))


# ---- literal restatements ------------------------------------------------------------------------------------------------------------
def same_conv_literal(x, w, stride):
    """tf.nn.conv2d, 'SAME': out = ceil(in / s), total pad = max((out - 1) * s + k - in, 0), the smaller half first; then a 'VALID'
    cross-correlation written as loops over output pixels."""
    n, h, wd, ci = x.shape
    kh, kw, _, co = w.shape
    oh, ow = -(-h // stride), -(-wd // stride)
    ph, pw = max((oh - 1) * stride + kh - h, 0), max((ow - 1) * stride + kw - wd, 0)
    xp = torch.zeros(n, h + ph, wd + pw, ci, dtype=x.dtype)
    xp[:, ph // 2:ph // 2 + h, pw // 2:pw // 2 + wd] = x
    out = torch.zeros(n, oh, ow, co, dtype=x.dtype)
    for oy in range(oh):
        for ox in range(ow):
            patch = xp[:, oy * stride:oy * stride + kh, ox * stride:ox * stride + kw, :]
            out[:, oy, ox, :] = torch.einsum('nuvc,uvcf->nf', patch, w)
    return out


@pytest.mark.parametrize('k,hw', [(3, (8, 8)), (5, (8, 8)), (3, (6, 10)), (5, (4, 12))])
def test_strided_same_conv_matches_pad_then_valid_loop(k, hw):
    x, w, b = _rand((2,) + hw + (3,), 1), _rand((k, k, 3, 4), 2), _rand((4,), 3)
    got = ops.conv2d(x, w, b, strides=(2, 2))
    assert got.shape == (2, hw[0] // 2, hw[1] // 2, 4)
    assert float((got - (same_conv_literal(x, w, 2) + b)).abs().max()) <= TOL


def test_same_padding_of_the_strided_conv_on_an_even_plane():
    """k - 2 in total, the smaller half first: 0 / 1 for 3x3, 1 / 2 for 5x5 (what the kernel embedding rests on)."""
    from oracle.tf_ops import same_pad
    for size in (4, 8, 64):
        assert same_pad(size, 3, 2) == (0, 1)
        assert same_pad(size, 5, 2) == (1, 2)
        assert same_pad(size, 4, 2) == (1, 1)
        assert same_pad(size, 6, 2) == (2, 2)


@pytest.mark.parametrize('hw', [(4, 4), (3, 5)])
def test_deconv2d_is_the_autograd_gradient_of_the_strided_same_conv(hw):
    """tf.nn.conv2d_transpose(y, kernel [k, k, F, Cin], output 2H x 2W, 'SAME') is d/dx of sum(conv2d(x, kernel, 2, 'SAME') * y)."""
    f_out, cin = 5, 3
    y, w, b = _rand((2,) + hw + (cin,), 4), _rand((3, 3, f_out, cin), 5), _rand((f_out,), 6)
    got = OLC.deconv2d(y, w, b, strides=(2, 2))
    assert got.shape == (2, 2 * hw[0], 2 * hw[1], f_out)
    x = torch.zeros(2, 2 * hw[0], 2 * hw[1], f_out, dtype=torch.float64, requires_grad=True)
    (same_conv_literal(x, w, 2) * y).sum().backward()
    assert float((got - (x.grad + b)).abs().max()) <= TOL


def test_elu_matches_torch_elu_and_its_derivative():
    z = torch.cat([_rand((960,), 7) * 3, torch.tensor([0.0, -0.0, 1e-9, -1e-9, -40.0, 40.0], dtype=torch.float64)])
    assert float((OLC.elu(z) - F.elu(z)).abs().max()) <= TOL
    zz = z.clone().requires_grad_(True)
    OLC.elu(zz).sum().backward()
    assert float((zz.grad - torch.where(z > 0, torch.ones_like(z), torch.exp(z))).abs().max()) <= TOL


# ---- the _v2 names are aliases ---------------------------------------------------------------------------------------------------------
def conv_then_avg_pool_literal(x, w):
    """conv_pool2d_v2 from ops.py:859-892: 'SAME' stride-1 convolution, then 2x2 average pooling with stride 2."""
    c = same_conv_literal(x, w, 1)
    return 0.25 * (c[:, 0::2, 0::2] + c[:, 1::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 1::2])


@pytest.mark.parametrize('k', [3, 5])
def test_conv_pool2d_v2_equals_conv_pool2d(k):
    x, w, b = _rand((2, 8, 6, 3), 8), _rand((k, k, 3, 4), 9), _rand((4,), 10)
    v1 = ops.conv_pool2d(x, w, b, strides=(2, 2))
    v2 = OLC.conv_pool2d_v2(x, w, b, strides=(2, 2))
    assert float((v2 - (conv_then_avg_pool_literal(x, w) + b)).abs().max()) <= TOL
    assert float((v1 - v2).abs().max()) <= TOL


def bilinear_valid_upsample_literal(x):
    """upsample2d_v2 with 'VALID' (ops.py:622-640): conv2d_transpose of every channel with the 4x4 bilinear kernel, stride 2 -> a scatter of
    each input pixel times the kernel into a (2H + 2) x (2W + 2) plane."""
    k1 = torch.tensor([0.25, 0.75, 0.75, 0.25], dtype=x.dtype)
    k = k1[:, None] * k1[None, :]
    n, h, w, c = x.shape
    out = torch.zeros(n, 2 * h + 2, 2 * w + 2, c, dtype=x.dtype)
    for i in range(h):
        for j in range(w):
            out[:, 2 * i:2 * i + 4, 2 * j:2 * j + 4, :] += x[:, i:i + 1, j:j + 1, :] * k[None, :, :, None]
    return out


def test_upsample_conv2d_v2_equals_upsample_conv2d():
    x, w, b = _rand((2, 4, 5, 3), 11), _rand((3, 3, 3, 4), 12), _rand((4,), 13)
    assert float((ops.get_bilinear_kernel((2, 2)) - np.outer([0.25, 0.75, 0.75, 0.25], [0.25, 0.75, 0.75, 0.25])).__abs__().max()) == 0.0
    up = bilinear_valid_upsample_literal(x)
    assert float((OLC.upsample2d_v2(x, (2, 2), padding='VALID') - up).abs().max()) <= TOL
    # 'FULL' stride-1 convolution = k - 1 zeros on every side, then 'VALID'; crop (ops.py:746-751): top = left = 1 + 2 - 1 = 2
    full = torch.zeros(2, up.shape[1] + 4, up.shape[2] + 4, 3, dtype=torch.float64)
    full[:, 2:-2, 2:-2] = up
    lit = torch.zeros(2, up.shape[1] + 2, up.shape[2] + 2, 4, dtype=torch.float64)
    for oy in range(lit.shape[1]):
        for ox in range(lit.shape[2]):
            lit[:, oy, ox] = torch.einsum('nuvc,uvcf->nf', full[:, oy:oy + 3, ox:ox + 3], w)
    lit = lit[:, 2:2 + 8, 2:2 + 10] + b
    v2 = OLC.upsample_conv2d_v2(x, w, b, strides=(2, 2))
    v1 = ops.upsample_conv2d(x, w, b, strides=(2, 2))
    assert v2.shape == v1.shape == (2, 8, 10, 4)
    assert float((v2 - lit).abs().max()) <= TOL
    assert float((v1 - v2).abs().max()) <= TOL


# ---- the installed oracle ---------------------------------------------------------------------------------------------------------------
def _hp(**over):
    hp = HParams(**savp_defaults())
    hp.override_from_dict(dict(dict(context_frames=2, sequence_length=4, ngf=8, nz=4), **over))
    return hp


def _run(hp, seed=3, H=64, W=64, B=1, return_vars=False):
    specs = V.variable_specs(hp, (H, W, 3), mode='test')
    vals = V.init_variables(specs, seed=seed)
    rng = np.random.default_rng(11)
    P = {}
    for k, v in vals.items():
        v = np.asarray(v, dtype=np.float64)
        if float(np.abs(v).max()) == 0.0:
            v = 0.1 * rng.standard_normal(v.shape)
        P[k] = torch.tensor(v, requires_grad=True)
    T = hp.sequence_length
    images = torch.tensor(rng.random((T, B, H, W, 3)))
    noise = {'eps': torch.tensor(rng.standard_normal((T - 1, B, hp.nz))),
             'prior': torch.tensor(rng.standard_normal((T - hp.context_frames, B, hp.nz)))}
    out = OS.generator_fn(OS.Scope(P).sub('generator'), {'images': images}, 'train', hp, noise)
    return (out, P, rng) if return_vars else out


def test_the_bare_oracle_refuses_the_new_values():
    for over in (dict(downsample_layer='conv2d'), dict(upsample_layer='deconv2d'), dict(activation_layer='elu')):
        with pytest.raises((NotImplementedError, KeyError)):
            _run(_hp(**over))


@pytest.mark.parametrize('over', [dict(), dict(norm_layer='layer'), dict(conv_rnn='gru'), dict(ablation_rnn=True)], ids=str)
def test_installed_oracle_is_bit_identical_on_the_defaults(over, monkeypatch):
    if over.get('norm_layer') == 'layer':          # the bare oracle has no layer norm: the reference is the layer-norm extension alone
        with monkeypatch.context() as m:
            OLN.install(m)
            ref = _run(_hp(**over))
    else:
        ref = _run(_hp(**over))
    OLC.install(monkeypatch)
    after = _run(_hp(**over))
    n = 0
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert torch.equal(v, after[k]), k
            n += 1
    assert n >= 2


def test_v2_names_give_the_default_model(monkeypatch):
    OLC.install(monkeypatch)
    a = _run(_hp())
    b = _run(_hp(downsample_layer='conv_pool2d_v2', upsample_layer='upsample_conv2d_v2'))
    assert float((a['gen_images'] - b['gen_images']).detach().abs().max()) <= 1e-11          # a whole unroll of 1e-12 identities
    assert float((a['gen_images'] - _run(_hp(downsample_layer='conv2d'))['gen_images']).detach().abs().max()) > 1e-4


def test_unknown_values_raise_value_error(monkeypatch):
    OLC.install(monkeypatch)
    for over, word in ((dict(downsample_layer='max_pool'), 'downsampling'), (dict(upsample_layer='nearest'), 'upsampling'),
                       (dict(activation_layer='gelu'), 'activation')):
        with pytest.raises(ValueError, match='Invalid %s layer' % word):
            V.variable_specs(_hp(**over), (64, 64, 3), mode='test') and _run(_hp(**over))


CASES = {
    'conv2d': dict(downsample_layer='conv2d'),
    'deconv2d': dict(upsample_layer='deconv2d'),
    'elu': dict(activation_layer='elu'),
    'all_three': dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu'),
    'all_three_layer_norm': dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu', norm_layer='layer',
                                 conv_rnn_norm_layer='layer'),
    'all_three_gru': dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu', conv_rnn='gru'),
    'all_three_ablation_rnn': dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu', ablation_rnn=True),
    'all_three_untiled': dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu', use_tile_concat=False),
    'all_three_where_add_input': dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu', where_add='input'),
    'all_three_where_add_middle': dict(downsample_layer='conv2d', upsample_layer='deconv2d', activation_layer='elu', where_add='middle'),
    'v2': dict(downsample_layer='conv_pool2d_v2', upsample_layer='upsample_conv2d_v2'),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_variable_table_matches_the_extended_oracle(name, monkeypatch):
    """As tests/test_variable_table_matches_oracle.py: the oracle runs on exactly the table's variables (a missing name or a shape it cannot
    use raises) and reads every generator variable of the table."""
    OLC.install(monkeypatch)
    hp = _hp(**CASES[name])
    out, P, rng = _run(hp, return_vars=True)
    total = 0.0
    for k, v in out.items():
        if torch.is_tensor(v) and v.is_floating_point() and v.requires_grad:
            total = total + (v * torch.tensor(rng.standard_normal(tuple(v.shape)))).sum()
    names = [k for k in P if k.startswith('generator/')]
    grads = torch.autograd.grad(total, [P[k] for k in names], allow_unused=True)
    unread = [k for k, g in zip(names, grads) if g is None]
    assert not unread, (name, unread)
    assert all(torch.isfinite(g).all() for g in grads)
    c = CASES[name]
    p = 'generator/rnn/savp_cell/'
    if c.get('downsample_layer') == 'conv2d':
        assert tuple(P[p + 'h0/conv2d/kernel'].shape)[:2] == (5, 5) and tuple(P[p + 'h1/conv2d/kernel'].shape)[:2] == (3, 3)
        assert not any('conv_pool2d' in k for k in P)
    if c.get('upsample_layer') == 'deconv2d':
        k3 = P[p + 'h3/deconv2d/kernel']
        assert tuple(k3.shape)[:3] == (3, 3, hp.ngf * 2), tuple(k3.shape)          # [k, k, filters, Cin]: output channels first
        assert tuple(P[p + 'h3/deconv2d/bias'].shape) == (hp.ngf * 2,)
        assert not any('upsample_conv2d' in k for k in P)
    if name == 'v2':
        assert set(P) == set(V.variable_specs(_hp(), (64, 64, 3), mode='test'))


# ---- the kernel embedding of the HIP path's 'down' / 'deconv' kinds --------------------------------------------------------------------
def embed(w):
    """What savp_fold_embed computes: [k, k, A, B] -> [k + 1, k + 1, A, B], taps at rows / columns 1..k."""
    k = w.shape[0]
    out = torch.zeros((k + 1, k + 1) + tuple(w.shape[2:]), dtype=w.dtype)
    out[1:, 1:] = w
    return out


def unembed(wf):
    return wf[1:, 1:].clone()


def symmetric_pad_conv(x, w, stride, pad):
    """The engine's geometry: one symmetric pad per axis (include/savp_hip.h: y[oy] = sum_u x[oy * s - p + u] w[u])."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), stride=stride, padding=pad)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize('k', [3, 5])
def test_embedded_kernel_in_the_pool_geometry_is_the_same_conv(k):
    from video_prediction_amd.engine import same_pad_before
    x, w = _rand((2, 8, 12, 3), 14), _rand((k, k, 3, 4), 15)
    assert torch.equal(unembed(embed(w)), w)
    pad = (same_pad_before(k + 1, 2, 8), same_pad_before(k + 1, 2, 12))
    assert pad == ((k - 1) // 2,) * 2
    got = symmetric_pad_conv(x, embed(w), 2, pad)
    assert float((got - ops.conv2d(x, w, strides=(2, 2))).abs().max()) <= TOL
    # the weight gradient read back from the same positions
    xe = embed(w).clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    dy = _rand(tuple(got.shape), 16)
    (symmetric_pad_conv(x, xe, 2, pad) * dy).sum().backward()
    (ops.conv2d(x, wr, strides=(2, 2)) * dy).sum().backward()
    assert float((unembed(xe.grad) - wr.grad).abs().max()) <= TOL


def test_deconv_is_the_data_gradient_of_the_embedded_conv():
    y, w = _rand((2, 4, 6, 3), 17), _rand((3, 3, 5, 3), 18)
    x = torch.zeros(2, 8, 12, 5, dtype=torch.float64, requires_grad=True)
    (symmetric_pad_conv(x, embed(w), 2, (1, 1)) * y).sum().backward()
    assert float((x.grad - ops.deconv2d(y, w, strides=(2, 2))).abs().max()) <= TOL

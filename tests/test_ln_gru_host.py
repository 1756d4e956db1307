"""Host side of the layer-norm ConvGRU cell (conv_rnn='gru' with conv_rnn_norm_layer='layer', opt-in; csrc/gru_two_pass.hip), no GPU: the
refusal without the opt-in, the selection with it, the variable table, the fp64 oracle cell of tests/oracle_ln_gru.py against a plain-loop
numpy restatement, and the workspace arithmetic and launch-free refusals of the new entries."""
import ctypes

import numpy as np
import pytest
import torch

import oracle.savp as OS
from tests import oracle_ln_gru as OLG
from tests.gpu_model_checks import make_hparams, make_noise, synth
from video_prediction_amd import variables as V
from video_prediction_amd.models import conv_rnn_cells as CC
from video_prediction_amd.models.savp_cell import check_norm_layers, ln_gru_opt_in

LN_GRU = dict(conv_rnn='gru', conv_rnn_norm_layer='layer')
TEXT = 'the GRU gate kernels are instance-norm only'
ENTRIES = ('savp_convgru_ln_gates_fwd', 'savp_convgru_ln_out_fwd', 'savp_convgru_ln_out_bwd', 'savp_convgru_ln_gates_bwd')


def _hp(**over):
    return make_hparams(context_frames=2, sequence_length=4, nz=8, **over)


# ---- the opt-in ---------------------------------------------------------------------------------------------------------------------
def test_refused_without_the_opt_in(monkeypatch):
    from video_prediction_amd.models.savp_model import SAVPEngine, SAVPVideoPredictionModel
    monkeypatch.delenv('SAVP_LN_GRU', raising=False)
    assert ln_gru_opt_in() is False and ln_gru_opt_in(True) is True
    hp = _hp(**LN_GRU)
    for fn in (check_norm_layers, CC.cell_class):
        with pytest.raises(NotImplementedError, match=TEXT):
            fn(hp)
        with pytest.raises(NotImplementedError, match=TEXT):
            fn(hp, ln_gru=False)
    with pytest.raises(NotImplementedError, match=TEXT):
        SAVPEngine(hp, (64, 64, 3), 2, mode='test', seed=1)
    # an explicit False wins over the environment; '0' and anything but '1' are off
    monkeypatch.setenv('SAVP_LN_GRU', '1')
    with pytest.raises(NotImplementedError, match=TEXT):
        check_norm_layers(hp, ln_gru=False)
    with pytest.raises(NotImplementedError, match=TEXT):
        SAVPEngine(hp, (64, 64, 3), 2, mode='test', seed=1, ln_gru=False)
    monkeypatch.setenv('SAVP_LN_GRU', '0')
    with pytest.raises(NotImplementedError, match=TEXT):
        CC.cell_class(hp)
    # the model class: refused when the graph is built
    monkeypatch.delenv('SAVP_LN_GRU', raising=False)
    model = SAVPVideoPredictionModel(mode='test', hparams_dict=dict(LN_GRU, context_frames=2, sequence_length=4, nz=8))
    assert model.ln_gru is False
    with pytest.raises(NotImplementedError, match=TEXT):
        model.build_graph({'images': torch.zeros(2, 4, 64, 64, 3)}, device='cpu')
    assert SAVPVideoPredictionModel(mode='test', hparams_dict=dict(LN_GRU, context_frames=2, sequence_length=4), ln_gru=True).ln_gru is True


@pytest.mark.parametrize('how', ['keyword', 'environment'])
def test_selection_with_the_opt_in(monkeypatch, how):
    if how == 'environment':
        monkeypatch.setenv('SAVP_LN_GRU', '1')
        kw = {}
    else:
        monkeypatch.delenv('SAVP_LN_GRU', raising=False)
        kw = dict(ln_gru=True)
    check_norm_layers(_hp(**LN_GRU), **kw)
    cls, out_norm = CC.cell_class(_hp(**LN_GRU), **kw)
    assert (cls, out_norm) == (CC.LayerNormGRU, False)
    assert issubclass(cls, CC.ConvGRU) and cls.has_c is False and cls.bias is False
    assert CC.cell_class(_hp(norm_layer='layer', **LN_GRU), zw=8, **kw) == (CC.LayerNormGRU, False)
    # the ablations keep their classes
    assert CC.cell_class(_hp(ablation_rnn=True, **LN_GRU), **kw) == (CC.AblationConv, False)
    assert CC.cell_class(_hp(ablation_conv_rnn_norm=True, **LN_GRU), **kw) == (CC.BareGRU, True)
    # every other refusal is unchanged
    for fn in (check_norm_layers, CC.cell_class):
        with pytest.raises(NotImplementedError, match='the untiled latent is only cancelled by an instance norm'):
            fn(_hp(use_tile_concat=False, **LN_GRU), **kw)
        with pytest.raises(NotImplementedError, match="conv_rnn_norm_layer='batch'"):
            fn(_hp(conv_rnn='gru', conv_rnn_norm_layer='batch'), **kw)
    # ... and every other row of the matrix
    assert CC.cell_class(_hp(conv_rnn='gru'), **kw) == (CC.InstanceNormGRU, False)
    assert CC.cell_class(_hp(conv_rnn_norm_layer='layer'), **kw) == (CC.LayerNormLSTM, False)
    assert CC.cell_class(_hp(), **kw) == (CC.InstanceNormLSTM, False)


# ---- the variable table -------------------------------------------------------------------------------------------------------------
GRU_LAYERS_64 = (0, 1, 2, 3, 4)          # every ladder layer but the last is recurrent at 64 x 64


def test_variable_table():
    hp = _hp(ngf=8, **LN_GRU)
    specs = V.variable_specs(hp, (64, 64, 3), mode='test')
    widths = {0: 8, 1: 16, 2: 32, 3: 16, 4: 8}
    cell_norm_names = sorted(k for k in specs if '/conv2dgru_cell/' in k and k.rsplit('/', 1)[-1] in ('gamma', 'beta'))
    want = {}
    for i in GRU_LAYERS_64:
        s, f = 'generator/rnn/savp_cell/gru_h%d/conv2dgru_cell/' % i, widths[i]
        want[s + 'gates/reset/gamma'] = ((f,), 'ones')
        want[s + 'gates/reset/beta'] = ((f,), 'ones')
        want[s + 'gates/update/gamma'] = ((f,), 'ones')
        want[s + 'gates/update/beta'] = ((f,), 'ones')
        want[s + 'candidate/state/gamma'] = ((f,), 'ones')
        want[s + 'candidate/state/beta'] = ((f,), 'zeros')
    assert cell_norm_names == sorted(want)
    for k, v in want.items():
        assert specs[k] == v, k
    assert not [k for k in specs if 'reset_update' in k]
    assert not [k for k in specs if '/conv2dgru_cell/' in k and k.endswith('bias')]
    vals = V.init_variables(specs, seed=4)
    s = 'generator/rnn/savp_cell/gru_h0/conv2dgru_cell/'
    assert (vals[s + 'gates/reset/beta'] == 1).all() and (vals[s + 'gates/update/beta'] == 1).all()
    assert (vals[s + 'candidate/state/beta'] == 0).all() and (vals[s + 'gates/update/gamma'] == 1).all()
    # everything outside the cell's norms is what gru + instance has
    inst = V.variable_specs(_hp(ngf=8, conv_rnn='gru'), (64, 64, 3), mode='test')
    assert {k: v for k, v in specs.items() if k not in want} == {k: v for k, v in inst.items() if 'reset_update' not in k and
                                                                  'candidate/state' not in k}


def test_variable_table_of_gru_instance_is_unchanged():
    specs = V.variable_specs(_hp(ngf=8, conv_rnn='gru'), (64, 64, 3), mode='test')
    for i, f in zip(GRU_LAYERS_64, (8, 16, 32, 16, 8)):
        s = 'generator/rnn/savp_cell/gru_h%d/conv2dgru_cell/' % i
        assert specs[s + 'gates/reset_update/gamma'] == ((2 * f,), 'ones') and specs[s + 'gates/reset_update/beta'] == ((2 * f,), 'ones')
        assert specs[s + 'candidate/state/gamma'] == ((f,), 'ones') and specs[s + 'candidate/state/beta'] == ((f,), 'zeros')
        assert s + 'gates/reset/gamma' not in specs and s + 'gates/update/gamma' not in specs
    names = [k for k in specs if '/conv2dgru_cell/' in k and k.rsplit('/', 1)[-1] in ('gamma', 'beta')]
    assert len(names) == 4 * len(GRU_LAYERS_64)


# ---- the oracle cell ----------------------------------------------------------------------------------------------------------------
def _np_layer_norm(x, gamma, beta):
    """tf.contrib.layers.layer_norm in plain loops: per sample, mean and biased variance over every other element, eps 1e-12."""
    N, H, W, C = x.shape
    out = np.zeros_like(x)
    for n in range(N):
        tot = 0.0
        for i in range(H):
            for j in range(W):
                for c in range(C):
                    tot += x[n, i, j, c]
        mean = tot / (H * W * C)
        sq = 0.0
        for i in range(H):
            for j in range(W):
                for c in range(C):
                    sq += (x[n, i, j, c] - mean) ** 2
        inv = 1.0 / np.sqrt(sq / (H * W * C) + 1e-12)
        for i in range(H):
            for j in range(W):
                for c in range(C):
                    out[n, i, j, c] = (x[n, i, j, c] - mean) * inv * gamma[c] + beta[c]
    return out


def _np_conv_same(x, k):
    """5x5 stride-1 SAME correlation, NHWC x HWIO, in plain loops."""
    N, H, W, Ci = x.shape
    kh, kw, _, Co = k.shape
    out = np.zeros((N, H, W, Co))
    for n in range(N):
        for i in range(H):
            for j in range(W):
                for a in range(kh):
                    for b in range(kw):
                        ii, jj = i + a - kh // 2, j + b - kw // 2
                        if 0 <= ii < H and 0 <= jj < W:
                            out[n, i, j] += x[n, ii, jj] @ k[a, b]
    return out


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def test_oracle_cell_against_a_plain_loop_restatement():
    N, H, W, F, Cx = 2, 3, 3, 4, 4
    rng = np.random.default_rng(11)
    x, h = rng.standard_normal((N, H, W, Cx)), rng.standard_normal((N, H, W, F))
    P = {'conv2dgru_cell/gates/kernel': 0.3 * rng.standard_normal((5, 5, Cx + F, 2 * F)),
         'conv2dgru_cell/candidate/kernel': 0.3 * rng.standard_normal((5, 5, Cx + 2 * F, F))}
    for nm in ('gates/reset', 'gates/update', 'candidate/state'):
        P['conv2dgru_cell/%s/gamma' % nm] = 1 + 0.3 * rng.standard_normal(F)
        P['conv2dgru_cell/%s/beta' % nm] = 0.5 * rng.standard_normal(F)
    read = set()

    class Rec(dict):
        def __getitem__(self, k):
            read.add(k)
            return dict.__getitem__(self, k)

    Pt = Rec({k: torch.tensor(v, dtype=torch.float64) for k, v in P.items()})
    got, state = OLG.conv_gru_cell_separate(OS.Scope(Pt), torch.tensor(x), torch.tensor(h), F)
    assert state is got and read == set(P)
    # one step, restated
    xh = np.concatenate([x, h], axis=-1)
    gates = _np_conv_same(xh, P['conv2dgru_cell/gates/kernel'])
    r = _sigmoid(_np_layer_norm(gates[..., :F], P['conv2dgru_cell/gates/reset/gamma'], P['conv2dgru_cell/gates/reset/beta']))
    u = _sigmoid(_np_layer_norm(gates[..., F:], P['conv2dgru_cell/gates/update/gamma'], P['conv2dgru_cell/gates/update/beta']))
    cand = _np_conv_same(np.concatenate([xh, r * h], axis=-1), P['conv2dgru_cell/candidate/kernel'])
    c = np.tanh(_np_layer_norm(cand, P['conv2dgru_cell/candidate/state/gamma'], P['conv2dgru_cell/candidate/state/beta']))
    want = u * h + (1 - u) * c
    assert float(np.abs(got.numpy() - want).max()) <= 1e-12
    # the two gates have their own statistics: a joint norm over the 2F channels gives another answer
    joint = _np_layer_norm(gates, np.ones(2 * F), np.zeros(2 * F))
    assert float(np.abs(joint[..., :F] - _np_layer_norm(gates[..., :F], np.ones(F), np.zeros(F))).max()) > 1e-3


def test_oracle_branch_reads_every_variable_of_the_table(monkeypatch):
    """generator_fn of the extended oracle on the table's variables: all six norm variables of every GRU layer are read, and the other
    branches are handed over (gru + instance still runs the original cell)."""
    OLG.install(monkeypatch)
    hp = _hp(ngf=8, nef=8, **LN_GRU)
    specs = V.variable_specs(hp, (32, 32, 3), mode='test')
    vals = V.init_variables(specs, seed=4)
    read = set()

    class Rec(dict):
        def __getitem__(self, k):
            read.add(k)
            return dict.__getitem__(self, k)

    P = Rec({k: torch.tensor(v, dtype=torch.float64) for k, v in vals.items()})
    out = OS.generator_fn(OS.Scope(P).sub('generator'), {'images': synth(hp, 2, 32, 32, 3, 0)}, 'test', hp, make_noise(hp, 2, sampling=True))
    assert bool(torch.isfinite(out['gen_images']).all())
    six = {k for k in specs if '/conv2dgru_cell/' in k and k.rsplit('/', 1)[-1] in ('gamma', 'beta')}
    assert len(six) == 6 * 3 and six <= read          # three recurrent layers at 32 x 32
    hp2 = _hp(ngf=8, nef=8, conv_rnn='gru')
    v2 = V.init_variables(V.variable_specs(hp2, (32, 32, 3), mode='test'), seed=4)
    P2 = {k: torch.tensor(v, dtype=torch.float64) for k, v in v2.items()}
    OS.generator_fn(OS.Scope(P2).sub('generator'), {'images': synth(hp2, 2, 32, 32, 3, 0)}, 'test', hp2, make_noise(hp2, 2, sampling=True))


# ---- the entries, without a launch --------------------------------------------------------------------------------------------------
def test_chunk_and_workspace_arithmetic(hip_lib):
    from video_prediction_amd import kernels as K
    for N in (1, 2, 3, 32):
        for HW in (1, 33, 97, 1024, 1280, 4800, 70000):
            c = K.convgru_ln_chunk(N, HW)
            assert c == hip_lib.savp_convgru_ln_chunk(N, HW) == hip_lib.savp_convgru_large_chunk(N, HW) and c >= 1
            for F in (4, 32, 264):
                assert K.convgru_ln_ws_bytes(N, HW, F) == N * ((HW + c - 1) // c) * 4 * F * 8 == hip_lib.savp_convgru_ln_ws_bytes(N, HW, F)
    assert K.convgru_ln_chunk(0, 16) == 0 == hip_lib.savp_convgru_ln_chunk(0, 16)
    assert K.convgru_ln_ws_bytes(2, 0, 8) == 0 == hip_lib.savp_convgru_ln_ws_bytes(2, 0, 8)


def _args(lib, N=1, HW=1280, F=8, ws_bytes=None):
    """A gates-forward problem over made-up (never dereferenced) aligned addresses."""
    a = lib.SavpGruLargeArgs()
    a.g.N, a.g.HW, a.g.F, a.g.eps = N, HW, F, 1e-12
    a.g.pre, a.g.gamma, a.g.beta, a.g.mean, a.g.rstd, a.g.u = 0x100000, 0x200000, 0x210000, 0x220000, 0x230000, 0x300000
    a.g.h.p, a.g.h.sn, a.g.h.sp = 0x400000, HW * F, F
    a.g.rh.p, a.g.rh.sn, a.g.rh.sp = 0x500000, HW * F, F
    a.ws = 0x600000
    a.ws_bytes = 8 * N * ((HW + 31) // 32) * 4 * F if ws_bytes is None else ws_bytes
    return a


def test_entries_refuse_without_a_launch(hip_lib):
    from video_prediction_amd import kernels as K
    from video_prediction_amd import lib
    for nm in ENTRIES:
        assert getattr(hip_lib, nm)(None, None) == -1
    fwd = hip_lib.savp_convgru_ln_gates_fwd
    need = hip_lib.savp_convgru_ln_ws_bytes(1, 1280, 8)
    assert _args(lib).ws_bytes == need

    def bad(**edit):
        a = _args(lib, **{k: v for k, v in edit.items() if k in ('N', 'HW', 'F', 'ws_bytes')})
        for k, v in edit.items():
            if k not in ('N', 'HW', 'F', 'ws_bytes'):
                obj, leaf = a, k.split('.')
                for part in leaf[:-1]:
                    obj = getattr(obj, part)
                setattr(obj, leaf[-1], v)
        return fwd(None, ctypes.byref(a))
    assert bad(F=6) == -1 and bad(F=0) == -1 and bad(N=0) == -1 and bad(HW=0) == -1 and bad(F=K.LN_GRU_MAX_F + 4) == -1
    assert bad(ws_bytes=need - 8) == -1 and bad(ws=None) == -1 and bad(ws=0x600004) == -1
    assert bad(**{'g.pre': None}) == -1 and bad(**{'g.u': None}) == -1 and bad(**{'g.mean': None}) == -1 and bad(**{'g.h.p': None}) == -1
    assert bad(**{'g.pre': 0x100008}) == -1 and bad(**{'g.h.p': 0x400008}) == -1 and bad(**{'g.rh.sp': 10}) == -1 and bad(**{'g.h.sn': 1282}) == -1
    assert bad(**{'g.mean': 0x220002}) == -1

"""The conv-RNN cell of a recurrent ladder layer: one class per variant of the matrix in DESIGN.md section 1, chosen by cell_class(hp).

A cell owns everything about its variant: its buffers, ConvLayers, Norms and workspaces, the launches of a time step forward and backward,
its weight gradients and its share of the z gradient.  SAVPGenerator (savp_cell.py) builds one per recurrent layer and calls only this
interface; a new variant is a new class here and a new row in cell_class.  The cell lives beside the layer's dict as L['cell'] and keeps
its buffers in that dict under fixed names (L['a'], L['gates'], L['rconv'], ...): bench.py and the tests read them, and bench.py's timer
hooks (L['cell_prof'], L['gate_ktimer'], L['cell_ktimer']) are set after construction, so they are looked up at every call.

The layer's first convolution + norm (SAVPGenerator._conv_in_act / _in_act_conv_bwd / _norm_bwd) is shared by all variants and stays a
generator method that the cells call.  Kernel wrappers are looked up as attributes of K when called (tests replace them on the module).
"""
import os

import torch

from .. import kernels as K
from ..engine import ConvLayer, add_views
from . import savp_cell as S      # Act, Norm, ConcatNorm, norm_fwd / norm_bwd and the module switches; the two modules import each other,
                                  # so everything of S is read when a cell is built or called, never while this module is imported


def cell_class(hp, zw=0, ln_gru=None, norm_none=None):
    """(class, out_norm) of the conv-RNN layers under `hp`.  out_norm: ablation_conv_rnn_norm, the bare cell's output h -- not the state
    handed to the next step -- goes through normalizer_fn (savp_model.py:380-384).  zw: width of the tiled slice [actions | state | z].
    ln_gru: the opt-in of LayerNormGRU (S.ln_gru_opt_in: None reads SAVP_LN_GRU); without it ('gru', 'layer') is refused.
    norm_none: the opt-in of norm_layer='none' (S.norm_none_opt_in: None reads SAVP_NORM_NONE); without it that value is refused."""
    S.check_norm_layers(hp, ln_gru, zw=zw, norm_none=norm_none)      # (also refuses the untiled latent of a bare cell where nothing cancels it)
    out_norm = bool(hp.ablation_conv_rnn_norm)
    # The cell WITHOUT a normaliser (ConvLSTM, rnn_ops.py:122-125: the gate convolution then has a bias; ConvGRU, :220-223: both
    # convolutions have one): conv_rnn_norm_layer = 'none', or ablation_conv_rnn_norm
    bare = hp.conv_rnn_norm_layer == 'none' or out_norm
    if out_norm and hp.conv_rnn_norm_layer == 'none':
        raise TypeError("ablation_conv_rnn_norm with conv_rnn_norm_layer='none': the reference calls normalizer_fn = None (savp_model.py:384)")
    if hp.ablation_rnn:
        return AblationConv, False
    if hp.conv_rnn == 'gru' and bare:
        return BareGRU, out_norm
    if hp.conv_rnn == 'gru':
        # 'layer' gets here with the opt-in only (check_norm_layers above)
        return (LayerNormGRU if hp.conv_rnn_norm_layer == 'layer' else InstanceNormGRU), False
    if bare:
        return BareLSTM, out_norm
    return (LayerNormLSTM if hp.conv_rnn_norm_layer == 'layer' else InstanceNormLSTM), False


class ConvRNNCell(object):
    """What the variants share: the layer's input buffer a = [x | tiled z | h_prev ...] with the next step's h slot, the first
    convolution + norm in front of the cell, the output norm of ablation_conv_rnn_norm, the learned initial state and the z gradient."""
    has_c = False          # the state is the LSTM tuple (c, h), not h alone

    def __init__(self, gen, L, prefix, out_norm=False):
        self.gen, self.L, self.out_norm = gen, L, out_norm
        self.f, self.hs = L['f'], L['f'] + L['zr']          # channels of x and of h; offset of h_prev in a
        self.plane = (gen.T1, gen.N) + L['hw']

    def _act(self, c, **kw):
        return S.Act(self.plane + (c,), self.gen.dev, grad=kw.pop('grad', self.gen.train), **kw)

    def _step(self, c):
        """A one-step gradient scratch [N, h, w, c] (train only)."""
        return torch.empty(self.plane[1:] + (c,), device=self.gen.dev) if self.gen.train else None

    # ---- the state slots ----
    def h_next(self, t):
        f, hs = self.f, self.hs
        return [self.L['a'].v[t + 1][..., hs:hs + f]] if t + 1 < self.gen.T1 else []

    def dh_next(self, t):
        f, hs = self.f, self.hs
        return [self.L['a'].g[t + 1][..., hs:hs + f]] if t + 1 < self.gen.T1 else []

    def c_prev(self, t):
        return self.L['c'].v[t - 1] if t > 0 else self.L.get('c0')

    def dc(self, t):
        """(gradient of step t's new c handed down by step t + 1, where step t leaves the gradient of its c_prev): a ping-pong pair."""
        dc = self.L['dc']
        return (dc[(t + 1) & 1] if t + 1 < self.gen.T1 else None), (dc[t & 1] if (t > 0 or self.gen.learn_init) else None)

    # ---- the layer's first convolution + norm, written into x of a ----
    def _in_fwd(self, t, st):
        L = self.L
        self.gen._conv_in_act(L['conv'], L['in'].v[t], L['pre'].v[t], st, L['norm'], [L['a'].v[t][..., 0:self.f]], t)

    def _in_bwd(self, t, st=None):
        a = self.L['a']
        self.gen._in_act_conv_bwd(self.L, t, a.v[t][..., 0:self.f], [a.g[t][..., 0:self.f]], st)

    # ---- ablation_conv_rnn_norm: normalizer_fn(h) on the layer's output, the state stays un-normalised ----
    def _make_out_norm(self, scope):
        if self.out_norm:
            self.L['h_raw'] = self._act(self.f)
            self.L['onorm'] = self.gen._norm(scope, self.f, self.gen.hp.conv_rnn_norm_layer)

    def h_dst(self, t):
        """Where the cell writes h': the layer's outputs (the raw buffer under an output norm) and the next step's state slot."""
        return ([self.L['h_raw'].v[t]] if self.out_norm else self.gen._out_views(self.L, t)) + self.h_next(t)

    def out_norm_fwd(self, t):
        if self.out_norm:
            L, on = self.L, self.L['onorm']
            S.norm_fwd(on, L['h_raw'].v[t], self.gen._out_views(L, t), on.mean[t], on.rstd[t], act='none', eps=S.EPS_IN)

    def dh(self, t, dys):
        """The gradients of h': those of the layer's outputs (through the output norm, if any) and the next step's."""
        if self.out_norm:
            L, on = self.L, self.L['onorm']
            S.norm_bwd(on, L['h_raw'].v[t], self.gen._out_views(L, t)[0], on.mean[t], on.rstd[t], dys, L['h_raw'].g[t], on.dgamma, on.dbeta,
                       act='none', eps=S.EPS_IN)
            dys = [L['h_raw'].g[t]]
        return dys + self.dh_next(t)

    # ---- learn_initial_state: variables in nest.flatten order, LSTM tuples as (c, h) ----
    def make_initial_state(self, var):
        L, hw_f = self.L, self.L['hw'] + (self.f,)
        if self.has_c:
            L['c0v'], L['c0g'] = var(hw_f)
            L['c0'] = torch.empty((self.gen.N,) + hw_f, device=self.gen.dev)
        L['h0v'], L['h0g'] = var(hw_f)

    def load_initial_state(self):
        L, f, hs = self.L, self.f, self.hs
        L['a'].v[0][..., hs:hs + f].copy_(L['h0v'])
        if self.has_c:
            L['c0'].copy_(L['c0v'])

    def initial_state_grad(self):
        L, f, hs = self.L, self.f, self.hs
        L['h0g'].add_(L['a'].g[0][..., hs:hs + f].float().sum(0))
        if self.has_c:
            L['c0g'].add_(L['dc'][0].sum(0))

    # ---- the interface beside forward(t, st) / backward(t, dys) ----
    def convs(self):
        return [self.L['rconv']]

    def prep(self):
        pass

    def backward_weights(self):
        a, gt = self.L['a'], self.L['gates']
        self.L['rconv'].backward_weights(a.flat(a.v), gt.flat(gt.g))

    def z_gradient(self, drz):
        """Adds the gradient of the z channels tiled into a (the conditioning columns in front of them are inputs: skipped)."""
        a, z0, nz = self.L['a'], self.f + self.gen.cw, self.gen.nz
        K.colsum(a.flat(a.g)[..., z0:z0 + nz], drz, per_row=True)


class AblationConv(ConvRNNCell):
    """ablation_rnn (savp_model.py:466-474,502-509): no recurrent state, conv2d 5x5 (+ tiled z) -> norm -> activation under conv_h<i>."""

    def __init__(self, gen, L, prefix, out_norm=False):
        super(AblationConv, self).__init__(gen, L, prefix)
        f, r, cin = self.f, prefix + 'conv_h%d/' % L['idx'], S.ceil4(L['f'] + L['zr'])
        a16 = torch.bfloat16 if gen.act16 else torch.float32
        L['a'] = self._act(cin, dtype=a16 if cin % 8 == 0 else torch.float32)
        L['pre2'] = self._act(f, grad_dtype=a16 if f % 8 == 0 else torch.float32)
        L['rconv'] = ConvLayer(gen.store, r + 'conv2d/kernel', r + 'conv2d/bias', 'conv', (5, 5), (1, 1), (2, 2), cx_pad=cin)
        L['n2'] = gen._norm(r, f, bias=r + 'conv2d/bias')
        hp = gen.hp
        if gen.nn and not hp.use_tile_concat and hp.where_add == 'all' and gen.zw:
            gen._untiled(L['n2'], r)          # no norm cancels conv_h<i>/dense(z) either (savp_model.py:475,511)

    def forward(self, t, st):
        L = self.L
        self._in_fwd(t, st)
        if self.gen.nn:
            L['n2'].add_fwd(t)
        self.gen._conv_norm(('abl', L['idx']), L['rconv'], L['a'].v[t], L['pre2'].v[t], L['n2'], self.gen._out_views(L, t), t)

    def backward(self, t, dys):
        L, n2 = self.L, self.L['n2']
        S.norm_bwd(n2, L['pre2'].v[t], self.gen._out_views(L, t)[0], n2.mean[t], n2.rstd[t], dys, L['pre2'].g[t], n2.dgamma, n2.dbeta,
                   act=self.gen.act, eps=S.EPS_IN)
        L['rconv'].backward_data(L['pre2'].g[t], L['a'].g[t], beta=0)
        self._in_bwd(t)

    def backward_weights(self):
        a, p2 = self.L['a'], self.L['pre2']
        self.L['rconv'].backward_weights(a.flat(a.v), p2.flat(p2.g), **self.gen.wkw)


class ConvGRU(ConvRNNCell):
    """Conv2DGRUCell (rnn_ops.py:174-267): a = [x | z | h_prev | r*h_prev]; the gates conv reads the first f+zc+f channels of the same
    buffer (a channel-slice view), the candidate conv reads all of it.  The four gate blocks are one call each of a wrapper in K: a
    subclass names them in `blocks` (a table like GRU_BLOCKS, resolved when called) and sets self.norms = (the norm of the gates, the norm
    of the candidate, the workspace arguments, eps) -- (None, None, (), None) without a normaliser."""
    bias = False           # without a normaliser the two convolutions carry a bias (rnn_ops.py:220-223)
    blocks = None

    def __init__(self, gen, L, prefix, out_norm=False):
        super(ConvGRU, self).__init__(gen, L, prefix, out_norm)
        f, zr = self.f, L['zr']
        self.scope = r = prefix + 'gru_h%d/conv2dgru_cell/' % L['idx']
        L['cin1'] = f + zr + f
        L['a'] = self._act(f + zr + 2 * f)
        L['gates'] = self._act(2 * f)
        L['cand'] = self._act(f)
        L['u'] = torch.empty(self.plane + (f,), device=gen.dev)
        L['du'] = self._step(f)
        L['dh_tmp'] = self._step(f)
        L['rconv'] = ConvLayer(gen.store, r + 'gates/kernel', (r + 'gates/bias') if self.bias else None, 'conv', (5, 5), (1, 1), (2, 2))
        L['cconv'] = ConvLayer(gen.store, r + 'candidate/kernel', (r + 'candidate/bias') if self.bias else None, 'conv', (5, 5), (1, 1), (2, 2))

    def convs(self):
        return [self.L['rconv'], self.L['cconv']]

    def _slots(self, buf):
        """(h_prev, r*h_prev) channels of a step's a (or of its gradient)."""
        f, hs = self.f, self.hs
        return buf[..., hs:hs + f], buf[..., hs + f:hs + 2 * f]

    def forward(self, t, st):
        L, a, nrm = self.L, self.L['a'], self.L['norm']
        L['conv'].forward(L['in'].v[t], L['pre'].v[t], stats=st)
        S.norm_fwd(nrm, L['pre'].v[t], [a.v[t][..., 0:self.f]], nrm.mean[t], nrm.rstd[t],
                   act=self.gen.act, eps=S.EPS_IN, stats=st, stats_shift=L['conv'].bias if st is not None else None)
        hprev, rh = self._slots(a.v[t])
        L['rconv'].forward(a.v[t][..., 0:L['cin1']], L['gates'].v[t])              # (+ bias: the bare cell)
        self.gates_fwd(t, hprev, rh)
        L['cconv'].forward(a.v[t], L['cand'].v[t])
        self.out_fwd(t, hprev, self.h_dst(t))
        self.out_norm_fwd(t)

    def backward(self, t, dys):
        L, a, nrm, f = self.L, self.L['a'], self.L['norm'], self.f
        dys = self.dh(t, dys)
        hprev = self._slots(a.v[t])[0]
        dhprev, drh = self._slots(a.g[t])
        self.out_bwd(t, hprev, dys)
        L['cconv'].backward_data(L['cand'].g[t], a.g[t], beta=0)
        add_views([L['dh_tmp']], dhprev)
        self.gates_bwd(t, hprev, drh, dhprev)
        L['rconv'].backward_data(L['gates'].g[t], a.g[t][..., 0:L['cin1']], beta=1)
        S.norm_bwd(nrm, L['pre'].v[t], a.v[t][..., 0:f], nrm.mean[t], nrm.rstd[t], [a.g[t][..., 0:f]], L['pre'].g[t], nrm.dgamma, nrm.dbeta,
                   act=self.gen.act, eps=S.EPS_IN)
        L['conv'].backward_data(L['pre'].g[t], L['in'].g[t], beta=0)

    def backward_weights(self):
        a, gt, cd = self.L['a'], self.L['gates'], self.L['cand']
        self.L['rconv'].backward_weights(a.flat(a.v)[..., 0:self.L['cin1']], gt.flat(gt.g))
        self.L['cconv'].backward_weights(a.flat(a.v), cd.flat(cd.g))

    # ---- the four gate blocks ----
    def _block(self, which, t, norm, pre, hprev, *operands):
        """K.<blocks[which]>(pre, h, [gamma, beta, mean, rstd,] operands, [dgamma, dbeta,] [workspace,] [eps])."""
        ws, eps = self.norms[2:]
        if norm is None:
            args = operands
        else:
            args = (norm.gamma, norm.beta, norm.mean[t], norm.rstd[t]) + operands + \
                   ((norm.dgamma, norm.dbeta) if which.endswith('bwd') else ()) + ws + (eps,)
        getattr(K, self.blocks[which])(pre, hprev, *args)
        if 'gru_large_calls' in self.L:
            self.L['gru_large_calls'] += 1

    def gates_fwd(self, t, hprev, rh):
        self._block('gates_fwd', t, self.norms[0], self.L['gates'].v[t], hprev, self.L['u'][t], rh)

    def out_fwd(self, t, hprev, hdst):
        self._block('out_fwd', t, self.norms[1], self.L['cand'].v[t], hprev, self.L['u'][t], hdst)

    def out_bwd(self, t, hprev, dys):
        L = self.L
        self._block('out_bwd', t, self.norms[1], L['cand'].v[t], hprev, L['u'][t], dys, L['cand'].g[t], L['du'], L['dh_tmp'])

    def gates_bwd(self, t, hprev, drh, dhprev):
        L = self.L
        self._block('gates_bwd', t, self.norms[0], L['gates'].v[t], hprev, L['du'], drh, L['gates'].g[t], dhprev)


# the gate blocks by family: names of wrappers in K, resolved when called
GRU_BLOCKS, GRU_LARGE_BLOCKS, LN_GRU_BLOCKS, BARE_GRU_BLOCKS = (
    {b: 'convgru_' + fam + b for b in ('gates_fwd', 'out_fwd', 'out_bwd', 'gates_bwd')} for fam in ('', 'large_', 'ln_', 'plain_'))


class InstanceNormGRU(ConvGRU):
    """The GRU cell with its instance norms (gates/reset_update, candidate/state) inside the gate blocks.  A plane the one-workgroup
    blocks (csrc/gru.hip) hold runs on them; a larger one (gru_large_layers) on the chunked two-pass blocks (csrc/gru_two_pass.hip), which
    take a per-layer workspace as one more argument.  The choice is made here, once per layer."""

    def __init__(self, gen, L, prefix, out_norm=False):
        super(InstanceNormGRU, self).__init__(gen, L, prefix)
        f, (h_, w_), r = self.f, L['hw'], self.scope
        L['n1'] = S.Norm(gen.store, r + 'gates/reset_update/', gen.T1, gen.N, 2 * f, gen.dev)
        L['n2'] = S.Norm(gen.store, r + 'candidate/state/', gen.T1, gen.N, f, gen.dev)
        L['gru_large'] = h_ * w_ > K.GRU_SMALL_MAX_HW
        if L['gru_large'] and gen.train:
            # Training at such frames is not pinned against the oracle yet: the ConvLSTM twin's train step misses the fp64 gradient
            # bounds at 64x80 (a video discriminator kernel) and at 96x96 (the latent LSTM's kernel), see profiles/gru_large.md.
            # The backward blocks below are wired and tested on their own; this refusal goes when that finding is settled.
            raise NotImplementedError("conv_rnn='gru' with its instance norm on a conv-RNN plane of %dx%d = %d pixels (layer h%d, above "
                                      "%d): mode='train' is not offered at this frame size yet, generation and evaluation are "
                                      "(profiles/gru_large.md)" % (h_, w_, h_ * w_, L['idx'], K.GRU_SMALL_MAX_HW))
        self.blocks, ws = GRU_BLOCKS, ()
        if L['gru_large']:
            L['gru_ws'] = K.convgru_large_ws(gen.dev, gen.N, h_ * w_, f)
            L['gru_large_calls'] = 0          # counts the calls of the large blocks (tests read it)
            self.blocks, ws = GRU_LARGE_BLOCKS, (L['gru_ws'],)
        self.norms = (L['n1'], L['n2'], ws, S.EPS_IN)


class LayerNormGRU(ConvGRU):
    """conv_rnn_norm_layer = 'layer' inside the GRU cell (separate_norms, rnn_ops.py:234-267): the gates convolution (no bias), a layer
    norm each for reset and update (one G = 2 block, parameters gathered per step), the candidate convolution, a layer norm of the
    candidate, h'.  The norms run inside the chunked two-pass gate blocks of csrc/gru_two_pass.hip: one code path for every plane size, a
    per-layer workspace created here, no normalised tensor stored.  Opt-in (S.ln_gru_opt_in)."""
    blocks = LN_GRU_BLOCKS

    def __init__(self, gen, L, prefix, out_norm=False):
        super(LayerNormGRU, self).__init__(gen, L, prefix)
        f, (h_, w_), r = self.f, L['hw'], self.scope
        if h_ * w_ > K.GRU_SMALL_MAX_HW and gen.train:
            # as for InstanceNormGRU: the train step is not pinned against the oracle at such frames (profiles/gru_large.md)
            raise NotImplementedError("conv_rnn='gru' with its layer norm on a conv-RNN plane of %dx%d = %d pixels (layer h%d, above "
                                      "%d): mode='train' is not offered at this frame size yet, generation and evaluation are "
                                      "(profiles/gru_large.md)" % (h_, w_, h_ * w_, L['idx'], K.GRU_SMALL_MAX_HW))
        # reset / update: one G = 2 launch over the gate tensor
        L['gn2'] = S.ConcatNorm([S.Norm(gen.store, r + 'gates/' + nm + '/', gen.T1, gen.N, f, gen.dev, groups=1)
                                 for nm in ('reset', 'update')], gen.T1, gen.N, gen.dev)
        L['nC'] = S.Norm(gen.store, r + 'candidate/state/', gen.T1, gen.N, f, gen.dev, groups=1)
        L['ln_gru_ws'] = K.convgru_ln_ws(gen.dev, gen.N, h_ * w_, f)
        self.norms = (L['gn2'], L['nC'], (L['ln_gru_ws'],), K.EPS_LN)

    def prep(self):
        self.L['gn2'].prep()

    def backward_weights(self):
        super(LayerNormGRU, self).backward_weights()
        self.L['gn2'].finish()


class BareGRU(ConvGRU):
    """The GRU cell without a normaliser: conv + bias, pointwise gate blocks of any plane size (csrc/gru.hip)."""
    bias = True
    blocks = BARE_GRU_BLOCKS

    def __init__(self, gen, L, prefix, out_norm=False):
        super(BareGRU, self).__init__(gen, L, prefix, out_norm)
        self._make_out_norm(prefix + 'gru_h%d/' % L['idx'])
        self.norms = (None, None, (), None)


class ConvLSTM(ConvRNNCell):
    """BasicConv2DLSTMCell (rnn_ops.py:137-171): a = [x | z | h_prev], one 5x5 gate convolution to 4f channels, the state c per step.
    Holds the buffers all three variants share and the gate block of csrc/lstm.hip, which runs with the cell's two instance norms
    (L['n1'] over the gates, L['n2'] over the new state) or, where the cell has none, without."""
    has_c = True
    bias = False           # without a normaliser the gate convolution has a bias (rnn_ops.py:122-125)
    fusable = False        # the fused cell of the bf16 datapath: the instance-norm variant only

    def __init__(self, gen, L, prefix, out_norm=False):
        super(ConvLSTM, self).__init__(gen, L, prefix, out_norm)
        f, zr, (h_, w_), g = self.f, L['zr'], L['hw'], gen.train
        self.scope = r = prefix + 'lstm_h%d/basic_conv2dlstm_cell/' % L['idx']
        # fused ConvLSTM cell of the bf16 datapath: the gate convolution's epilogue produces the statistics of the first
        # instance norm and stores the gate pre-activations as bf16 (csrc/conv_ring.hip) -> conv + 2 launches per cell
        L['fused'] = bool(self.fusable and K.PRECISION['value'] == 1 and os.environ.get('SAVP_FUSED_CELL', '1') == '1' and
                          h_ % 8 == 0 and w_ % 8 == 0 and 16 <= f <= 256 and (f & (f - 1)) == 0 and (f + zr + f) % 8 == 0)
        # The cell's input buffer [x | z | h] and the gate gradient are held in bf16 (round 3: validated on MI355X, identical
        # numbers -- their only readers are the gate convolution's FPROP / DGRAD / WGRAD, which round to bf16 when they stage
        # their operands anyway -- and half the bytes; step time unchanged within noise, 61.04 vs 61.21 ms).  The producers
        # (instance norm of the layer's conv, tile_channels, the h' output and the gate gradient of the gate kernels) write bf16
        # through their out_bf16 / h_bf16 / dgates_bf16 flags.  SAVP_BF16_ACT=0 / SAVP_BF16_DGATES=0 keep fp32 tensors.
        a_dt = torch.bfloat16 if (L['fused'] and os.environ.get('SAVP_BF16_ACT', '1') == '1') else torch.float32
        L['a'] = self._act(f + zr + f, dtype=a_dt)
        dg_dt = torch.bfloat16 if (L['fused'] and g and os.environ.get('SAVP_BF16_DGATES', '1') == '1') else torch.float32
        L['gates'] = self._act(4 * f, dtype=torch.bfloat16 if L['fused'] else torch.float32, grad_dtype=dg_dt)
        L['dg_raw'] = torch.empty(self.plane[1:] + (4 * f,), device=gen.dev) if dg_dt == torch.bfloat16 else None
        L['c'] = self._act(f, grad=False)
        L['dc'] = [self._step(f), self._step(f)] if g else None
        L['rconv'] = ConvLayer(gen.store, r + 'kernel', (r + 'bias') if self.bias else None, 'conv', (5, 5), (1, 1), (2, 2))
        L['zless'] = False          # see InstanceNormLSTM

    def _norm_args(self, t):
        """(gamma1, beta1, gamma2, beta2), the saved statistics and the parameter-gradient accumulators of n1 / n2; Nones without them."""
        n1, n2 = self.L.get('n1'), self.L.get('n2')
        if n1 is None:
            return (None, None, None, None), None, None
        return (n1.gamma, n1.beta, n2.gamma, n2.beta), [n1.mean[t], n1.rstd[t], n2.mean[t], n2.rstd[t]], [n1.dgamma, n1.dbeta, n2.dgamma, n2.dbeta]

    def _gates_fwd(self, t, hdst, **kw):
        L, (params, stats, _) = self.L, self._norm_args(t)
        return K.convlstm_gates_fwd(L['gates'].v[t], self.c_prev(t), *params, L['c'].v[t], hdst, stats, **kw)

    def _gates_bwd(self, t, dys, **kw):
        L, (params, stats, dparams), (dc_new, dc_prev) = self.L, self._norm_args(t), self.dc(t)
        return K.convlstm_gates_bwd(L['gates'].v[t], self.c_prev(t), *params, stats, dys, dc_new, L['gates'].g[t], dc_prev, dparams, **kw)


class InstanceNormLSTM(ConvLSTM):
    """The default cell: instance norms over the four gates and over the new state, inside the gate block.  On the bf16 datapath the
    whole cell forward is one launch where a tile holds whole images, and gate block + gate convolution are one host call each way."""
    fusable = True

    def __init__(self, gen, L, prefix, out_norm=False):
        super(InstanceNormLSTM, self).__init__(gen, L, prefix)
        f, zr, (h_, w_), r = self.f, L['zr'], L['hw'], self.scope
        # the gate convolution's own kernel (bf16 datapath, csrc/conv_gate.hip); where a tile holds whole images (planes of <= 256
        # pixels) also the interleaved pack: savp_convlstm_cell_fwd then runs the whole cell forward as one launch
        L['rconv'].enable_gate_pack(cell=bool(L['fused']) and h_ * w_ <= 256)
        L['n1'] = S.Norm(gen.store, r + 'input_transform_forget_output/', gen.T1, gen.N, 4 * f, gen.dev)
        L['n2'] = S.Norm(gen.store, r + 'state/', gen.T1, gen.N, f, gen.dev)
        # The data gradient of the gate convolution leaves the tiled-z channels of [x | z | h] out (their gradient is a per-sample
        # sum, taken once over all timesteps from region sums of the gate gradient: csrc/tiled_z.hip), which keeps its column count
        # on a tile boundary (72 / 136 / 264 -> 64 / 128 / 256; KTH's nz = 32: 96 / 160 / 288 -> 64 / 128 / 256).  bf16 datapath (the ring kernel owns the column gap).
        L['zless'] = bool(gen.train and zr and not gen.cw and L['fused'] and os.environ.get('SAVP_ZLESS_DGRAD', '1') == '1' and
                          K.tiled_z_ok(h_, w_, 4 * f, zr, L['rconv'].geom))
        if L['zless']:
            L['weff'] = torch.empty(25, 4 * f, K.tiled_z_pad(zr), device=gen.dev)

    def _ws(self):
        """Scratch of the coalesced ConvLSTM gate kernels (one buffer of the generator shared by all layers: the launches are serial)."""
        gen, (h, w) = self.gen, self.L['hw']
        need = K.lstm_ws_floats(gen.N, h * w, self.f)
        ws = getattr(gen, '_lstm_ws_buf', None)
        if ws is None or ws.numel() < need:
            ws = gen._lstm_ws_buf = torch.empty(max(need, K.lstm_ws_floats(gen.N, gen.H * gen.W // 4, 32)), device=self.L['gates'].v.device)
        return ws

    def forward(self, t, st):
        L, a = self.L, self.L['a']
        self._in_fwd(t, st)
        stats1 = s1 = None
        if L['fused']:
            stats1, s1 = K.lstm_stats_ws(self.gen.dev, self.gen.N, self.f)
        cp = L.get('cell_prof')                  # bench.py: HIP events around the whole cell (gate conv + gate passes)
        if cp is not None:
            ce0, ce1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ce0.record()
        hdst = self.h_dst(t)
        gk = L.get('gate_ktimer')                # bench.py: the gate-block launch's own begin / end stamps
        # the whole cell as ONE host call (savp_convlstm_cell_fwd) unless a measurement wants the two launches apart
        ca = (L['rconv'].forward(a.v[t], L['gates'].v[t], use_bias=False, stats=s1, defer=True)
              if (S.FUSED_ENTRIES and cp is None and gk is None and K.fused_ok()) else None)
        if ca is not None:
            ck = L.get('cell_ktimer')            # bench.py: the one-launch cell's own begin / end stamps (the kernel takes the armed pair)
            if ck is not None:
                ck.arm()
            K.convlstm_cell_fwd(ca, self._gates_fwd(t, hdst, eps=S.EPS_IN, ws=self._ws(), stats1=stats1, defer=True))
            if ck is not None:
                ck.taken()
        else:
            L['rconv'].forward(a.v[t], L['gates'].v[t], use_bias=False, stats=s1)
            if gk is not None:
                gk.arm()
            self._gates_fwd(t, hdst, eps=S.EPS_IN, ws=self._ws(), stats1=stats1)
            if gk is not None:
                gk.taken()
        if cp is not None:
            ce1.record()
            cp.append((ce0, ce1))

    def backward(self, t, dys):
        L, a, nrm = self.L, self.L['a'], self.L['norm']
        dys = self.dh(t, dys)
        skip = (self.f, L['zr']) if L['zless'] else None
        nb = self.gen._norm_bwd('nbstats', L, L['rconv'], L['gates'].g[t], a.g[t], nrm, L['pre'].v[t], skip)
        if nb is not None:
            nb['mean'], nb['rstd'] = nrm.mean[t], nrm.rstd[t]
        if S.FUSED_ENTRIES and K.fused_ok():       # gate block backward + the gate convolution's DGRAD: one host call
            K.convlstm_cell_bwd(L['rconv'].backward_data(L['gates'].g[t], a.g[t], beta=0, skip=skip, norm_bwd=nb, defer=True),
                                self._gates_bwd(t, dys, eps=S.EPS_IN, ws=self._ws(), dgates_raw=L.get('dg_raw'), defer=True))
        else:
            self._gates_bwd(t, dys, eps=S.EPS_IN, ws=self._ws(), dgates_raw=L.get('dg_raw'))
            L['rconv'].backward_data(L['gates'].g[t], a.g[t], beta=0, skip=skip, norm_bwd=nb)
        self._in_bwd(t, nb['ws'] if nb is not None else None)

    def z_gradient(self, drz):
        if not self.L['zless']:
            return super(InstanceNormLSTM, self).z_gradient(drz)
        # z gradient of the gate convolution from the gate gradients of all timesteps (the DGRADs left those channels out)
        L, gt, nz = self.L, self.L['gates'], self.gen.nz
        K.tiled_z_weff(L['rconv'].W, L['rconv'].geom, self.f, nz, L['weff'])
        K.tiled_z_grad(gt.flat(gt.g), L['weff'], drz.reshape(-1, nz), beta=1)


class BareLSTM(ConvLSTM):
    """The LSTM cell without a normaliser: conv + bias, the gate block without its norms."""
    bias = True

    def __init__(self, gen, L, prefix, out_norm=False):
        super(BareLSTM, self).__init__(gen, L, prefix, out_norm)
        self._make_out_norm(prefix + 'lstm_h%d/' % L['idx'])

    def forward(self, t, st):
        self._in_fwd(t, st)
        self.L['rconv'].forward(self.L['a'].v[t], self.L['gates'].v[t])                       # conv + bias
        self._gates_fwd(t, self.h_dst(t))
        self.out_norm_fwd(t)

    def backward(self, t, dys):
        self._gates_bwd(t, self.dh(t, dys))
        self.L['rconv'].backward_data(self.L['gates'].g[t], self.L['a'].g[t], beta=0)
        self._in_bwd(t)


class LayerNormLSTM(ConvLSTM):
    """conv_rnn_norm_layer = 'layer' inside the cell (separate_norms, rnn_ops.py:147-165): the gate convolution (no bias), a layer norm
    per gate (one G = 4 launch, parameters gathered per step), the pointwise state update, a layer norm of the new state, h'
    (csrc/ln_lstm.hip)."""

    def __init__(self, gen, L, prefix, out_norm=False):
        super(LayerNormLSTM, self).__init__(gen, L, prefix)
        f, r = self.f, self.scope
        # input / transform / forget / output: one G = 4 launch over the gate tensor
        L['gn4'] = S.ConcatNorm([S.Norm(gen.store, r + nm + '/', gen.T1, gen.N, f, gen.dev, groups=1)
                                 for nm in ('input', 'transform', 'forget', 'output')], gen.T1, gen.N, gen.dev)
        L['nS'] = S.Norm(gen.store, r + 'state/', gen.T1, gen.N, f, gen.dev, groups=1)
        L['gnv'] = self._act(4 * f)          # the normalised gates and their gradient
        L['cpre'] = self._act(f)             # the state before its norm
        L['dcn'] = self._step(f)

    def prep(self):
        self.L['gn4'].prep()

    def forward(self, t, st):
        L, g4, nS = self.L, self.L['gn4'], self.L['nS']
        self._in_fwd(t, st)
        L['rconv'].forward(L['a'].v[t], L['gates'].v[t], use_bias=False)
        K.groupnorm_act_fwd(L['gates'].v[t], g4.gamma, g4.beta, [L['gnv'].v[t]], g4.mean[t], g4.rstd[t], groups=4, act='none')
        K.lnlstm_state_fwd(L['gnv'].v[t], self.c_prev(t), L['cpre'].v[t])
        K.groupnorm_act_fwd(L['cpre'].v[t], nS.gamma, nS.beta, [L['c'].v[t]], nS.mean[t], nS.rstd[t], groups=1, act='none')
        K.lnlstm_out_fwd(L['gnv'].v[t], L['c'].v[t], self.h_dst(t))

    def backward(self, t, dys):
        L, g4, nS, gnv, cpre = self.L, self.L['gn4'], self.L['nS'], self.L['gnv'], self.L['cpre']
        dc_new, dc_prev = self.dc(t)
        K.lnlstm_out_bwd(gnv.v[t], L['c'].v[t], self.dh(t, dys), dc_new, L['dcn'], gnv.g[t])
        K.groupnorm_act_bwd(cpre.v[t], nS.gamma, nS.beta, nS.mean[t], nS.rstd[t], [L['dcn']], cpre.g[t], nS.dgamma, nS.dbeta,
                            groups=1, act='none')
        K.lnlstm_state_bwd(gnv.v[t], self.c_prev(t), cpre.g[t], gnv.g[t], dc_prev)
        K.groupnorm_act_bwd(L['gates'].v[t], g4.gamma, g4.beta, g4.mean[t], g4.rstd[t], [gnv.g[t]], L['gates'].g[t], g4.dgamma, g4.dbeta,
                            groups=4, act='none')
        L['rconv'].backward_data(L['gates'].g[t], L['a'].g[t], beta=0)
        self._in_bwd(t)

    def backward_weights(self):
        super(LayerNormLSTM, self).backward_weights()
        self.L['gn4'].finish()

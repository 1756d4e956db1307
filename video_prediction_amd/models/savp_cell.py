"""SAVPCell unrolled over time on the HIP kernels: forward and back-propagation through time.

Mirrors SAVPCell.call (/root/reference/video_prediction/models/savp_model.py:393-686) and its unroll
(generator_given_z_fn :689-696, tf_utils.unroll_rnn tf_utils.py:134-141) for the published SAVP family
(conv_pool2d / upsample_conv2d, instance norm, ConvLSTM, CDNA, tile_concat).

MI355X-first layout decisions:
  * every activation lives in a time-major buffer [T-1, N, H, W, C] that stays resident in HBM for the whole step
    (288 GB), so back-propagation never recomputes and every weight gradient is ONE split-K GEMM over all
    timesteps x samples instead of T-1 small ones;
  * concatenations (tile_concat with z, skip connections, [x, h_prev] of the ConvLSTM, [h_masks, transformed
    images]) are never materialised by copies: producers write straight into channel slices of the consumer's
    concat buffer, gradients are read back from the same slices;
  * the posterior and prior unrolls share weights, so they run as ONE unroll of batch 2B (all ops are per-sample).

What a recurrent ladder layer runs (ConvLSTM / ConvGRU with or without their norms, ablation_rnn's convolution) is one class per variant in
conv_rnn_cells.py; this module builds the chosen class per layer (L['cell']) and calls only its interface.
"""
import os

import torch

from .. import kernels as K
from .. import lib
from ..engine import ConcatConv, ConvLayer, same_pad_before, copy_view, prep_layers
from ..variables import ACTIVATIONS, NORM_SCOPES, down_scope, layer_specs, num_masks, up_scope

CONV_STATS = os.environ.get('SAVP_CONV_STATS', '1') == '1'      # developer A/B switch of the conv-epilogue statistics
FUSED_ENTRIES = os.environ.get('SAVP_FUSED_ENTRIES', '1') == '1'      # one host call per fused operator (csrc/fused_ops.hip); 0: the halves apart
NORM_BWD_STATS = os.environ.get('SAVP_NORM_BWD_STATS', '1') == '1'      # ... and of the norm-backward sums from the DGRAD that produces dy
EPS_IN = 1e-6   # fused_instance_norm epsilon (layers/normalization.py:37)


def ln_gru_opt_in(flag=None):
    """The opt-in of the layer-norm ConvGRU cell (conv_rnn='gru' with conv_rnn_norm_layer='layer', conv_rnn_cells.LayerNormGRU): the
    keyword where one was given, else SAVP_LN_GRU=1 in the environment, read when called.  Without it the combination stays refused."""
    return bool(flag) if flag is not None else os.environ.get('SAVP_LN_GRU', '0') == '1'


def norm_none_opt_in(flag=None):
    """The opt-in of norm_layer='none' (the generator and the encoders without a normaliser, NoNorm below): the keyword where one was
    given, else SAVP_NORM_NONE=1 in the environment, read when called.  Without it the value stays refused, as it was."""
    return bool(flag) if flag is not None else os.environ.get('SAVP_NORM_NONE', '0') == '1'


def check_norm_layers(hp, ln_gru=None, zw=None, norm_none=None):
    """The normaliser combinations of the HIP path; anything else raises with the combination named.  ln_gru: see ln_gru_opt_in;
    norm_none: see norm_none_opt_in.  zw: width of the slice [actions | state | z] the cell tiles or adds (default: the latent alone, hp.nz)."""
    zw = hp.nz if zw is None else zw
    if hp.conv_rnn not in ('lstm', 'gru'):
        raise NotImplementedError("conv_rnn=%r" % hp.conv_rnn)
    if hp.norm_layer not in ('instance', 'layer', 'none'):
        raise NotImplementedError("norm_layer=%r: the HIP path covers 'instance' and 'layer'" % hp.norm_layer)
    if hp.norm_layer == 'none' and not norm_none_opt_in(norm_none):
        raise NotImplementedError("norm_layer='none': the model without a normaliser is opt-in on the HIP path (SAVP_NORM_NONE=1, or the "
                                  "keyword norm_none=True of the model class / SAVPEngine)")
    if hp.conv_rnn_norm_layer not in ('instance', 'layer', 'none'):
        raise NotImplementedError("conv_rnn_norm_layer=%r: the HIP path covers 'instance', 'layer' and 'none'" % hp.conv_rnn_norm_layer)
    layer = 'layer' in (hp.norm_layer, hp.conv_rnn_norm_layer)
    if layer and not hp.use_tile_concat:
        # the untiled latent (dense(z) added to a convolution's output) is dropped because an instance norm removes a per-(sample,
        # channel) constant exactly; a layer norm removes only its mean over the channels, so the latent would matter
        raise NotImplementedError("use_tile_concat=False with norm_layer=%r, conv_rnn_norm_layer=%r: the untiled latent is only "
                                  "cancelled by an instance norm" % (hp.norm_layer, hp.conv_rnn_norm_layer))
    if hp.conv_rnn_norm_layer == 'layer' and not hp.ablation_rnn:
        # (under ablation_conv_rnn_norm the cell itself has no normaliser and the layer norm sits on the layer's output: covered)
        if hp.conv_rnn == 'gru' and not hp.ablation_conv_rnn_norm and not ln_gru_opt_in(ln_gru):
            raise NotImplementedError("conv_rnn='gru' with conv_rnn_norm_layer='layer': the GRU gate kernels are instance-norm only")
    # The untiled latent inside a cell WITHOUT a normaliser (conv_rnn_norm_layer='none' or ablation_conv_rnn_norm; both at once is the
    # selection's own TypeError, conv_rnn_cells.cell_class): no norm stands behind the cell's convolutions, so dense(z) (`weights`,
    # gates/weights, candidate/weights) is NOT cancelled there, and the cells do not compute it.
    bare = (hp.conv_rnn_norm_layer == 'none') != bool(hp.ablation_conv_rnn_norm)
    if bare and not hp.ablation_rnn and not hp.use_tile_concat and hp.where_add == 'all' and zw:
        if hp.conv_rnn == 'gru':
            raise NotImplementedError("conv_rnn='gru' without a cell normaliser (conv_rnn_norm_layer='none' or ablation_conv_rnn_norm) with "
                                      "use_tile_concat=False, where_add='all' and a latent: the untiled latent of the bare cell is not on "
                                      "the HIP path")
        if hp.norm_layer == 'none':
            # with norm_layer='instance' the bare ConvLSTM cell's missing term is the known gap of DESIGN.md section 7, left as it is;
            # a model without any normaliser must not widen it
            raise NotImplementedError("norm_layer='none' with conv_rnn='lstm' without a cell normaliser (conv_rnn_norm_layer='none' or "
                                      "ablation_conv_rnn_norm), use_tile_concat=False, where_add='all' and a latent: the untiled latent of "
                                      "the bare cell is not on the HIP path")


def gru_large_layers(height, width, ngf=32):
    """Indices into the encoder + decoder layer table of the conv-RNN layers whose plane exceeds the 1024 pixels the one-workgroup
    ConvGRU gate blocks (csrc/gru.hip) hold: with the instance-norm GRU cell those layers run on K.convgru_large_* (csrc/gru_two_pass.hip),
    the others on K.convgru_*.  A function of the frame size alone."""
    enc, dec = layer_specs(ngf, height, width)
    out, h, w = [], height, width
    for i, (_, use_rnn) in enumerate(enc + dec):
        h, w = (h // 2, w // 2) if i < len(enc) else (h * 2, w * 2)
        if use_rnn and h * w > K.GRU_SMALL_MAX_HW:
            out.append(i)
    return out


def last_frame_steps(t, L):
    """The steps whose (scheduled-sampling selected) input images are step t's last_images, oldest first: the reference starts from
    [images[0]] * L and appends each step's image (savp_model.py:281,349,406-407), so source j is step max(t - L + 1 + j, 0)."""
    return [max(t - L + 1 + j, 0) for j in range(L)]


def ceil4(n):
    return (n + 3) // 4 * 4


def ceil8(n):
    """Channel counts of convolution INPUT buffers are padded to multiples of 8 (zero channels, zero weight rows): the ring / thin kernels of
    the bf16 datapath take a reduction dimension in whole 8-channel chunks only -- with 4-channel padding KTH's first layer (2 + 32 -> 36
    channels) and its mask convolution (32 + 7 + 3 -> 44) fell to the general kernel, 35 us instead of 17 us per time step each."""
    return (n + 7) // 8 * 8


class Act(object):
    """Time-major activation buffer with an optional gradient twin."""

    def __init__(self, shape, device, grad=True, zero_grad=False, dtype=torch.float32, grad_dtype=torch.float32):
        self.v = torch.zeros(shape, device=device, dtype=dtype)            # the gradient twin is fp32 unless asked otherwise
        self.g = None
        if grad:
            self.g = torch.zeros(shape, device=device, dtype=grad_dtype) if zero_grad else \
                torch.empty(shape, device=device, dtype=grad_dtype)

    def flat(self, t):
        """[T, N, ...] -> [T*N, ...] view (time folded into the batch for the batched weight gradients)."""
        return t.reshape((t.shape[0] * t.shape[1],) + tuple(t.shape[2:]))


class Norm(object):
    """Parameters and saved statistics of one normalizer_fn.  groups None: fused_instance_norm (mean / rstd per (sample, channel));
    an integer: statistics shared by that many groups of consecutive channels (1 = tf.contrib.layers.layer_norm, mean / rstd
    per sample; csrc/group_norm.hip)."""

    def __init__(self, store, scope, T1, N, C, device, groups=None, bias=None):
        self.gamma, self.beta = store[scope + 'gamma'], store[scope + 'beta']
        # a layer norm does not cancel the bias of the convolution in front of it: with a bf16 output gradient (which the bf16 WGRAD
        # reads, and which takes no bias gradient) the norm's backward adds the column sums of its fp32 dx here (float64, exact)
        self.dbias = store.grad64(bias) if (groups is not None and bias is not None) else None
        # float64 accumulators (ParamGroup.grad64): every (sample, channel slab) workgroup of a norm-backward launch adds to them
        self.dgamma, self.dbeta = store.grad64(scope + 'gamma'), store.grad64(scope + 'beta')
        self.groups = groups
        self.mean = torch.empty(T1, N, C if groups is None else groups, device=device)
        self.rstd = torch.empty(T1, N, C if groups is None else groups, device=device)


class _PerStep(object):
    """What a NoNorm site hands out where a Norm hands out its saved statistics of step t (nrm.mean[t], nrm.rstd[t])."""

    def __init__(self, get):
        self.get = get

    def __getitem__(self, t):
        return self.get(t)


class NoNorm(object):
    """A normalizer_fn that is the identity (norm_layer = 'none', ops.py:1062-1074): no gamma / beta, no saved statistics; the site is
    act(x + add) on csrc/plain_act.hip.  `groups` is 0, not None: everything that assumes an instance norm behind a convolution (the fused
    conv + norm entries, the statistics and norm-backward epilogues) switches off as it does for a layer norm.

    The bias of the convolution in front is not cancelled by anything.  With an fp32 output gradient that convolution's weight-gradient
    pass takes the bias gradient as everywhere; with a bf16 one (which takes none) the backward kernel's float64 column sums of its fp32
    dx supply it: `psum`, folded into the bias variables by finish().

    add: the untiled latent (use_tile_concat=False): dense([actions | state | z]) of every step, [T1, N, C], set by untiled().  Its
    gradient is the per-(step, sample) rows of the same column sums."""
    groups = 0
    gamma = beta = dgamma = dbeta = None

    def __init__(self, store, T1, N, C, device, bias=None, train=True):
        self.T1, self.N, self.C, self.dev, self.train = T1, N, C, device, train
        self.dbias = [(store.grad64(bias), 0, C)] if (bias is not None and train) else []      # (float64 accumulator, first channel, count)
        self.psum = torch.zeros(N, C, device=device, dtype=torch.float64) if train else None      # all steps add to it
        self.bias_from_psum = False       # a bf16 dx has been written: decided by the first backward call
        self.add = self.dadd = self.dense = None
        # the two slots every caller passes on to norm_fwd / norm_bwd: (step t's add term, where step t's column sums go), and nothing
        self.mean = _PerStep(lambda t: (self.add[t] if self.add is not None else None, self.dadd[t] if self.dadd is not None else self.psum))
        self.rstd = _PerStep(lambda t: None)

    def untiled(self, dense, zfull):
        """The site adds dense(zfull) to its input: dense is the bias-free 1x1 ConvLayer of <scope>dense/kernel, zfull [T1, N, zw]."""
        self.dense, self.zfull = dense, zfull
        self.add = torch.zeros(self.T1, self.N, self.C, device=self.dev)
        if self.train:
            self.dadd = torch.zeros(self.T1, self.N, self.C, device=self.dev, dtype=torch.float64)      # per step: the gradient of add
            self.dadd32 = torch.empty(self.T1, self.N, self.C, device=self.dev)
            self.dzfull = torch.empty(self.T1, self.N, zfull.shape[-1], device=self.dev)

    def add_fwd(self, t):
        if self.dense is not None:
            self.dense.forward(self.zfull[t], self.add[t])          # the few-row dense kernel, once per step and site

    def finish(self):
        """After the last step's backward: the bias gradient where the column sums supply it, and with an untiled latent the gradients of
        dense/kernel (zfull^T . dadd) and of zfull (dadd . W^T, kept for z_gradient).  Clears the accumulators."""
        acc = self.dadd if self.dadd is not None else self.psum
        if self.bias_from_psum:
            tot = acc.sum(0) if acc.dim() == 2 else acc.sum((0, 1))
            for g64, c0, c in self.dbias:
                g64.add_(tot[c0:c0 + c])
        if self.dense is not None:
            R, zw = self.T1 * self.N, self.zfull.shape[-1]
            self.dadd32.copy_(self.dadd)
            d4 = self.dadd32.reshape(R, 1, 1, self.C)
            self.dense.backward_weights(self.zfull.reshape(R, 1, 1, zw), d4)
            self.dense.backward_data(d4, self.dzfull.reshape(R, 1, 1, zw), beta=0)
        if self.bias_from_psum or self.dense is not None:
            acc.zero_()

    def z_gradient(self, drz, cw):
        """Adds the latent's share of the untiled term's gradient to drz [T1, N, nz] (the cw conditioning columns in front of it are
        inputs: skipped)."""
        if self.dense is not None:
            drz.add_(self.dzfull[..., cw:])


def norm_fwd(nrm, x, outs, mean, rstd, act='relu', eps=EPS_IN, **kw):
    """normalizer_fn + activation of `nrm`'s kind (the instance norm's own epsilon is the caller's; a layer norm always takes 1e-12)."""
    if nrm.groups == 0:               # NoNorm: `mean` is (the step's add term, the step's column-sum accumulator)
        assert kw.pop('stats', None) is None and kw.pop('stats_shift', None) is None, 'no normaliser: nothing takes statistics'
        K.plain_act_fwd(x, mean[0], outs, act=act, **kw)
    elif nrm.groups is None:
        K.instnorm_act_fwd(x, nrm.gamma, nrm.beta, outs, mean, rstd, act=act, eps=eps, **kw)
    else:
        K.groupnorm_act_fwd(x, nrm.gamma, nrm.beta, outs, mean, rstd, groups=nrm.groups, act=act, eps=K.EPS_LN, **kw)


def norm_bwd(nrm, x, out0, mean, rstd, dys, dx, dgamma, dbeta, act='relu', eps=EPS_IN, stats=None, **kw):
    """Backward of norm_fwd (out0 is not read)."""
    if nrm.groups == 0:               # NoNorm: the column sums are wanted for a bf16 dx (the bias gradient) and for an add term (its gradient)
        assert stats is None, 'no normaliser: nothing takes backward sums'
        add, psum = mean
        if dx.dtype == torch.bfloat16:
            nrm.bias_from_psum = True
        K.plain_act_bwd(x, add, dys, dx, act=act, psum=psum if (dx.dtype == torch.bfloat16 or add is not None) else None, **kw)
    elif nrm.groups is None:
        K.instnorm_act_bwd(x, nrm.gamma, nrm.beta, out0, mean, rstd, dys, dx, dgamma, dbeta, act=act, eps=eps, stats=stats, **kw)
    else:
        assert stats is None, 'the layer norm takes its own backward sums'
        dsum = nrm.dbias if dx.dtype == torch.bfloat16 else None       # an fp32 dx: the convolution's WGRAD takes the bias gradient itself
        K.groupnorm_act_bwd(x, nrm.gamma, nrm.beta, mean, rstd, dys, dx, dgamma, dbeta, groups=nrm.groups, act=act, eps=K.EPS_LN,
                            dsum=dsum, **kw)


class ConcatNorm(object):
    """Instance norms of several heads that are normalised by ONE launch over their concatenated channels (instance norm is per
    channel, so concatenation changes nothing numerically): gamma / beta are gathered into one vector per step, their gradients
    are scattered back to the master variables after the backward pass."""

    def __init__(self, norms, T1, N, device):
        self.norms = norms
        self.sizes = [n.gamma.numel() for n in norms]
        C = sum(self.sizes)
        self.gamma, self.beta = torch.empty(C, device=device), torch.empty(C, device=device)
        self.dgamma, self.dbeta = torch.zeros(C, device=device, dtype=torch.float64), torch.zeros(C, device=device, dtype=torch.float64)
        # layer norms: one group per head (equal widths), so the heads keep their own statistics
        self.groups = None if norms[0].groups is None else len(norms)
        if self.groups is not None and len(set(self.sizes)) != 1:
            raise NotImplementedError('layer-normalised heads of different widths')
        self.mean = torch.empty(T1, N, C if self.groups is None else self.groups, device=device)
        self.rstd = torch.empty(T1, N, C if self.groups is None else self.groups, device=device)
        self.dbias = None
        if self.groups is not None and all(n.dbias is not None for n in norms):
            self.dbias = torch.zeros(C, device=device, dtype=torch.float64)

    def prep(self):
        off = 0
        for n, c in zip(self.norms, self.sizes):
            K.axpby(1.0, n.gamma, 0.0, None, self.gamma[off:off + c])
            K.axpby(1.0, n.beta, 0.0, None, self.beta[off:off + c])
            off += c

    def finish(self):
        off = 0
        for n, c in zip(self.norms, self.sizes):
            n.dgamma.add_(self.dgamma[off:off + c])          # float64 accumulators on both sides
            n.dbeta.add_(self.dbeta[off:off + c])
            if self.dbias is not None:
                n.dbias.add_(self.dbias[off:off + c])
            off += c
        self.dgamma.zero_()
        self.dbeta.zero_()
        if self.dbias is not None:
            self.dbias.zero_()


class ConcatNoNorm(NoNorm):
    """ConcatNorm's counterpart for heads without a normaliser: ONE activation launch over the concatenated channels; the column sums of
    a bf16 gradient go back to each head's own bias variable."""

    def __init__(self, norms, T1, N, device, train=True):
        super(ConcatNoNorm, self).__init__(None, T1, N, sum(n.C for n in norms), device, train=train)
        off = 0
        for n in norms:
            self.dbias += [(g64, off + c0, c) for g64, c0, c in n.dbias]
            off += n.C

    def prep(self):
        pass


def check_kernel_size(hp):
    """kernel_size of the CDNA / DNA transformations: sides of at least 1 and at most 49 taps (csrc/cdna_composite.hip keeps 49 per-tap
    accumulators).  Refused when the model is built -- by the engine before it sizes the kernel heads -- not by the first forward."""
    if hp.transformation not in ('cdna', 'dna'):
        return
    kh, kw = hp.kernel_size
    if kh < 1 or kw < 1:
        raise ValueError('kernel_size = %r: both sides must be at least 1' % (tuple(hp.kernel_size),))
    if kh * kw > 49:
        raise NotImplementedError('kernel_size = %r: the transformation kernels take at most 49 taps' % (tuple(hp.kernel_size),))


from . import conv_rnn_cells      # noqa: E402  (the cells build on Act, Norm and norm_fwd / norm_bwd above: the two modules import each other)


class SAVPGenerator(object):
    def __init__(self, store, hp, image_shape, N, train=True, prefix='generator/rnn/savp_cell/', cond=(0, 0), pix=0, ln_gru=None, norm_none=None):
        """cond = (n_actions, n_states): widths of inputs['actions'] / inputs['states'] (savp_model.py:411-444): [actions_t | state_t]
        joins the latent in every tile-concatenated slice, the next state is predicted by `state_pred/dense` (:655-658).
        pix = P: designated pixels of inputs['pix_distribs'] (:408-410,598-621,648-653); 0 = the model has no such input and nothing below
        allocates or launches anything for it."""
        H, W, C = image_shape
        self.hp, self.store, self.N, self.H, self.W, self.C = hp, store, N, H, W, C
        self._ones = None
        self.T1 = T1 = hp.sequence_length - 1
        self.train = train
        dev = store.device
        self.dev = dev
        self._cstats = {}                # head name -> the conv's epilogue supplies the instance norm's statistics (decided at first use)
        norm_none = norm_none_opt_in(norm_none)          # read once: every later check sees the same answer
        check_norm_layers(hp, ln_gru, norm_none=norm_none)
        # norm_layer = 'layer': every norm_layer site (the ladder's layers, ablation_rnn's conv_h<i>, the 3x3 heads) is a layer norm,
        # variables under <scope>/LayerNorm/ (csrc/group_norm.hip with one group; the heads' merged launch: one group per head)
        self.ln = hp.norm_layer == 'layer'
        # norm_layer = 'none': every one of those sites is the activation alone (NoNorm, csrc/plain_act.hip), no variables beside the
        # convolutions' biases; plain_sites: every such site, for finish() after the backward pass
        self.nn = hp.norm_layer == 'none'
        self.plain_sites = []
        # what a convolution in front of a norm_layer site tells its weight-gradient pass about a bf16 output gradient
        self.wkw = dict(bias_grad_elsewhere=True) if self.nn else dict(feeds_instance_norm=True)
        # downsample_layer / upsample_layer / activation_layer (ops.py:1052-1098; savp_model.py:395-397).  conv2d: the strided SAME
        # convolution, ConvLayer kind 'down'; deconv2d: conv2d_transpose, kind 'deconv'; the _v2 names are aliases (variables.DOWN_SCOPES).
        # elu: the activation code of every norm_layer site of the cell (the ladder, ablation_rnn's conv_h<i>, the 3x3 heads).
        self.down_op, self.up_op = down_scope(hp), up_scope(hp)
        if hp.activation_layer not in ACTIVATIONS:
            raise ValueError('Invalid activation layer %s' % hp.activation_layer)
        self.act = hp.activation_layer
        if hp.transformation not in ('cdna', 'flow', 'dna') or hp.last_frames < 1 or not hp.num_transformed_images:
            raise NotImplementedError('HIP path covers transformation in (cdna, flow, dna) with last_frames >= 1 and num_transformed_images >= 1')
        # the multi-source transformation kernels (csrc/cdna_composite.hip, csrc/warp_dna.hip) take up to lib.MAX_SOURCES source frames
        # of up to 8 CDNA kernels each; the compositing kernel up to 16 masks; the CDNA head's few-row dense kernel (savp_dense_fwd) up to
        # 256 output columns
        if hp.last_frames > lib.MAX_SOURCES:
            raise NotImplementedError('last_frames = %d: the transformation kernels take at most %d source frames'
                                      % (hp.last_frames, lib.MAX_SOURCES))
        if hp.transformation == 'cdna' and hp.num_transformed_images > 8:
            raise NotImplementedError('num_transformed_images = %d: at most 8 CDNA kernels per source frame' % hp.num_transformed_images)
        check_kernel_size(hp)
        ncol = hp.kernel_size[0] * hp.kernel_size[1] * hp.last_frames * hp.num_transformed_images
        if hp.transformation == 'cdna' and ncol > 256:
            raise NotImplementedError('CDNA head of %d columns (kernel taps x last_frames x num_transformed_images): the dense kernel takes '
                                      'at most 256' % ncol)
        if num_masks(hp) > 16:
            raise NotImplementedError('%d masks (last_frames = %d): the compositing kernel takes at most 16' % (num_masks(hp), hp.last_frames))
        # dilation_rate never reaches the transformations on SAVPCell: last_images is always a list, and the list branch of apply_kernels
        # recurses as apply_kernels(image, kernels) without it (savp_model.py:939-944), so apply_cdna_kernels / apply_dna_kernels run
        # with their default of (1, 1); nothing else in the cell reads it.  Any value computes what (1, 1) computes.
        if hp.nz and hp.use_rnn_z and hp.rnn not in ('lstm', 'gru') and not hp.ablation_rnn:
            raise NotImplementedError(hp.rnn)                                  # savp_model.py:360-361
        if hp.where_add not in ('input', 'all', 'middle'):
            raise ValueError('Invalid where_add %s' % hp.where_add)                      # savp_model.py:176-177
        # ablation_rnn (savp_model.py:272-291,426-429,466-474,502-509): no recurrent state anywhere -- every conv-RNN becomes conv2d 5x5
        # (+ tiled z) -> norm -> ReLU under scope conv_h<i>, the latent's cell becomes dense + tanh under scope fc_z
        self.abl_rnn = bool(hp.ablation_rnn)
        # (learn_initial_state under ablation_rnn: the reference's state_size then holds no conv_rnn_states / rnn_z_state entries, so no
        #  initial_state variables exist -- savp_model.py:269-307 -- and the flag does nothing; variables.py creates none either)
        self.nz = nz = hp.nz
        self.use_rnn_z = bool(nz and hp.use_rnn_z)
        self.tv = None                       # (weight, leading samples the loss covers, float64 [1] accumulator): set by the engine for tv_weight
        self.na, self.ns = na, ns = int(cond[0]), int(cond[1])
        self.cw = cw = na + ns                 # conditioning columns in front of the latent: state_action_z = [actions | state | z]
        self.zw = zw = cw + nz                 # width of every tiled slice
        if cw > 32:
            raise NotImplementedError('actions + states wider than 32 (csrc/state_pred.hip keeps them in registers)')
        # where the latent is tile-concatenated (savp_model.py:456-470,492-506): 'all' = the input of every down / upsample conv and of
        # every conv-RNN; 'input' = the first encoder conv only; 'middle' = the first decoder conv only
        # use_tile_concat=False (savp_model.py:458-460,470-471,495-496,506-507 -> _maybe_tile_concat_layer :983-993, rnn_ops.py:128-135,
        # 145-146): the latent enters as dense(z)[:, None, None, :] ADDED to the convolution's output instead of as tiled input channels.
        # Every such sum sits directly in front of an instance norm here (norm_layer / conv_rnn_norm_layer == 'instance' are required
        # above), and a per-(sample, channel) constant is removed exactly by the norm's mean subtraction: the outputs do not depend on
        # z, the `dense/kernel` / `weights` variables and z itself get zero gradients.  The layers therefore run without z channels and
        # those variables keep their (zero-initialised) gradients; pinned against the oracle, which computes the sums literally.
        # norm_layer = 'none' is the exception: nothing cancels the sum at a ladder layer's (and ablation_rnn's conv_h<i>) site, so there
        # dense([actions | state | z]) with <scope>dense/kernel is computed per step and added inside the site's activation kernel
        # (NoNorm.untiled); its gradients come from that kernel's column sums.  Inside a bare cell the term stays refused (check_norm_layers).
        tile = bool(hp.use_tile_concat)
        self.untiled = []                    # (NoNorm site, its dense layer): wired to [actions | state | z] once that buffer exists
        # which conv-RNN cell the recurrent layers run (the matrix of DESIGN.md section 1), and whether its output takes a norm of its own
        cell, out_norm = conv_rnn_cells.cell_class(hp, zw, ln_gru, norm_none)
        zr = zw if (hp.where_add == 'all' and tile) else 0              # tiled channels in a conv-RNN's input [x | actions state z | h]
        g = train
        # bf16 storage of tensors whose ONLY readers are convolutions of the bf16 datapath (round 4; the cell input [x | z | h] and the
        # gate gradient have been stored this way since round 3): the inputs of the down / upsample convolutions behind layer 0, the
        # last decoder layer's output (read by the 3x3 heads) and the gradient of every conv_pool / upsample / head convolution's output
        # (written by the instance norm's backward, read by that convolution's DGRAD / WGRAD).  Those kernels round their operands to
        # bf16 while staging anyway: identical numbers, half the bytes of the batched weight gradients' activation stream, and the
        # ring kernel stages a bf16 source by LDS-DMA.  SAVP_BF16_CONVIO=0 keeps fp32 tensors.
        self.act16 = bool(K.PRECISION['value'] == 1 and hp.conv_rnn == 'lstm' and os.environ.get('SAVP_BF16_CONVIO', '1') == '1')
        a16 = torch.bfloat16 if self.act16 else torch.float32
        enc_specs, dec_specs = layer_specs(hp.ngf, H, W)
        self.ne, self.nd = len(enc_specs), len(dec_specs)

        # ---- layers and their input buffers ----------------------------------------------------------------
        self.layers = []
        h_, w_ = H, W
        prev_f = None
        for i, (f, use_rnn) in enumerate(enc_specs + dec_specs):
            L = {'f': f, 'rnn': use_rnn, 'idx': i, 'dec': i >= self.ne}
            s = prefix + 'h%d/' % i
            j_dec = i - len(enc_specs)
            sel = hp.where_add == 'all' or (hp.where_add == 'input' and i == 0) or (hp.where_add == 'middle' and j_dec == 0)
            zc = zw if (tile and sel) else 0
            L['zc'], L['zr'] = zc, zr
            if i < self.ne:
                cx = 2 * C if i == 0 else prev_f
                k = 5 if i == 0 else 3
                L['in'] = Act((T1, N, h_, w_, ceil8(cx + zc)), dev, grad=g,      # pad channels stay zero
                              dtype=a16 if i > 0 else torch.float32)     # layer 0 holds the input image: fp32
                L['zoff_in'] = cx
                # 'down' (ops.conv2d, strides 2, SAME) runs in the folded pool kernel's (k+1)-tap geometry: engine.ConvLayer
                L['conv'] = ConvLayer(store, s + self.down_op + '/kernel', s + self.down_op + '/bias',
                                      'pool' if self.down_op == 'conv_pool2d' else 'down', (k, k), (2, 2),
                                      (same_pad_before(k + 1, 2, h_), same_pad_before(k + 1, 2, w_)),
                                      cx_pad=ceil8(cx + zc))
                h_, w_ = h_ // 2, w_ // 2
            else:
                j = i - self.ne
                skip = 0 if j == 0 else self.layers[self.ne - j - 1]['f']
                cx = prev_f + skip
                L['in'] = Act((T1, N, h_, w_, cx + zc), dev, grad=g, dtype=a16 if (cx + zc) % 8 == 0 else torch.float32)
                L['zoff_in'] = cx
                L['skip_off'] = prev_f
                h_, w_ = h_ * 2, w_ * 2
                if self.up_op == 'deconv2d':          # the data gradient of the 3x3 'down' convolution: its 4-tap geometry
                    L['conv'] = ConvLayer(store, s + 'deconv2d/kernel', s + 'deconv2d/bias', 'deconv', (3, 3), (2, 2),
                                          (same_pad_before(4, 2, h_), same_pad_before(4, 2, w_)))
                else:
                    L['conv'] = ConvLayer(store, s + 'upsample_conv2d/kernel', s + 'upsample_conv2d/bias', 'up', (3, 3), (2, 2),
                                          (same_pad_before(6, 2, h_), same_pad_before(6, 2, w_)))
            L['hw'] = (h_, w_)
            # (a decoder layer whose input keeps an odd channel count -- conditioning widths that are no multiple of 8 -- stays fp32 on both
            #  sides: the weight gradient of an upsample conv reads the input as its `dy` operand, and only whole 4-channel groups ride
            #  the bf16-operand kernel)
            pre16 = f % 8 == 0 and (i < self.ne or L['in'].v.dtype == torch.bfloat16 or not self.act16)
            L['pre'] = Act((T1, N, h_, w_, f), dev, grad=g, grad_dtype=a16 if pre16 else torch.float32)
            L['norm'] = self._norm(s, f, bias=L['conv'].bias_name)
            if self.nn and not tile and zw and sel:
                self._untiled(L['norm'], s)
            if use_rnn:
                L['cell'] = cell(self, L, prefix, out_norm)          # its buffers, ConvLayers and Norms go into L (conv_rnn_cells.py)
            else:
                L['out'] = None
            self.layers.append(L)
            prev_f = f
        nl = len(self.layers)
        last = self.layers[-1]
        ngf = hp.ngf
        self.M = M = num_masks(hp)
        self.L = hp.last_frames
        self.nk = nk = hp.last_frames * hp.num_transformed_images
        self.nti = hp.num_transformed_images
        kh, kw = hp.kernel_size
        self.kh, self.kw = kh, kw

        # ---- heads ------------------------------------------------------------------------------------------
        self.tf = hp.transformation
        self.h_last = Act((T1, N, H, W, last['f']), dev, grad=g, dtype=a16 if last['f'] % 8 == 0 else torch.float32)
        tf_convs = []
        if self.tf == 'cdna':
            sh_, sw_ = H // 2 ** self.ne, W // 2 ** self.ne
            small_f = self.layers[self.ne - 1]['f']
            self.hsmall = Act((T1, N, sh_, sw_, small_f), dev, grad=g)
            self.cdna_dense = ConvLayer(store, prefix + 'cdna_kernels/dense/kernel', prefix + 'cdna_kernels/dense/bias', 'conv',
                                        (1, 1), (1, 1), (0, 0))
            self.cdna_raw = Act((T1, N, kh * kw * nk), dev, grad=g)
            self.cdna_kern = Act((T1, N, kh * kw, nk), dev, grad=False)
            # gradient of the normalised CDNA kernels of ONE timestep, float64: the image tiles' partial sums meet in it through float64
            # atomics (exact, order-independent: include/savp_hip.h SavpCdnaArgs.dkern); consumed by cdna_kernels_bwd right away
            self.cdna_dkern = torch.zeros(N, kh * kw, nk, device=dev, dtype=torch.float64) if g else None
            tf_convs = [self.cdna_dense]
        else:
            # flow: h_flow = relu(IN(conv3x3)); flows = conv3x3 -> 2*nk   (savp_model.py:522-530)
            # dna : h_dna_kernel = relu(IN(conv3x3)); kernels = conv3x3 -> kh*kw*nk   (:534-544)
            hs, os_, cy = (('h%d_flow/' % nl, 'flows/', 2 * nk) if self.tf == 'flow' else
                           ('h%d_dna_kernel/' % nl, 'dna_kernels/', kh * kw * nk))
            s = prefix + hs
            self.tf_conv = ConvLayer(store, s + 'conv2d/kernel', s + 'conv2d/bias', 'conv', (3, 3), (1, 1), (1, 1))
            self.tf_pre = Act((T1, N, H, W, ngf), dev, grad=g)
            self.tf_norm = self._norm(s, ngf, bias=s + 'conv2d/bias')
            self.tf_h = Act((T1, N, H, W, ngf), dev, grad=g)
            self.tf_out = ConvLayer(store, prefix + os_ + 'conv2d/kernel', prefix + os_ + 'conv2d/bias', 'conv', (3, 3), (1, 1),
                                    (1, 1), cy_pad=ceil4(cy))
            self.tf_cy = ceil4(cy)
            self.tf_raw = Act((T1, N, H, W, self.tf_cy), dev, grad=g)
            if self.tf == 'dna':
                if self.tf_cy != cy:
                    raise NotImplementedError('dna with kh*kw*nk not a multiple of 4')
                self.dna_kern = torch.empty(T1, N, H, W, cy, device=dev)
            tf_convs = [self.tf_conv, self.tf_out]
        self.merge_heads = os.environ.get('SAVP_MERGE_HEADS', '1') == '1' and ngf % 4 == 0
        sep = not self.merge_heads          # separate pre-activation buffers only when every head has its own launch
        self.scratch = bool(hp.generate_scratch_image)          # savp_model.py:561-572; without it the head and its mask slot do not exist
        self.dep_mask = bool(hp.dependent_mask)                  # :631-632: the mask conv also reads the transformed images
        self.Cs = Cs = ceil4(C)                       # scratch conv writes a 4-aligned channel group into its maskin slot
        if self.scratch:
            s = prefix + 'h%d_scratch/' % nl
            self.scratch_conv = ConvLayer(store, s + 'conv2d/kernel', s + 'conv2d/bias', 'conv', (3, 3), (1, 1), (1, 1))
            self.scratch_pre = Act((T1, N, H, W, ngf), dev, grad=g) if sep else None
            self.scratch_norm = self._norm(s, ngf, bias=s + 'conv2d/bias')
            self.scratch_h = Act((T1, N, H, W, ngf), dev, grad=g)
            s = prefix + 'scratch_image/'
            self.scratch_out = ConvLayer(store, s + 'conv2d/kernel', s + 'conv2d/bias', 'conv', (3, 3), (1, 1), (1, 1), cy_pad=Cs)
            self.dscratch_pre = torch.empty(T1, N, H, W, Cs, device=dev) if g else None
        s = prefix + 'h%d_masks/' % nl
        self.masks_conv = ConvLayer(store, s + 'conv2d/kernel', s + 'conv2d/bias', 'conv', (3, 3), (1, 1), (1, 1))
        self.masks_pre = Act((T1, N, H, W, ngf), dev, grad=g) if sep else None
        self.masks_norm = self._norm(s, ngf, bias=s + 'conv2d/bias')
        # background images in the reference's order (savp_model.py:581-594): the step's input image, then frames of the INPUT video --
        # ('fixed', k) = images[k] at every step, ('last_context',) = images[min(t, context_frames - 1)]
        cf = hp.context_frames
        self.bgs = [('prev',)] if hp.prev_image_background else []
        if hp.context_images_background:
            self.bgs += [('fixed', k) for k in range(cf)]
        else:
            self.bgs += ([('fixed', 0)] if hp.first_image_background else []) + ([('fixed', cf - 1)] if hp.last_image_background else []) + \
                        ([('last_context',)] if hp.last_context_image_background else [])
        nb = len(self.bgs)
        assert M == nk + nb + int(self.scratch)
        if M < 2:
            raise NotImplementedError('a single transformed image (mask == 1 everywhere, savp_model.py:636-637)')
        # maskin = [h_masks (ngf) | nk transformed images | background images | scratch image]   (savp_model.py:632)
        self.Cmask = Cmask = ceil8(ngf + M * C + ((Cs - C) if self.scratch else 0))     # scratch slot is last: room for its padded write
        self.Ml = Ml = ceil4(M)                                    # padded logits row
        self.maskin = Act((T1, N, H, W, Cmask), dev, grad=g)
        self.o_cdna = ngf
        self.o_bg = [ngf + (nk + i) * C for i in range(nb)]
        self.o_prev = self.o_bg[self.bgs.index(('prev',))] if ('prev',) in self.bgs else None
        self.o_scratch = ngf + (nk + nb) * C
        s = prefix + 'masks/'
        self.mask_cin = Cmask if self.dep_mask else ngf            # channels of maskin the mask conv reads
        self.masks_out = ConvLayer(store, s + 'conv2d/kernel', s + 'conv2d/bias', 'conv', (3, 3), (1, 1), (1, 1),
                                   cx_pad=self.mask_cin, cy_pad=Ml)
        self.logits = Act((T1, N, H, W, Ml), dev, grad=g)
        self.masks = torch.empty(T1, N, H, W, M, device=dev)
        self.gen = Act((T1, N, H, W, C), dev, grad=g, zero_grad=True)
        # gradient of the transformations' source image: one step's (last_frames = 1) or, for last_frames > 1, one accumulator per step
        # (a generated frame is a source of up to last_frames later steps; BPTT adds their shares in a fixed order, see backward)
        self.dimg_cdna = torch.empty(N, H, W, C, device=dev) if (g and self.L == 1) else None
        self.dimg_acc = torch.empty(T1, N, H, W, C, device=dev) if (g and self.L > 1) else None

        # ---- actions / states (savp_model.py:411-422,655-658) -----------------------------------------------------
        # saz [T1, N, zw] = what every slice tiles: [actions_t | state_t | rnn_z_t]; the state recurrence (state_t = ground truth or the
        # previous step's prediction, gen_state_t = dense([actions_t | state_t])) involves no image, so one launch runs all steps
        # (csrc/state_pred.hip) before the unroll.  The tiled copy is under stop_gradient (:421-422): only the state loss reaches state_pred.
        self.saz = torch.zeros(T1, N, zw, device=dev) if cw else None
        if ns:
            s_ = prefix + 'state_pred/dense/'
            self.spW, self.spb = store[s_ + 'kernel'], store[s_ + 'bias']
            self.dspW, self.dspb = (store.grad64(s_ + 'kernel'), store.grad64(s_ + 'bias')) if g else (None, None)
            self.sa = torch.zeros(T1, N, cw, device=dev)
            self.gen_states = Act((T1, N, ns), dev, grad=g, zero_grad=True)
        # ---- z path -------------------------------------------------------------------------------------------
        if nz:
            self.zs = Act((T1, N, nz), dev, grad=g)
            self.rnn_z = Act((T1, N, nz), dev, grad=g, zero_grad=True)
            if self.use_rnn_z and self.abl_rnn:
                self.fc_z = ConvLayer(store, prefix + 'fc_z/dense/kernel', prefix + 'fc_z/dense/bias', 'conv', (1, 1), (1, 1), (0, 0))
                self.fcz_pre = Act((T1 * N, 1, 1, nz), dev, grad=g)
            elif self.use_rnn_z and hp.rnn == 'gru':            # tf.contrib.rnn.GRUCell under scope gru_z (savp_model.py:358-359,426)
                z = prefix + 'gru_z/gru_cell/'
                self.zg = ConvLayer(store, z + 'gates/kernel', z + 'gates/bias', 'conv', (1, 1), (1, 1), (0, 0))
                self.zc = ConvLayer(store, z + 'candidate/kernel', z + 'candidate/bias', 'conv', (1, 1), (1, 1), (0, 0))
                for c_ in (self.zg, self.zc):
                    c_.need_wt = c_.need_wd = False
                self.zA = torch.zeros(T1, N, 2 * nz, device=dev)
                self.zA2 = torch.zeros(T1, N, 2 * nz, device=dev)
                self.z_ru = torch.empty(T1, N, 2 * nz, device=dev)
                self.z_cand = torch.empty(T1, N, nz, device=dev)
                if g:
                    self.z_dGg = torch.empty(T1, N, 2 * nz, device=dev)
                    self.z_dGc = torch.empty(T1, N, nz, device=dev)
                    self.z_dA = torch.empty(T1, N, 2 * nz, device=dev)
            elif self.use_rnn_z:
                z = prefix + 'lstm_z/basic_lstm_cell/'
                self.zW, self.zb = store[z + 'kernel'], store[z + 'bias']
                self.dzW, self.dzb = store.grad64(z + 'kernel'), store.grad64(z + 'bias')      # float64 accumulators (one workgroup per sample adds to them)
                self.z_gates = torch.empty(T1, N, 4 * nz, device=dev)
                self.z_cs = torch.empty(T1, N, nz, device=dev)
        for nrm, dense in self.untiled:
            nrm.untiled(dense, self.saz if cw else self.rnn_z.v)
        # ---- learn_initial_state (savp_model.py:295-307,344-352): the conv-RNN states and the rnn_z state start from variables
        # `generator/initial_state_<i>/initial_state` (i = position in nest.flatten of {'conv_rnn_states': [...], 'rnn_z_state': ...}: layer
        # order, LSTM tuples as (c, h), the latent cell last), tiled over the batch; both unrolls (N = 2B) share them.  Forward: a broadcast
        # copy into step 0's state slots; backward: what step 0 hands back, summed over the batch.
        self.learn_init = bool(hp.learn_initial_state) and not self.abl_rnn
        if self.learn_init:
            k = 0

            def var(shape, acc64=False):
                nonlocal k
                name = 'generator/initial_state_%d/initial_state' % k
                k += 1
                assert tuple(store[name].shape) == tuple(shape), (name, tuple(store[name].shape), shape)
                return store[name], ((store.grad64(name) if acc64 else store.grad(name)) if g else None)
            for L in self.layers:
                if L['rnn']:
                    L['cell'].make_initial_state(var)
            if self.use_rnn_z and hp.rnn == 'gru':               # GRUCell: the state is h alone (savp_model.py:288-291)
                self.z_h0, self.z_dh0 = var((nz,), acc64=True)
            elif self.use_rnn_z:
                self.z_c0, self.z_dc0 = var((nz,), acc64=True)    # savp_lstm_z_bwd_init adds to them from every sample's workgroup
                self.z_h0, self.z_dh0 = var((nz,), acc64=True)
        # ---- merged 3x3 heads on the last decoder layer (SAVP_MERGE_HEADS=0: one launch per head, the reference's structure) ----
        # h6_scratch, h6_masks (and h6_flow / h6_dna_kernel) all read h_last through a 3x3 conv + instance norm + relu: ONE conv with
        # concatenated output channels, ONE instance norm over them, outputs routed by channel range; backward likewise.
        head_convs = ([self.scratch_conv] if self.scratch else []) + [self.masks_conv]
        if self.merge_heads:
            parts = ([(self.scratch_conv.kernel_name, self.scratch_conv.bias_name)] if self.scratch else []) + \
                    [(self.masks_conv.kernel_name, self.masks_conv.bias_name)]
            norms = ([self.scratch_norm] if self.scratch else []) + [self.masks_norm]
            if self.tf != 'cdna':
                parts.append((self.tf_conv.kernel_name, self.tf_conv.bias_name))
                norms.append(self.tf_norm)
                tf_convs = [self.tf_out]
            self.nheads = len(parts)
            self.heads_conv = ConcatConv(store, parts, (3, 3), (1, 1), (1, 1))
            if self.nn:
                for n in norms:                    # the merged launch stands for them (backward finishes it with heads_norm.finish())
                    self.plain_sites.remove(n)
                self.heads_norm = ConcatNoNorm(norms, T1, N, dev, train=g)
            else:
                self.heads_norm = ConcatNorm(norms, T1, N, dev)
            self.heads_pre = Act((T1, N, H, W, self.nheads * ngf), dev, grad=g,
                                 grad_dtype=a16 if (self.nheads * ngf) % 8 == 0 else torch.float32)
            head_convs = [self.heads_conv]
        # (the cells' convolutions kind by kind -- every layer's gate convolution, then every GRU candidate convolution: prep_layers packs
        #  the weights and finish_weight_grad folds the gradients in this order)
        cell_convs = [L['cell'].convs() for L in self.layers if L['rnn']]
        self.convs = [L['conv'] for L in self.layers] + [c for kind in zip(*cell_convs) for c in kind] + \
                     ([self.fc_z] if (self.use_rnn_z and self.abl_rnn) else []) + [d for _, d in self.untiled] + \
                     tf_convs + head_convs + ([self.scratch_out] if self.scratch else []) + [self.masks_out]
        # ---- pix_distribs: one launch after the unroll (pix_distribs_forward); the slots in the reference's order (:598-621) ----
        self.P = int(pix)
        if self.P:
            kinds = {'prev': lib.PIX_SLOT_CURRENT, 'fixed': lib.PIX_SLOT_FIXED, 'last_context': lib.PIX_SLOT_LAST_CONTEXT}
            self.pix_slots = [(lib.PIX_SLOT_TRANSFORMED, m) for m in range(nk)] + \
                             [(kinds[bg[0]], bg[1] if bg[0] == 'fixed' else 0) for bg in self.bgs] + \
                             ([(lib.PIX_SLOT_CURRENT, 0)] if self.scratch else [])          # :620-621: the scratch slot takes pix_distrib again
            assert len(self.pix_slots) == M
            self.gen_pix = torch.empty(T1, N, H, W, self.P, device=dev)
            self.tr_pix = None                   # [T1, N, H, W, P, M], allocated when first asked for
        # only FPROP packs needed at inference
        self._routes()

    # ---------------------------------------------------------------------------------------------------------
    def _routes(self):
        """Where the output of layer i (layers[i][-1] in the reference) is written: list of (Act, channel offset)."""
        ne, nd = self.ne, self.nd
        for i, L in enumerate(self.layers):
            r = []
            if i + 1 < len(self.layers):
                r.append((self.layers[i + 1]['in'], 0))
            else:
                r.append((self.h_last, 0))
            if i < ne:
                j = ne - 1 - i              # decoder layer that takes this encoder layer as skip (j > 0)
                if 1 <= j < nd:
                    r.append((self.layers[ne + j]['in'], self.layers[ne + j]['skip_off']))
                if i == ne - 1 and self.tf == 'cdna':
                    r.append((self.hsmall, 0))
            L['routes'] = r

    prefix_root = 'generator/rnn/'       # every variable of the generator cell lives under this scope (one gradient chunk)

    def weight_layers(self):
        return self.convs

    def prep_weights(self):
        prep_layers(self.convs)
        if self.merge_heads:
            self.heads_norm.prep()
        for L in self.layers:
            if L['rnn']:
                L['cell'].prep()

    # ---------------------------------------------------------------------------------------------------------
    def _out_views(self, L, t):
        f = L['f']
        return [buf.v[t][..., off:off + f] for buf, off in L['routes']]

    def _out_grads(self, L, t):
        f = L['f']
        return [buf.g[t][..., off:off + f] for buf, off in L['routes']]

    def forward(self, images, zs=None, gt_mask=None, collect_masks=False, actions=None, states=None):
        """images [T>=T1, N, H, W, C] device fp32 (frame t feeds step t); zs [T1, N, nz]; gt_mask int32 [T1, N]
        (1 = take the ground-truth frame: self.ground_truth of savp_model.py:333-334); actions [T1, N, na] / states [>=T1, N, ns] when
        the generator was built with cond.  Fills self.gen.v (and self.gen_states.v)."""
        T1, N, C = self.T1, self.N, self.C
        nz = self.nz
        self.images = images
        self.gt_mask = gt_mask
        cw, na = self.cw, self.na
        if cw:
            if (na and actions is None) or (self.ns and states is None):
                raise ValueError('this generator was built for inputs with actions / states (cond=%r)' % ((na, self.ns),))
            if self.ns:
                K.state_pred_fwd(actions[:T1].contiguous() if na else None, states[:T1].contiguous(), gt_mask, self.spW, self.spb, self.sa,
                                 self.gen_states.v)
                self.saz[..., :cw].copy_(self.sa)
            else:
                self.saz[..., :na].copy_(actions[:T1])
        if nz:
            self.zs.v.copy_(zs)
            if self.use_rnn_z and self.abl_rnn:           # tanh(dense(z)) (savp_model.py:426-429)
                self.fc_z.forward(self.zs.v.reshape(T1 * N, 1, 1, nz), self.fcz_pre.v)
                torch.tanh(self.fcz_pre.v.reshape(T1, N, nz), out=self.rnn_z.v)
            elif self.use_rnn_z and self.hp.rnn == 'gru':
                self.zA[..., :nz].copy_(self.zs.v)
                K.gru_seq_fwd(self.zA, self.zA2, self.zg.W, self.zg.bias, self.zc.W, self.zc.bias, self.rnn_z.v, self.z_ru, self.z_cand, nz,
                              h0=self.z_h0 if self.learn_init else None)
            elif self.use_rnn_z:
                K.lstm_z_fwd(self.zs.v, self.zW, self.zb, self.rnn_z.v, self.z_gates, self.z_cs,
                             init=(self.z_c0, self.z_h0) if self.learn_init else None)
            else:
                self.rnn_z.v.copy_(self.zs.v)
            if cw:
                self.saz[..., cw:].copy_(self.rnn_z.v)
        if self.zw:
            zw = self.zw
            zflat = (self.saz if cw else self.rnn_z.v).reshape(T1 * N, zw)
            for L in self.layers:
                b = L['in']
                if L['zc']:
                    K.tile_channels(zflat, b.flat(b.v)[..., L['zoff_in']:L['zoff_in'] + zw])
                if L['rnn'] and L['zr']:
                    a = L['a']
                    K.tile_channels(zflat, a.flat(a.v)[..., L['f']:L['f'] + zw])
        if self.learn_init:                # step 0's state slots <- the learned initial states, tiled over the batch
            for L in self.layers:
                if L['rnn']:
                    L['cell'].load_initial_state()
        in0, maskin = self.layers[0]['in'], self.maskin
        # the first frame feeds every step (savp_model.py:399-400): ONE launch writes it into all T1 steps' buffers -- time is the
        # kernel's sample index (source stride 0), the N*H*W pixels of a step its pixel index
        if self._ones is None:
            self._ones = torch.ones(max(N, T1), dtype=torch.int32, device=self.dev)
        NH = N * self.H
        mflat = maskin.v.reshape(T1, NH, self.W, -1)

        def frame_all_steps(k, t0=0):          # images[k] seen from steps t0 .. T1-1 (source stride 0 over time)
            return images[k].reshape(1, NH, self.W, C).expand(T1 - t0, NH, self.W, C)
        first_dsts = [in0.v.reshape(T1, NH, self.W, -1)[..., C:2 * C]]
        for bg, off in zip(self.bgs, self.o_bg):
            if bg == ('fixed', 0):
                first_dsts.append(mflat[..., off:off + C])
        K.select(self._ones, frame_all_steps(0), None, first_dsts)
        cf = self.hp.context_frames
        for bg, off in zip(self.bgs, self.o_bg):
            if bg[0] == 'fixed' and bg[1] != 0:
                K.select(self._ones, frame_all_steps(bg[1]), None, [mflat[..., off:off + C]])
            elif bg[0] == 'last_context':          # images[t] while t < context_frames, images[context_frames - 1] afterwards
                n = min(cf, T1)
                copy_view(images[:n].reshape(n, NH, self.W, C), [mflat[:n][..., off:off + C]])
                if T1 > n:
                    K.select(self._ones, frame_all_steps(cf - 1, n), None, [mflat[n:][..., off:off + C]])
        fuse_select = os.environ.get('SAVP_FUSE_SELECT', '1') == '1'

        def image_slots(t):         # where step t's input image goes: the first conv's input and the 'prev' background slot
            return [in0.v[t][..., 0:C]] + ([maskin.v[t][..., self.o_prev:self.o_prev + C]] if self.o_prev is not None else [])
        for t in range(T1):
            # image = tf.where(ground_truth[t], inputs['images'], states['gen_image'])     (savp_model.py:406); from step 1 on the
            # compositing kernel of step t-1 has already written it (composite_fwd(next_inputs=...))
            if t == 0 or not fuse_select:
                prev_gen = self.gen.v[t - 1] if t > 0 else None
                K.select(gt_mask[t], images[t], prev_gen, image_slots(t))
            for L in self.layers:
                f = L['f']
                # the conv's epilogue leaves the instance norm's statistics behind where it can (bf16 datapath, whole tiles): the
                # norm is then ONE launch (SAVP_CONV_STATS=0: the norm takes its own statistics)
                ck = ('cstats', K.PRECISION['value'])          # the answer depends on the datapath in use: decided once per precision
                if ck not in L:
                    L[ck] = (CONV_STATS and not self.nn and f <= 256 and (f & (f - 1)) == 0 and L['conv'].stats_ok(L['in'].v[t], L['pre'].v[t]))
                st = K.stats_ws(self.dev, N, f) if L[ck] else None
                if self.nn:
                    L['norm'].add_fwd(t)          # the untiled latent's dense(z) of this step, where the site takes one
                if L['rnn']:
                    L['cell'].forward(t, st)
                else:
                    self._conv_in_act(L['conv'], L['in'].v[t], L['pre'].v[t], st, L['norm'], self._out_views(L, t), t)
            tslot = maskin.v[t][..., self.o_cdna:self.o_cdna + self.nk * C]
            ngf = self.hp.ngf
            if self.merge_heads:
                # one conv + one instance norm for every 3x3 head on h_last; outputs routed by channel range
                hn = self.heads_norm
                outs = ([self.scratch_h.v[t]] if self.scratch else []) + [maskin.v[t][..., 0:ngf]] + \
                       ([self.tf_h.v[t]] if self.tf != 'cdna' else [])
                self._conv_norm('heads', self.heads_conv, self.h_last.v[t], self.heads_pre.v[t], hn, outs, t,
                                out_ranges=[(i * ngf, ngf) for i in range(self.nheads)])
            # last_frames > 1: the kernels / flows are split into L groups, group j applied to source j (apply_kernels / apply_flows,
            # savp_model.py:926-965); the step's input buffers keep every selected image, so the sources are read where they are
            srcs = [in0.v[s][..., 0:C] for s in last_frame_steps(t, self.L)] if self.L > 1 else None
            if self.tf == 'cdna':
                # CDNA kernels from the smallest layer (savp_model.py:546-559) and their application (:580, :893-923)
                self.cdna_dense.forward(self.hsmall.v[t].reshape(N, -1), self.cdna_raw.v[t])
                K.cdna_kernels_fwd(self.cdna_raw.v[t], self.cdna_kern.v[t], self.kh, self.kw, self.nk)
                if srcs is None:
                    K.cdna_apply_fwd(in0.v[t][..., 0:C], self.cdna_kern.v[t], tslot, self.kh, self.kw, self.nk)
                else:
                    K.cdna_apply_multi_fwd(srcs, self.cdna_kern.v[t], tslot, self.kh, self.kw, self.nti)
            else:
                if not self.merge_heads:
                    self._conv_norm('tf', self.tf_conv, self.h_last.v[t], self.tf_pre.v[t], self.tf_norm, [self.tf_h.v[t]], t)
                self.tf_out.forward(self.tf_h.v[t], self.tf_raw.v[t])
                if self.tf == 'flow' and srcs is None:
                    K.image_warp_fwd(in0.v[t][..., 0:C], self.tf_raw.v[t], tslot, self.nk)            # apply_flows :955-965
                elif self.tf == 'flow':
                    K.image_warp_multi_fwd(srcs, self.tf_raw.v[t], tslot, self.nti)
                elif srcs is None:
                    K.dna_apply_fwd(in0.v[t][..., 0:C], self.tf_raw.v[t], self.dna_kern[t], tslot, self.kh, self.kw, self.nk)
                else:
                    K.dna_apply_multi_fwd(srcs, self.tf_raw.v[t], self.dna_kern[t], tslot, self.kh, self.kw, self.nti)
            # scratch image (savp_model.py:561-572): sigmoid fused into the conv epilogue, written into its mask-conv slot
            if self.scratch and not self.merge_heads:
                self._conv_norm('scratch', self.scratch_conv, self.h_last.v[t], self.scratch_pre.v[t], self.scratch_norm,
                                [self.scratch_h.v[t]], t)
            if self.scratch:
                self.scratch_out.forward(self.scratch_h.v[t], maskin.v[t][..., self.o_scratch:self.o_scratch + self.Cs],
                                         act=lib.ACT_SIGMOID)
            # masks (savp_model.py:623-646)
            if not self.merge_heads:
                self._conv_norm('masks', self.masks_conv, self.h_last.v[t], self.masks_pre.v[t], self.masks_norm,
                                [maskin.v[t][..., 0:self.hp.ngf]], t)
            self.masks_out.forward(maskin.v[t][..., 0:self.mask_cin], self.logits.v[t])
            nxt = (gt_mask[t + 1], images[t + 1], image_slots(t + 1)) if (fuse_select and t + 1 < T1) else None
            K.composite_fwd(self.logits.v[t], maskin.v[t][..., self.hp.ngf:self.hp.ngf + self.M * C], self.gen.v[t],
                            self.masks[t] if collect_masks else None, M=self.M, next_inputs=nxt)
        return self.gen.v

    def pix_distribs_forward(self, pix_in, transformed=False):
        """gen_pix_distribs (and transformed_pix_distribs) of the unroll forward() has just run: pix_in [>= T1, N, H, W, P] time-major, the
        scheduled-sampling mask, kernels / flows and mask logits are the unroll's own.  One launch (csrc/pix_distribs.hip), never part of a
        train step or a captured sequence.  Returns gen_pix [T1, N, H, W, P] (a buffer of the generator)."""
        if not self.P:
            raise RuntimeError('this generator was built without pix_distribs (pix=0)')
        if transformed and self.tr_pix is None:
            self.tr_pix = torch.empty(self.T1, self.N, self.H, self.W, self.P, self.M, device=self.dev)
        tfp = self.cdna_kern.v if self.tf == 'cdna' else (self.dna_kern if self.tf == 'dna' else self.tf_raw.v)
        K.pix_distribs_fwd(pix_in, self.gt_mask, self.tf, tfp, self.logits.v, self.gen_pix, self.pix_slots, self.L, self.nti,
                           self.hp.context_frames, self.kh, self.kw, transformed=self.tr_pix if transformed else None)
        return self.gen_pix

    def _norm(self, scope, c, kind=None, bias=None):
        """The normalizer_fn of `kind` (default: norm_layer) under `scope`: <scope>InstanceNorm/ or <scope>LayerNorm/; bias: the variable
        name of the bias of the convolution in front of it (a layer norm's backward can supply that bias's gradient, and so can the
        site of kind 'none', which has no variables of its own)."""
        kind = kind or self.hp.norm_layer
        if kind == 'none':                # the identity: a parameter-less site (NoNorm)
            site = NoNorm(self.store, self.T1, self.N, c, self.dev, bias=bias, train=self.train)
            self.plain_sites.append(site)
            return site
        return Norm(self.store, scope + NORM_SCOPES[kind], self.T1, self.N, c, self.dev, groups=1 if kind == 'layer' else None, bias=bias)

    def _untiled(self, nrm, scope):
        """The NoNorm site `nrm` takes the untiled latent: dense([actions | state | z]) with <scope>dense/kernel (no bias,
        savp_model.py:983-993) added to its input.  The layer is a 1x1 ConvLayer among self.convs; __init__ wires it to the buffer."""
        self.untiled.append((nrm, ConvLayer(self.store, scope + 'dense/kernel', None, 'conv', (1, 1), (1, 1), (0, 0))))

    # ---------------------------------------------------------------------------------------------------------
    def _conv_norm(self, name, conv, x, pre, nrm, outs, t, **kw):
        """conv -> instance norm + ReLU of a head; the conv's epilogue supplies the norm's statistics where it can (see forward)."""
        ok = self._cstats.get((name, K.PRECISION['value']))
        if ok is None:
            c = pre.shape[-1]
            ok = self._cstats[(name, K.PRECISION['value'])] = bool(CONV_STATS and nrm.groups != 0 and c <= 256 and (c & (c - 1)) == 0 and
                                                                   conv.stats_ok(x, pre))          # (groups 0: no norm, no statistics)
        st = K.stats_ws(self.dev, self.N, pre.shape[-1]) if ok else None
        self._conv_in_act(conv, x, pre, st, nrm, outs, t, **kw)

    def _conv_in_act(self, conv, x, pre, st, nrm, outs, t, **kw):
        """conv -> fused_instance_norm + ReLU as ONE host call (savp_conv_in_act_fwd) where nothing instruments the conv; st = the
        statistics slice the conv's epilogue fills for the norm (None: the norm takes its own)."""
        bias = getattr(conv, 'inner', conv).bias          # ConcatConv keeps the concatenated bias in its inner layer
        nkw = dict(act=self.act, eps=EPS_IN, stats=st, stats_shift=bias if st is not None else None, **kw)
        ca = conv.forward(x, pre, stats=st, defer=True) if (FUSED_ENTRIES and K.fused_ok() and nrm.groups is None) else None
        if ca is not None:
            K.conv_in_act_fwd(ca, K.instnorm_act_fwd(pre, nrm.gamma, nrm.beta, outs, nrm.mean[t], nrm.rstd[t], defer=True, **nkw))
        else:
            conv.forward(x, pre, stats=st)
            norm_fwd(nrm, pre, outs, nrm.mean[t], nrm.rstd[t], **nkw)

    def _norm_bwd(self, key, holder, conv, dy, dx, nrm, x, skip=None):
        """The instance norm (over x, parameters nrm) whose OUTPUT gradient is the channels [0, C) that conv.backward_data(dy, dx) is
        about to write: where the ring kernel can, its epilogue leaves that norm's backward sums behind (SavpConvArgs.nb_*), and the
        norm's backward is then ONE launch.  Returns the norm_bwd dict for backward_data (None: the norm takes its own sums); its 'ws'
        is what instnorm_act_bwd(stats=...) gets.  The decision is made once per layer (holder[key])."""
        if nrm.groups is not None:            # the epilogue's sums take per-(sample, channel) statistics: the layer norm takes its own
            return None
        if self.act == 'elu':                 # the epilogue knows the 0 / 1 / alpha masks only (SavpConvArgs.nb_act): an ELU norm takes its own
            return None
        t_ = dict(x=x, mean=nrm.mean[0], rstd=nrm.rstd[0], gamma=nrm.gamma, beta=nrm.beta, c0=0, act=self.act)
        key = (key, K.PRECISION['value'])
        ok = holder.get(key)
        if ok is None:
            # savp_instnorm_act_bwd(stats_ready) runs the coalesced apply pass alone: C % 4 == 0, C <= 256 and a whole number of pixel rows
            # per 256-thread workgroup (256 % (C / 4) == 0) -- the forward twin's guard (non-power-of-two ngf would otherwise raise in every backward)
            c = x.shape[-1]
            ok = holder[key] = bool(NORM_BWD_STATS and dx.dtype == torch.float32 and c <= 256 and c % 4 == 0 and 256 % (c // 4) == 0 and
                                    conv.norm_bwd_ok(dy, dx, t_, skip))
        if not ok:
            return None
        t_['ws'] = K.stats_ws(self.dev, self.N, x.shape[-1])
        return t_

    def _in_act_conv_bwd(self, L, t, y0, dys, st):
        """Backward of a ladder layer's instance norm + ReLU and of its conv_pool / upsample convolution's data path: one host call
        (savp_conv_in_act_bwd).  st: the norm-backward sums a data gradient's epilogue has already left (None: the norm takes them)."""
        nrm = L['norm']
        nargs = (L['pre'].v[t], nrm.gamma, nrm.beta, y0, nrm.mean[t], nrm.rstd[t], dys, L['pre'].g[t], nrm.dgamma, nrm.dbeta)
        if FUSED_ENTRIES and K.fused_ok() and nrm.groups is None:
            K.conv_in_act_bwd(L['conv'].backward_data(L['pre'].g[t], L['in'].g[t], beta=0, defer=True),
                              K.instnorm_act_bwd(*nargs, act=self.act, eps=EPS_IN, stats=st, defer=True))
        else:
            norm_bwd(nrm, *nargs[:1], *nargs[3:], act=self.act, eps=EPS_IN, stats=st)
            L['conv'].backward_data(L['pre'].g[t], L['in'].g[t], beta=0)

    def backward(self, state_grad=False):
        """BPTT.  Expects self.gen.g (zero-initialised each step by the caller) to hold dL/dgen_images (and, with state_grad,
        self.gen_states.g to hold dL/dgen_states).
        Accumulates every generator-cell weight gradient into the store and returns dL/dzs [T1, N, nz] (or None)."""
        T1, N, C, nz = self.T1, self.N, self.C, self.nz
        ngf = self.hp.ngf
        in0, maskin = self.layers[0]['in'], self.maskin
        for t in range(T1 - 1, -1, -1):
            # composite + masks head
            K.composite_bwd(self.logits.v[t], maskin.v[t][..., ngf:ngf + self.M * C], self.gen.g[t], self.logits.g[t], maskin.g[t],
                            ngf, M=self.M)
            self.masks_out.backward_data(self.logits.g[t], maskin.g[t][..., 0:self.mask_cin], beta=1)
            if self.scratch:       # scratch head: d(sigmoid) then the scratch_image conv's data gradient
                K.sigmoid_bwd(maskin.g[t][..., self.o_scratch:self.o_scratch + self.Cs],
                              maskin.v[t][..., self.o_scratch:self.o_scratch + self.Cs], self.dscratch_pre[t])
                self.scratch_out.backward_data(self.dscratch_pre[t], self.scratch_h.g[t], beta=0)
            # pixel transformation head (everything behind its 3x3 feature conv)
            dslot = maskin.g[t][..., self.o_cdna:self.o_cdna + self.nk * C]
            if self.L > 1:
                # source j is step tau = t - L + 1 + j; its gradient goes to that step's accumulator, read by step tau's select_bwd
                # below once t has come down to tau.  Step tau's first share (from the latest step that reads it, where j == 0 or
                # t == T1 - 1) overwrites, the later ones add.  tau <= 0 is dropped: step 0's image is a context frame.
                steps = last_frame_steps(t, self.L)
                srcs = [in0.v[s][..., 0:C] for s in steps]
                taus = [t - self.L + 1 + j for j in range(self.L)]
                dsrcs = [self.dimg_acc[tau] if tau > 0 else None for tau in taus]
                betas = [0 if (j == 0 or t == T1 - 1) else 1 for j in range(self.L)]
            if self.tf == 'cdna':
                if self.L > 1:
                    K.cdna_apply_multi_bwd(srcs, self.cdna_kern.v[t], dslot, dsrcs, self.cdna_dkern, self.kh, self.kw, self.nti, betas)
                else:
                    K.cdna_apply_bwd(in0.v[t][..., 0:C], self.cdna_kern.v[t], dslot, self.dimg_cdna, self.cdna_dkern, self.kh,
                                     self.kw, self.nk)
                K.cdna_kernels_bwd(self.cdna_raw.v[t], self.cdna_dkern, self.cdna_raw.g[t], self.kh, self.kw, self.nk)
                self.cdna_dense.backward_data(self.cdna_raw.g[t], self.hsmall.g[t].reshape(N, -1), beta=0)
            else:
                if self.tf == 'flow':
                    if self.L > 1:
                        K.image_warp_multi_bwd(srcs, self.tf_raw.v[t], dslot, self.tf_raw.g[t], dsrcs, self.nti, betas)
                    else:
                        K.image_warp_bwd(in0.v[t][..., 0:C], self.tf_raw.v[t], dslot, self.tf_raw.g[t], self.dimg_cdna, self.nk)
                    if self.tv is not None:          # total-variation loss of the flows (base_model.py:763-769): this step's share + gradient
                        w_tv, rows, acc = self.tv
                        s1 = 1.0 / (T1 * rows * (self.H - 1) * self.W)
                        s2 = 1.0 / (T1 * rows * self.H * (self.W - 1))
                        K.tv_loss(self.tf_raw.v[t][:rows], 2 * self.nk, s1, s2, w_tv, acc, self.tf_raw.g[t][:rows])
                elif self.L > 1:
                    K.dna_apply_multi_bwd(srcs, self.tf_raw.v[t], self.dna_kern[t], dslot, self.tf_raw.g[t], dsrcs, self.kh, self.kw,
                                          self.nti, betas)
                else:
                    K.dna_apply_bwd(in0.v[t][..., 0:C], self.tf_raw.v[t], self.dna_kern[t], dslot, self.tf_raw.g[t],
                                    self.dimg_cdna, self.kh, self.kw, self.nk)
                self.tf_out.backward_data(self.tf_raw.g[t], self.tf_h.g[t], beta=0)
            # the 3x3 feature convs on h_last: instance norm + conv data gradients into h_last.g
            if self.merge_heads:
                hn = self.heads_norm
                dys = ([self.scratch_h.g[t]] if self.scratch else []) + [maskin.g[t][..., 0:ngf]] + \
                      ([self.tf_h.g[t]] if self.tf != 'cdna' else [])
                norm_bwd(hn, self.heads_pre.v[t], None, hn.mean[t], hn.rstd[t], dys, self.heads_pre.g[t],
                                   hn.dgamma, hn.dbeta, act=self.act, eps=EPS_IN, dy_ranges=[(i * ngf, ngf) for i in range(self.nheads)])
                Ll = self.layers[-1]
                nb_last = None
                if not Ll['rnn']:          # h_last is the output of the last layer's instance norm: its backward sums leave with this DGRAD
                    nl_ = Ll['norm']
                    nb_last = self._norm_bwd('nb_heads', self._cstats, self.heads_conv, self.heads_pre.g[t], self.h_last.g[t], nl_,
                                             Ll['pre'].v[t])
                    if nb_last is not None:
                        nb_last['mean'], nb_last['rstd'] = nl_.mean[t], nl_.rstd[t]
                self.heads_conv.backward_data(self.heads_pre.g[t], self.h_last.g[t], beta=0, norm_bwd=nb_last)
            else:
                mn = self.masks_norm
                norm_bwd(mn, self.masks_pre.v[t], maskin.v[t][..., 0:ngf], mn.mean[t], mn.rstd[t],
                                   [maskin.g[t][..., 0:ngf]], self.masks_pre.g[t], mn.dgamma, mn.dbeta, act=self.act, eps=EPS_IN)
                self.masks_conv.backward_data(self.masks_pre.g[t], self.h_last.g[t], beta=0)
                if self.scratch:
                    sn = self.scratch_norm
                    norm_bwd(sn, self.scratch_pre.v[t], self.scratch_h.v[t], sn.mean[t], sn.rstd[t],
                                       [self.scratch_h.g[t]], self.scratch_pre.g[t], sn.dgamma, sn.dbeta, act=self.act, eps=EPS_IN)
                    self.scratch_conv.backward_data(self.scratch_pre.g[t], self.h_last.g[t], beta=1)
                if self.tf != 'cdna':
                    tn = self.tf_norm
                    norm_bwd(tn, self.tf_pre.v[t], self.tf_h.v[t], tn.mean[t], tn.rstd[t], [self.tf_h.g[t]],
                                       self.tf_pre.g[t], tn.dgamma, tn.dbeta, act=self.act, eps=EPS_IN)
                    self.tf_conv.backward_data(self.tf_pre.g[t], self.h_last.g[t], beta=1)
            if not self.merge_heads:
                nb_last = None
            # decoder / encoder ladder in reverse
            for L in reversed(self.layers):
                dys = self._out_grads(L, t)
                if L['rnn']:
                    L['cell'].backward(t, dys)
                else:
                    y0 = self._out_views(L, t)[0]
                    st_ = nb_last['ws'] if (L is self.layers[-1] and nb_last is not None and len(dys) == 1) else None
                    self._in_act_conv_bwd(L, t, y0, dys, st_)
            # d image -> previous step's generated frame where it was fed back (not ground truth)
            if t > 0:
                K.select_bwd(self.gt_mask[t], [in0.g[t][..., 0:C], self.dimg_cdna if self.L == 1 else self.dimg_acc[t]] +
                             ([maskin.g[t][..., self.o_prev:self.o_prev + C]] if self.o_prev is not None else []), self.gen.g[t - 1])
        if self.learn_init:                # gradients of the learned initial states: step 0's state gradients summed over the batch
            for L in self.layers:
                if L['rnn']:
                    L['cell'].initial_state_grad()
        # ---- weight gradients: one split-K GEMM per layer over all (t, n) ----------------------------------------
        for L in self.layers:
            b, pre = L['in'], L['pre']
            L['conv'].backward_weights(b.flat(b.v), pre.flat(pre.g), **self.wkw)
            if L['rnn']:
                L['cell'].backward_weights()
        hl = self.h_last
        if self.tf == 'cdna':
            hs = self.hsmall
            self.cdna_dense.backward_weights(hs.v.reshape(T1 * N, -1), self.cdna_raw.g.reshape(T1 * N, -1))
        else:
            if not self.merge_heads:
                self.tf_conv.backward_weights(hl.flat(hl.v), hl.flat(self.tf_pre.g), **self.wkw)
            self.tf_out.backward_weights(hl.flat(self.tf_h.v), hl.flat(self.tf_raw.g))
        if self.merge_heads:
            self.heads_conv.backward_weights(hl.flat(hl.v), hl.flat(self.heads_pre.g), **self.wkw)
            self.heads_norm.finish()
        else:
            if self.scratch:
                self.scratch_conv.backward_weights(hl.flat(hl.v), hl.flat(self.scratch_pre.g), **self.wkw)
            self.masks_conv.backward_weights(hl.flat(hl.v), hl.flat(self.masks_pre.g), **self.wkw)
        if self.scratch:
            self.scratch_out.backward_weights(hl.flat(self.scratch_h.v), self.dscratch_pre.reshape(T1 * N, self.H, self.W, self.Cs))
        self.masks_out.backward_weights(hl.flat(maskin.v)[..., 0:self.mask_cin], hl.flat(self.logits.g))
        for site in self.plain_sites:      # norm_layer = 'none': bias gradients from the column sums, the untiled latent's dense layers
            site.finish()
        for c in self.convs:
            c.finish_weight_grad()
        # ---- state prediction: the state loss's gradient (the caller left it in gen_states.g) through the recurrence ----------
        if self.ns and state_grad:
            K.state_pred_bwd(self.gt_mask, self.spW, self.sa, self.gen_states.g, self.dspW, self.dspb)
        # ---- z path ----------------------------------------------------------------------------------------------
        if not nz:
            return None
        drz = self.rnn_z.g
        drz.zero_()
        cw = self.cw                     # the conditioning columns of each tiled slice are inputs / under stop_gradient: skipped
        for L in self.layers:
            b = L['in']
            if L['zc']:
                K.colsum(b.flat(b.g)[..., L['zoff_in'] + cw:L['zoff_in'] + cw + nz], drz, per_row=True)
            if L['rnn'] and L['zr']:
                L['cell'].z_gradient(drz)
        for nrm, _ in self.untiled:
            nrm.z_gradient(drz, cw)
        if self.use_rnn_z and self.abl_rnn:             # tanh(dense(z)) backward: d pre = d rnn_z * (1 - rnn_z^2)
            dpre = self.fcz_pre.g.reshape(T1, N, nz)
            torch.mul(self.rnn_z.v, self.rnn_z.v, out=dpre)
            dpre.neg_().add_(1.0).mul_(drz)
            zs4 = self.zs.v.reshape(T1 * N, 1, 1, nz)
            self.fc_z.backward_data(self.fcz_pre.g, self.zs.g.reshape(T1 * N, 1, 1, nz), beta=0)
            self.fc_z.backward_weights(zs4, self.fcz_pre.g)
            self.fc_z.finish_weight_grad()
            return self.zs.g
        if self.use_rnn_z and self.hp.rnn == 'gru':
            R = T1 * N
            K.gru_seq_bwd(self.zA, self.zg.W, self.zc.W, self.z_ru, self.z_cand, drz, self.z_dGg, self.z_dGc, self.z_dA, nz,
                          dh0=self.z_dh0 if self.learn_init else None)
            self.zg.backward_weights(self.zA.reshape(R, 1, 1, 2 * nz), self.z_dGg.reshape(R, 1, 1, 2 * nz))
            self.zc.backward_weights(self.zA2.reshape(R, 1, 1, 2 * nz), self.z_dGc.reshape(R, 1, 1, nz))
            self.zs.g.copy_(self.z_dA[..., :nz])
            return self.zs.g
        if self.use_rnn_z:
            K.lstm_z_bwd(self.zs.v, self.zW, self.rnn_z.v, self.z_gates, self.z_cs, drz, self.zs.g, self.dzW, self.dzb,
                         init=(self.z_c0, self.z_h0) if self.learn_init else None,
                         dinit=(self.z_dc0, self.z_dh0) if self.learn_init else None)
            return self.zs.g
        return drz

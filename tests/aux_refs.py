"""Hand-written float64 references of the GRU, sequence-RNN, loss, state-prediction and instance-norm entry points that
tests/gpu_checks_aux.py compares the HIP kernels with.  Each restates one oracle function in the form the kernel computes it (gate
math after the convolutions, every buffer of a recurrence) and takes a `mutate` switch naming a plausible kernel fault;
tests/test_aux_references.py pins every reference to its oracle function and shows that each mutation moves it past the tolerance
of the GPU rows.  CPU only: no device code here."""
import torch

from oracle import ops as O
from oracle import tf_ops as TF

EPS_IN = 1e-6


def act_fn(act, alpha):
    return {'relu': torch.relu, 'lrelu': lambda t: O.lrelu(t, alpha), 'none': lambda t: t}[act]


def inorm(x, gamma, beta, eps=EPS_IN, mutate=None):
    """fused_instance_norm (ops.py, oracle.ops.fused_instance_norm) per (sample, channel) over every spatial position, biased
    variance.  mutate='eps': epsilon 1e-5 instead of the cell's 1e-6."""
    if mutate == 'eps':
        eps = 1e-5
    dims = tuple(range(1, x.dim() - 1))
    m = x.mean(dim=dims, keepdim=True)
    v = ((x - m) ** 2).mean(dim=dims, keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * gamma + beta


def inorm_act(x, gamma, beta, act='relu', alpha=0.0, eps=EPS_IN, mutate=None):
    return act_fn(act, alpha)(inorm(x, gamma, beta, eps, mutate))


# ---- Conv2DGRUCell gate blocks (oracle.savp.conv_gru_cell after its convolutions) --------------------------------------------------
def gru_gates(pre_g, h, g1, b1, eps=EPS_IN):
    """IN(2F) -> sigmoid -> (r, u); returns u and r*h (what the candidate convolution reads in its last F input channels)."""
    r, u = torch.chunk(torch.sigmoid(inorm(pre_g, g1, b1, eps)), 2, dim=-1)
    return u, r * h


def gru_out(pre_c, h, u, g2, b2, eps=EPS_IN):
    """IN(F) -> tanh -> h' = u*h + (1-u)*c."""
    c = torch.tanh(inorm(pre_c, g2, b2, eps))
    return u * h + (1 - u) * c


def conv_gru(x, h, kg, kc, g1, b1, g2, b2, mutate=None):
    """conv_gru_cell restated through gru_gates / gru_out.  The candidate convolution reads [x, h, r*h] (rnn_ops.py:242,258);
    mutate='candidate': it reads [x, r*h] (TF's GRUCell, not this cell) with kc's h rows dropped."""
    pre_g = TF.conv2d(torch.cat([x, h], dim=-1), kg, (1, 1), 'SAME')
    u, rh = gru_gates(pre_g, h, g1, b1)
    if mutate == 'candidate':
        ci = x.shape[-1]
        kc2 = torch.cat([kc[:, :, :ci], kc[:, :, ci + h.shape[-1]:]], dim=2)
        pre_c = TF.conv2d(torch.cat([x, rh], dim=-1), kc2, (1, 1), 'SAME')
    else:
        pre_c = TF.conv2d(torch.cat([x, h, rh], dim=-1), kc, (1, 1), 'SAME')
    return gru_out(pre_c, h, u, g2, b2)


# ---- ConvLSTM gate math without a normaliser (conv_rnn_norm_layer = 'none': rnn_ops.py:148-165 with the bias in the conv) -------------
def lstm_plain(gates, c, forget_bias=1.0, mutate=None):
    """gates [..., 4F] (i, j, f, o) -> (c', h').  mutate='forget_bias': the forget bias is dropped."""
    fb = 0.0 if mutate == 'forget_bias' else forget_bias
    i, j, f, o = torch.chunk(gates, 4, dim=-1)
    cn = c * torch.sigmoid(f + fb) + torch.sigmoid(i) * torch.tanh(j)
    return cn, torch.tanh(cn) * torch.sigmoid(o)


# ---- sequence RNNs: every buffer savp_{lstm,gru}_seq_fwd fills ------------------------------------------------------------------
def _hprev(hs, h0, t, mutate):
    """h_{t-1} of the recurrence; mutate='shift': h_{t-2} (a one-step shift in what the next step reads)."""
    k = t - 2 if mutate == 'shift' else t - 1
    return hs[k] if k >= 0 else h0


def gru_seq(xs, Wg, bg, Wc, bc, h0=None, mutate=None):
    """tf GRUCell over xs [T, B, I] (oracle.tf_ops.gru_cell, unrolled).  Returns A [T,B,I+U] (x | h_{t-1}), A2 (x | r*h_{t-1}),
    ru [T,B,2U], cand [T,B,U], hout [T,B,U], and per step the pre-activations pg / pc and the h_{t-1} node hin (for autograd).  mutate='shift' (see _hprev), 'candidate': the candidate reads [x, h] instead of [x, r*h]."""
    T, B, _ = xs.shape
    U = bc.shape[0]
    h0 = torch.zeros(B, U, dtype=xs.dtype) if h0 is None else h0.expand(B, U)
    A, A2, RU, C, H, PG, PC, HIN = [], [], [], [], [], [], [], []
    for t in range(T):
        h = _hprev(H, h0, t, mutate) * 1.0          # a node of its own: its gradient is what step t alone hands back
        if not h.requires_grad:                     # the zero / fixed initial state: a leaf, so that autograd reports dA there
            h.requires_grad_(True)
        a = torch.cat([xs[t], h], dim=-1)
        pg = a @ Wg + bg
        ru = torch.sigmoid(pg)
        r, u = ru[..., :U], ru[..., U:]
        a2 = torch.cat([xs[t], h if mutate == 'candidate' else r * h], dim=-1)
        pc = a2 @ Wc + bc
        c = torch.tanh(pc)
        A.append(a), A2.append(a2), RU.append(ru), C.append(c), H.append(u * h + (1 - u) * c)
        PG.append(pg), PC.append(pc), HIN.append(h)
    out = {k: torch.stack(v) for k, v in zip(('A', 'A2', 'ru', 'cand', 'hout'), (A, A2, RU, C, H))}
    out.update(pg=PG, pc=PC, hin=HIN)
    return out


def lstm_seq(xs, W, b, forget_bias=1.0, mutate=None):
    """BasicLSTMCell over xs [T, B, I] (oracle.tf_ops.lstm_cell, unrolled; zero state).  Returns A (x | h_{t-1}), gates [T,B,4U],
    cs [T,B,U], hout [T,B,U], and per step the pre-activations g and the h_{t-1} node hin.  mutate='forget_bias' drops the forget bias, 'shift' (see _hprev)."""
    T, B, _ = xs.shape
    U = b.shape[0] // 4
    fb = 0.0 if mutate == 'forget_bias' else forget_bias
    z = torch.zeros(B, U, dtype=xs.dtype)
    A, G, CS, H, HIN = [], [], [], [], []
    c = z
    for t in range(T):
        h = _hprev(H, z, t, mutate) * 1.0
        if not h.requires_grad:                     # the zero / fixed initial state: a leaf, so that autograd reports dA there
            h.requires_grad_(True)
        a = torch.cat([xs[t], h], dim=-1)
        g = a @ W + b
        i, j, f, o = torch.chunk(g, 4, dim=-1)
        c = torch.sigmoid(f + fb) * c + torch.sigmoid(i) * torch.tanh(j)
        A.append(a), G.append(g), CS.append(c), H.append(torch.sigmoid(o) * torch.tanh(c)), HIN.append(h)
    out = {k: torch.stack(v) for k, v in zip(('A', 'gates', 'cs', 'hout'), (A, G, CS, H))}
    out.update(g=G, hin=HIN)
    return out


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
def clip10(r, mutate=None):
    """tf.clip_by_value(r, -10, 10): the gradient passes on the CLOSED interval [-10, 10].  mutate='open_clip': only inside (-10, 10)."""
    inside = (r > -10) & (r < 10) if mutate == 'open_clip' else (r >= -10) & (r <= 10)
    return torch.where(inside, r, r.detach().clamp(-10.0, 10.0))


def kl_gauss(mu1, ls1_raw, mu2, ls2_raw, mutate=None):
    """losses.kl_loss(mu1, clip(ls1), mu2, clip(ls2)) (oracle.train.kl_loss): mean over rows of the per-row sum over the last axis."""
    l1, l2 = clip10(ls1_raw, mutate), clip10(ls2_raw, mutate)
    v = (l2 - l1) / 2 + (torch.exp(l1) + (mu1 - mu2) ** 2) / (2 * torch.exp(l2)) - 0.5
    return v.sum(dim=-1).mean()


def gan_loss(logits, label, gan_loss_type):
    """losses.gan_loss for GAN (sigmoid cross-entropy with a constant label) and SNGAN (softplus), stable forms."""
    def sp(x):                           # exact softplus (torch's switches to x above 20, a relative error of e^-20)
        return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))
    if gan_loss_type == 'GAN':          # softplus(l) - l*z written without the cancellation of its two terms (sp(l) - l = sp(-l))
        return ((1 - label) * sp(logits) + label * sp(-logits)).mean()
    return (sp(logits) if label == 0.0 else sp(-logits)).mean()


def tv_loss(flows, n_channels, s1, s2):
    """base_model.py:763-769 with its means written as the scales the kernel takes: s1 * sum |d/dy| + s2 * sum |d/dx| over the first
    n_channels channels of flows [n, H, W, C]."""
    f = flows[..., :n_channels]
    return s1 * (f[:, 1:] - f[:, :-1]).abs().sum() + s2 * (f[:, :, 1:] - f[:, :, :-1]).abs().sum()


# ---- robot-state recurrence (include/savp_hip.h, savp_state_pred_fwd) ---------------------------------------------------------------
def state_pred(actions, states_in, gt, W, b, mutate=None):
    """state_t = gt[t] ? states_in[t] : gen_{t-1} (gen_{-1} = 0); gen_t = [actions_t | state_t] W + b.  Returns (sa, gen) [T, N, .].
    mutate='shift': a step that takes the prediction reads gen_{t-2}."""
    T, N, ns = states_in.shape
    gens, sas = [], []
    for t in range(T):
        k = t - 2 if mutate == 'shift' else t - 1
        prev = gens[k] if k >= 0 else torch.zeros(N, ns, dtype=states_in.dtype)
        st = torch.where(gt[t][:, None].bool(), states_in[t], prev)
        sa = torch.cat([actions[t], st], dim=-1) if actions is not None else st
        sas.append(sa)
        gens.append(sa @ W + b)
    return torch.stack(sas), torch.stack(gens), gens


def rel(got, ref):
    """max|got - ref| / max|ref| (CPU, fp64)."""
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)

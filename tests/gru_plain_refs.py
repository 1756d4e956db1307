"""Float64 restatements of Conv2DGRUCell WITHOUT a normaliser (normalizer_fn = None, rnn_ops.py:214-224,234-267: conv_rnn_norm_layer =
'none' and ablation_conv_rnn_norm) in the form the pointwise HIP blocks of csrc/gru.hip compute it: the gate math after the two
convolutions, whose outputs include their bias.  tests/test_gru_plain_reference.py pins the composition to oracle.savp.conv_gru_cell and
shows that each `mutate` switch -- a plausible kernel or wiring fault -- moves it past the tolerance of the GPU rows.  CPU only."""
import torch

from oracle import tf_ops as TF


def rel(got, ref):
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def gru_plain_gates(pre_g, h, mutate=None):
    """pre_g [..., 2F] (conv + bias) -> (u, r*h): r = sigmoid(pre_g[..., :F]), u = sigmoid(pre_g[..., F:]); r*h is what the candidate
    convolution reads in its last F input channels.  mutate='swap': r and u taken from the other half."""
    r, u = torch.chunk(torch.sigmoid(pre_g), 2, dim=-1)
    if mutate == 'swap':
        r, u = u, r
    return u, r * h


def gru_plain_out(pre_c, h, u, mutate=None):
    """pre_c [..., F] (conv + bias) -> h' = u*h + (1-u)*tanh(pre_c).  mutate='blend': h' = (1-u)*h + u*c (TF's GRUCell convention reversed)."""
    c = torch.tanh(pre_c)
    if mutate == 'blend':
        return (1 - u) * h + u * c
    return u * h + (1 - u) * c


def conv_gru_plain(x, h, kg, bg, kc, bc, mutate=None):
    """oracle.savp.conv_gru_cell(..., normalized=False) restated through gru_plain_gates / gru_plain_out.  The candidate convolution reads
    [x, h, r*h] (rnn_ops.py:242,258).  mutate: 'bias' -- both biases omitted; 'candidate' -- the candidate's last F channels hold h instead
    of r*h; 'swap' / 'blend' -- see the two blocks."""
    if mutate == 'bias':
        bg, bc = torch.zeros_like(bg), torch.zeros_like(bc)
    pre_g = TF.conv2d(torch.cat([x, h], dim=-1), kg, (1, 1), 'SAME') + bg
    u, rh = gru_plain_gates(pre_g, h, mutate)
    if mutate == 'candidate':
        rh = h
    pre_c = TF.conv2d(torch.cat([x, h, rh], dim=-1), kc, (1, 1), 'SAME') + bc
    return gru_plain_out(pre_c, h, u, mutate)

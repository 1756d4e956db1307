"""CPU self-test of the float64 references in tests/aux_refs.py (no GPU): each equals the oracle function it restates, and each named
mutation -- a plausible kernel fault -- moves it past the tolerance of the GPU rows in tests/gpu_checks_aux.py, so those rows have teeth."""
import numpy as np
import torch

from oracle import ops as O
from oracle import savp as OS
from oracle import tf_ops as TF
from oracle import train as OT
from tests import aux_refs as R

TOL_OP, TOL_GRAD = 2e-5, 1e-4


def rnd(rng, *shape):
    return torch.tensor(rng.standard_normal(shape), dtype=torch.float64)


def test_inorm_matches_oracle_and_eps_matters():
    rng = np.random.default_rng(0)
    x = rnd(rng, 3, 7, 9, 12) * 2 + 0.7
    x[..., 1] = 0.3 + 1e-3 * rnd(rng, 3, 7, 9)
    g, b = rnd(rng, 12) * 0.5 + 1, rnd(rng, 12)
    for act, alpha in (('relu', 0.0), ('lrelu', 0.2), ('none', 0.0)):
        ref = R.act_fn(act, alpha)(O.fused_instance_norm(x, g, b))
        assert R.rel(R.inorm_act(x, g, b, act, alpha), ref) < 1e-12
        assert R.rel(R.inorm_act(x, g, b, act, alpha, mutate='eps'), ref) > 100 * TOL_OP


def test_conv_gru_matches_oracle_and_candidate_input_matters():
    rng = np.random.default_rng(1)
    N, H, W, Ci, F = 2, 6, 5, 3, 8
    x, h = rnd(rng, N, H, W, Ci), rnd(rng, N, H, W, F)
    kg, kc = rnd(rng, 5, 5, Ci + F, 2 * F) * 0.1, rnd(rng, 5, 5, Ci + 2 * F, F) * 0.1
    p = {'conv2dgru_cell/gates/kernel': kg, 'conv2dgru_cell/candidate/kernel': kc,
         'conv2dgru_cell/gates/reset_update/gamma': rnd(rng, 2 * F) * 0.3 + 1, 'conv2dgru_cell/gates/reset_update/beta': rnd(rng, 2 * F) * 0.3,
         'conv2dgru_cell/candidate/state/gamma': rnd(rng, F) * 0.3 + 1, 'conv2dgru_cell/candidate/state/beta': rnd(rng, F) * 0.3}
    ref, _ = OS.conv_gru_cell(OS.Scope(p), x, h, F)
    args = (x, h, kg, kc, p['conv2dgru_cell/gates/reset_update/gamma'], p['conv2dgru_cell/gates/reset_update/beta'],
            p['conv2dgru_cell/candidate/state/gamma'], p['conv2dgru_cell/candidate/state/beta'])
    assert R.rel(R.conv_gru(*args), ref) < 1e-12
    assert R.rel(R.conv_gru(*args, mutate='candidate'), ref) > 100 * TOL_OP


def test_lstm_plain_matches_oracle_and_forget_bias_matters():
    rng = np.random.default_rng(2)
    gates, c = rnd(rng, 2, 4, 4, 32) * 1.5, rnd(rng, 2, 4, 4, 8)
    # oracle.tf_ops.lstm_cell with an identity kernel on [x, h] = [gates, 0] reproduces the gate math after the convolution
    eye = torch.cat([torch.eye(32, dtype=torch.float64), torch.zeros(8, 32, dtype=torch.float64)])
    h_ref, (c_ref, _) = TF.lstm_cell(gates, c, torch.zeros(2, 4, 4, 8, dtype=torch.float64), eye, torch.zeros(32, dtype=torch.float64))
    cn, hn = R.lstm_plain(gates, c)
    assert R.rel(cn, c_ref) < 1e-12 and R.rel(hn, h_ref) < 1e-12
    assert R.rel(R.lstm_plain(gates, c, mutate='forget_bias')[0], c_ref) > 100 * TOL_OP


def _unroll(cell, xs, h0, *w):
    h, hs = h0, []
    for t in range(xs.shape[0]):
        h, _ = cell(xs[t], h, *w)
        hs.append(h)
    return torch.stack(hs)


def test_gru_seq_matches_oracle_and_mutations_fail():
    rng = np.random.default_rng(3)
    T, B, I, U = 6, 3, 5, 8
    xs, h0 = rnd(rng, T, B, I), rnd(rng, U) * 0.5
    Wg, bg, Wc, bc = rnd(rng, I + U, 2 * U) * 0.5, rnd(rng, 2 * U) * 0.3, rnd(rng, I + U, U) * 0.5, rnd(rng, U) * 0.3
    ref = _unroll(TF.gru_cell, xs, h0.expand(B, U), Wg, bg, Wc, bc)
    out = R.gru_seq(xs, Wg, bg, Wc, bc, h0)
    assert R.rel(out['hout'], ref) < 1e-12
    assert R.rel(out['A'][..., I:][1:], ref[:-1]) < 1e-12 and R.rel(out['A'][0, :, I:], h0.expand(B, U)) < 1e-12
    for m in ('shift', 'candidate'):
        assert R.rel(R.gru_seq(xs, Wg, bg, Wc, bc, h0, mutate=m)['hout'], ref) > 100 * TOL_OP


def test_lstm_seq_matches_oracle_and_mutations_fail():
    rng = np.random.default_rng(4)
    T, B, I, U = 6, 3, 5, 16
    xs = rnd(rng, T, B, I)
    W, b = rnd(rng, I + U, 4 * U) * 0.4, rnd(rng, 4 * U) * 0.3
    z = torch.zeros(B, U, dtype=torch.float64)
    c, h, hs = z, z, []
    for t in range(T):
        h, (c, _) = TF.lstm_cell(xs[t], c, h, W, b, forget_bias=1.0)
        hs.append(h)
    ref = torch.stack(hs)
    assert R.rel(R.lstm_seq(xs, W, b, 1.0)['hout'], ref) < 1e-12
    for m in ('shift', 'forget_bias'):
        assert R.rel(R.lstm_seq(xs, W, b, 1.0, mutate=m)['hout'], ref) > 100 * TOL_OP


def test_kl_matches_oracle_and_closed_clip_interval():
    rng = np.random.default_rng(5)
    mu1, mu2 = rnd(rng, 4, 8), rnd(rng, 4, 8)
    ls1, ls2 = rnd(rng, 4, 8) * 3, rnd(rng, 4, 8) * 3
    ls1[0, :4] = torch.tensor([10.0, -10.0, 12.0, -11.0], dtype=torch.float64)
    ls2[1, :2] = torch.tensor([10.0, -10.0], dtype=torch.float64)
    ref = OT.kl_loss(mu1, ls1.clamp(-10, 10), mu2, ls2.clamp(-10, 10))
    assert abs(float(R.kl_gauss(mu1, ls1, mu2, ls2) - ref)) <= 1e-12 * abs(float(ref))

    def grads(mutate):
        leaves = [t.clone().requires_grad_(True) for t in (mu1, ls1, mu2, ls2)]
        R.kl_gauss(*leaves, mutate=mutate).backward()
        return [t.grad for t in leaves]
    g = grads(None)
    assert float(g[1][0, 0]) != 0.0 and float(g[1][0, 1]) != 0.0          # gradient passes at exactly +-10
    assert float(g[1][0, 2]) == 0.0 and float(g[1][0, 3]) == 0.0          # and not beyond
    g_open = grads('open_clip')
    assert max(R.rel(a, b) for a, b in zip(g_open, g)) > 100 * TOL_GRAD


def test_gan_and_tv_match_oracle():
    rng = np.random.default_rng(6)
    lg = rnd(rng, 257) * 3
    lg[:4] = torch.tensor([30.0, -30.0, 90.0, -90.0], dtype=torch.float64)
    for typ in ('GAN', 'SNGAN'):
        for label in (0.0, 1.0):
            ref = OT.gan_loss(lg, label, typ)
            assert abs(float(R.gan_loss(lg, label, typ) - ref)) <= 1e-12 * abs(float(ref))
    f = rnd(rng, 3, 2, 9, 8)
    n, H, W = 3, 2, 9
    d1 = f[:, 1:, :, :6] - f[:, :-1, :, :6]
    d2 = f[:, :, 1:, :6] - f[:, :, :-1, :6]
    ref = d1.abs().sum(dim=-1).mean() + d2.abs().sum(dim=-1).mean()      # base_model.py:763-769 with one flow group
    assert abs(float(R.tv_loss(f, 6, 1.0 / (n * (H - 1) * W), 1.0 / (n * H * (W - 1))) - ref)) <= 1e-12 * float(ref)


def test_state_pred_recurrence_and_shift_fails():
    rng = np.random.default_rng(7)
    T, N, na, ns = 6, 4, 3, 2
    acts, sts = rnd(rng, T, N, na), rnd(rng, T, N, ns)
    gt = torch.tensor([[1] * N] + [[0, 1, 0, 0]] * (T - 1), dtype=torch.int32)
    W, b = rnd(rng, na + ns, ns), rnd(rng, ns)
    sa, gen, _ = R.state_pred(acts, sts, gt, W, b)
    prev = torch.zeros(N, ns, dtype=torch.float64)
    for t in range(T):                 # savp_model.py:411-422: the step takes the ground truth where given, its own prediction elsewhere
        st = torch.where(gt[t][:, None].bool(), sts[t], prev)
        prev = torch.cat([acts[t], st], dim=-1) @ W + b
        assert R.rel(gen[t], prev) < 1e-12
    assert R.rel(R.state_pred(acts, sts, gt, W, b, mutate='shift')[1], gen) > 100 * TOL_OP

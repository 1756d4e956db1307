"""CPU self-test of tests/gru_plain_refs.py (no GPU): the composed cell equals oracle.savp.conv_gru_cell(..., normalized=False), and each
named mutation moves it past 100x the tolerance of the GPU rows in tests/test_gpu_gru_plain.py on seeded inputs with non-zero biases -- so
those rows, and the model-level parity behind them, have teeth."""
import numpy as np
import pytest
import torch

from oracle import savp as OS
from tests import gru_plain_refs as R

TOL_OP = 2e-5          # tests/gpu_checks.py


def rnd(rng, *shape):
    return torch.tensor(rng.standard_normal(shape), dtype=torch.float64)


def _case():
    rng = np.random.default_rng(11)
    N, H, W, Ci, F = 2, 6, 5, 3, 8
    x, h = rnd(rng, N, H, W, Ci), rnd(rng, N, H, W, F)
    kg, kc = rnd(rng, 5, 5, Ci + F, 2 * F) * 0.1, rnd(rng, 5, 5, Ci + 2 * F, F) * 0.1
    bg, bc = rnd(rng, 2 * F) * 0.3 + 1.0, rnd(rng, F) * 0.3         # around the reference's initial values (ones / zeros), non-zero
    p = {'conv2dgru_cell/gates/kernel': kg, 'conv2dgru_cell/gates/bias': bg,
         'conv2dgru_cell/candidate/kernel': kc, 'conv2dgru_cell/candidate/bias': bc}
    ref, state = OS.conv_gru_cell(OS.Scope(p), x, h, F, False)
    assert state is ref
    return (x, h, kg, bg, kc, bc), ref


def test_conv_gru_plain_matches_the_oracle():
    args, ref = _case()
    assert R.rel(R.conv_gru_plain(*args), ref) < 1e-12


@pytest.mark.parametrize('mutate', ['bias', 'candidate', 'swap', 'blend'])
def test_each_mutation_moves_the_result(mutate):
    args, ref = _case()
    moved = R.rel(R.conv_gru_plain(*args, mutate=mutate), ref)
    print(mutate, moved)
    assert moved > 100 * TOL_OP


def test_blocks_are_the_stated_formulas():
    """The two blocks on their own, against the formulas written out (what the GPU rows differentiate)."""
    rng = np.random.default_rng(12)
    F = 4
    pre_g, pre_c, h = rnd(rng, 2, 3, 3, 2 * F), rnd(rng, 2, 3, 3, F), rnd(rng, 2, 3, 3, F)
    u, rh = R.gru_plain_gates(pre_g, h)
    assert R.rel(u, torch.sigmoid(pre_g[..., F:])) < 1e-14 and R.rel(rh, torch.sigmoid(pre_g[..., :F]) * h) < 1e-14
    assert R.rel(R.gru_plain_out(pre_c, h, u), u * h + (1 - u) * torch.tanh(pre_c)) < 1e-14

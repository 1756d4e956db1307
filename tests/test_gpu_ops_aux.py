"""Op-level GPU parity of the GRU, sequence-RNN, loss, state-prediction, fold, plain ConvLSTM, instance-norm option and fused-call entry
points against float64 references (tests/gpu_checks_aux.py)."""
import pytest

pytestmark = pytest.mark.gpu


def _run(name):
    from tests import gpu_checks, gpu_checks_aux
    res = dict(gpu_checks_aux.ALL_AUX_CHECKS)[name]()
    bad = gpu_checks.failures(res)
    assert not bad, 'parity failures (name, err, tol): %r' % bad


def test_instnorm_act_options():
    _run('inorm_options')


def test_convgru_gate_blocks():
    _run('convgru_blocks')


def test_gru_seq():
    _run('gru_seq')


def test_lstm_seq():
    _run('lstm_seq')


def test_losses():
    _run('losses')


def test_state_pred_and_fold64():
    _run('state_pred_fold')


def test_convlstm_gates_no_norm():
    _run('lstm_no_norm')


def test_fused_host_calls():
    _run('fused_calls')

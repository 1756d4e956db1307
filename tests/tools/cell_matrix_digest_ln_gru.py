"""tests/tools/cell_matrix_digest.py with one more row of the conv-RNN matrix: `gru_layer`, the opt-in layer-norm ConvGRU cell
(conv_rnn = 'gru', conv_rnn_norm_layer = 'layer').  Same arguments, same line format:

    python tests/tools/cell_matrix_digest_ln_gru.py [--cell-file OTHER_savp_cell.py] [--only NAME ...] [--out FILE]

The opt-in is set through SAVP_LN_GRU=1 in this process: the switch is read when a model is built and only that row consults it, so every
other line is what cell_matrix_digest.py prints."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.tools import cell_matrix_digest as D      # noqa: E402

D.TRAIN_CONFIGS.append(('gru_layer', 'f32', None, dict(conv_rnn='gru', conv_rnn_norm_layer='layer')))

if __name__ == '__main__':
    os.environ['SAVP_LN_GRU'] = '1'
    D.main()

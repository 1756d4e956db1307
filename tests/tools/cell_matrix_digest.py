"""Launch sequence and result bits of small engines over the conv-RNN matrix: one line per configuration, to compare
two versions of the generator's host code (video_prediction_amd/models/savp_cell.py and what it calls) on one library.

    python tests/tools/cell_matrix_digest.py [--cell-file OTHER_savp_cell.py] [--only NAME ...] [--out FILE]

Every line holds the configuration's name, the number of C-ABI calls of two train_step()s plus one generate(), a SHA-256 of the sequence of
the entry names (recorded by a forwarding proxy returned from lib.get(), the debug poison switches off) and a SHA-256 over the raw bytes of
the generated frames, the loss buffer and every variable and both Adam moments after the second step.  The engines are small (B = 2, T = 5,
64 x 64 x 3, nz = 8, transformation = 'cdna', fixed seeds): the smallest at which every layer of the ladder, every cell class and -- in the
two generate()-only lines at 64 x 80, where training with the instance-norm GRU is refused -- both GRU block families are reached.  The flow
transformation is left out: its scatter is the one kernel whose sums depend on arrival order.

--cell-file loads the given file as video_prediction_amd.models.savp_cell (before savp_model imports it): the same tool then digests
another version of that module, for instance the one of an earlier commit, on the same build.  Two outputs that are equal line for line
mean the same launches in the same order and the same bits.  The SAVP_FUSED_ENTRIES=0 line runs in a child process, because the switch is
read when savp_cell is imported."""
import argparse
import hashlib
import importlib.abc
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CELL_MODULE = 'video_prediction_amd.models.savp_cell'
ABL_NORM = dict(ablation_conv_rnn_norm=True)
# name, datapath, environment of a child process (None: in this process), hparams
TRAIN_CONFIGS = [
    ('lstm_f32', 'f32', None, {}),
    ('lstm_bf16', 'bf16', None, {}),          # the one-launch cell at 16x16 and 8x8, gate convolution + gate block at 32x32
    ('lstm_bf16_fused_entries_0', 'bf16', {'SAVP_FUSED_ENTRIES': '0'}, {}),
    ('lstm_none', 'f32', None, dict(conv_rnn_norm_layer='none')),
    ('lstm_layer', 'f32', None, dict(conv_rnn_norm_layer='layer')),
    ('lstm_abl_norm_instance', 'f32', None, dict(ABL_NORM)),
    ('lstm_abl_norm_layer', 'f32', None, dict(ABL_NORM, conv_rnn_norm_layer='layer')),
    ('gru_instance', 'f32', None, dict(conv_rnn='gru')),
    ('gru_none', 'f32', None, dict(conv_rnn='gru', conv_rnn_norm_layer='none')),
    ('gru_abl_norm', 'f32', None, dict(ABL_NORM, conv_rnn='gru')),
    ('ablation_rnn', 'bf16', None, dict(ablation_rnn=True)),
    ('lstm_learn_initial_state', 'bf16', None, dict(learn_initial_state=True)),
]
# generate() only, 64 x 80: layers 0 and 4 of the instance-norm GRU take the large blocks
TEST_CONFIGS = [('gru_instance_64x80_generate_f32', 'f32'), ('gru_instance_64x80_generate_bf16', 'bf16')]
B, T, NZ = 2, 5, 8


class _CellFile(importlib.abc.MetaPathFinder):
    """Finds CELL_MODULE in the given file; everything else is left to the ordinary finders."""

    def __init__(self, path):
        self.path = path

    def find_spec(self, fullname, path=None, target=None):
        return importlib.util.spec_from_file_location(fullname, self.path) if fullname == CELL_MODULE else None


class _Recorder(object):
    """Stands in for the library: forwards every entry point and notes its name when it is called."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('savp_'):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def _sha(chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c)
    return h.hexdigest()


def _bytes(t):
    import torch
    return t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()


_REC = None


def run_config(name):
    global _REC
    import torch
    from tests import gpu_model_checks as MC
    from video_prediction_amd import debug, kernels as K, lib, variables as V
    from video_prediction_amd.models.savp_model import SAVPEngine
    assert not any(debug.POISON.values()), 'the poison switches change the launch sequence'
    if _REC is None:
        _REC = _Recorder(lib.get())
        lib.get = lambda: _REC
    train = {c[0]: c for c in TRAIN_CONFIGS}
    dev = 'cuda:0'
    if name in train:
        _, prec, _, over = train[name]
        H, W, mode = 64, 64, 'train'
    else:
        prec, over = dict(TEST_CONFIGS)[name], dict(conv_rnn='gru')
        H, W, mode = 64, 80, 'test'
    K.set_conv_precision(prec)
    del _REC.names[:]
    hp = MC.make_hparams(context_frames=2, sequence_length=T, nz=NZ, transformation='cdna', **over)
    vals = V.init_variables(V.variable_specs(hp, (H, W, 3), mode=mode), seed=4)
    eng = SAVPEngine(hp, (H, W, 3), B, mode=mode, values=vals, device=dev)
    eng.set_images(MC.synth(hp, B, H, W, 3, 0).float().to(dev), time_major=True)
    data = []
    if mode == 'train':
        for it in range(2):
            eng.train_step(MC.make_noise(hp, B, seed=100 + it, sampling=True))
        torch.cuda.synchronize()
        data.append(_bytes(eng.loss_buf))
        for g in sorted(eng.store.groups):
            grp = eng.store.groups[g]
            data += [_bytes(grp.p), _bytes(grp.m), _bytes(grp.v)]
    gen = eng.generate(MC.make_noise(hp, B, seed=7, sampling=True))
    torch.cuda.synchronize()
    data.insert(0, _bytes(gen))
    line = '%s calls=%d entries=%s bits=%s' % (name, len(_REC.names), _sha(n.encode() + b'\n' for n in _REC.names), _sha(data))
    del eng, gen
    torch.cuda.empty_cache()
    K.set_conv_precision('f32')
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cell-file', help='a file to load as %s' % CELL_MODULE)
    ap.add_argument('--only', nargs='*', help='names of the configurations to run (default: all)')
    ap.add_argument('--out', help='also write the lines to this file')
    args = ap.parse_args()
    if args.cell_file:
        sys.meta_path.insert(0, _CellFile(os.path.abspath(args.cell_file)))
    names = [c[0] for c in TRAIN_CONFIGS] + [c[0] for c in TEST_CONFIGS]
    child_env = {c[0]: c[2] for c in TRAIN_CONFIGS if c[2]}
    lines = []
    for name in (args.only or names):
        if name not in names:
            ap.error('unknown configuration %r (one of %s)' % (name, ', '.join(names)))
        if name in child_env:          # a switch read at import: a child process with its environment
            cmd = [sys.executable, os.path.abspath(__file__), '--run-one', name] + (['--cell-file', args.cell_file] if args.cell_file else [])
            out = subprocess.run(cmd, env=dict(os.environ, **child_env[name]), stdout=subprocess.PIPE, universal_newlines=True,
                                 timeout=240, check=True).stdout
            line = [ln for ln in out.splitlines() if ln.startswith(name + ' ')][-1]
        else:
            line = run_config(name)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--run-one':
        if '--cell-file' in sys.argv:
            sys.meta_path.insert(0, _CellFile(os.path.abspath(sys.argv[sys.argv.index('--cell-file') + 1])))
        print(run_config(sys.argv[2]), flush=True)
    else:
        main()

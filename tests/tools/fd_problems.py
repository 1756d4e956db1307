"""The implicit-GEMM (conv_fd_kernel) launches of one train step, by distinct problem: which of them the fixed table of
csrc/conv_fd_fixed.h should list.

Build a library with conv_igemm.hip compiled under -DSAVP_FD_LOG (tests/tools/build_fd_log.sh), then
  SAVP_LIB=<that library> python tests/tools/fd_problems.py run 2> fd.log     # two eager steps of the default workload, the last one marked
  python tests/tools/fd_problems.py report fd.log
Every launch leaves one FDLOG line: the planned problem in the order of a table line (between braces: paste it), the epilogue switches,
both tensors' strides, what the caller asked for (tile, split-K) and the index of the table entry it matched (-1: none).  The report
counts the distinct lines of the marked step.  T / B / HW in the environment change the workload (default: the bench configuration)."""
import collections
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def run():
    import torch
    from tests.gpu_model_checks import make_hparams
    from video_prediction_amd.models.savp_model import SAVPEngine
    from video_prediction_amd import kernels as K
    os.environ['SAVP_GRAPH'] = '0'
    K.set_conv_precision('bf16'); K.enable_autotune(True)
    K.load_tuning(os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json'))
    B, T, HW_ = int(os.environ.get('B', 16)), int(os.environ.get('T', 30)), int(os.environ.get('HW', 64))
    hp = make_hparams(context_frames=2, sequence_length=T, batch_size=B, lr=2e-4, beta1=0.5, beta2=0.999, l1_weight=100.0,
                      l2_weight=0.0, kl_weight=1.0, video_sn_vae_gan_weight=0.1, video_sn_gan_weight=0.1,
                      vae_gan_feature_cdist_weight=10.0, gan_feature_cdist_weight=0.0)
    eng = SAVPEngine(hp, (HW_, HW_, 3), B, mode='train')
    eng.set_images(torch.rand(T, B, HW_, HW_, 3, device='cuda:0'), time_major=True)
    eng.train_step()
    torch.cuda.synchronize()
    sys.stderr.write('FDLOG_MARK\n'); sys.stderr.flush()
    eng.train_step()
    torch.cuda.synchronize()


def report(path):
    marked, count = False, collections.Counter()
    for line in open(path):
        line = line.strip()
        if line == 'FDLOG_MARK':
            marked = True
        elif marked and line.startswith('FDLOG '):
            count[line[6:]] += 1
    for k, v in sorted(count.items(), key=lambda kv: -kv[1]):
        print('%4d  %s' % (v, k))
    hit = sum(v for k, v in count.items() if not k.endswith('fixed=-1'))
    print('%d distinct problems, %d launches, %d of them on a fixed instantiation' % (len(count), sum(count.values()), hit))


if __name__ == '__main__':
    run() if sys.argv[1] == 'run' else report(sys.argv[2])

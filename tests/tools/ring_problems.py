"""The ring-kernel launches of one train step, by distinct problem: which of them the fixed table of csrc/conv_ring_fixed.h should list.

Build a library with conv_ring.hip compiled under -DSAVP_RING_LOG (as tests/tools/build_ring_dev.sh does for its flag), then
  SAVP_LIB=<that library> python tests/tools/ring_problems.py run 2> ring.log     # two eager steps of the default workload, the last one marked
  python tests/tools/ring_problems.py report ring.log
Every launch leaves one RINGLOG line (planned geometry, tile, split-K, staging switches, epilogue switches, strides) and one RINGFIXED line
(index of the table entry it matched, -1: none).  The report counts the distinct lines of the marked step; fields a call does not use (the
nb_* group without a workspace) are uninitialised in ConvP and dropped."""
import collections
import os
import re
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
    sys.stderr.write('RINGLOG_MARK\n'); sys.stderr.flush()
    eng.train_step()
    torch.cuda.synchronize()


def report(path):
    marked, count, last = False, collections.Counter(), None
    for line in open(path):
        line = line.strip()
        if line == 'RINGLOG_MARK':
            marked = True
        elif marked and line.startswith('RINGLOG '):
            if ' nb=0,' in line:
                line = re.sub(r'nb=0,\S+ nbx=\S+', 'nb=0', line)
            last = line[8:]
        elif marked and line.startswith('RINGFIXED ') and last:
            count[last + ' fixed=' + line.split()[1]] += 1
            last = None
    for k, v in sorted(count.items(), key=lambda kv: -kv[1]):
        print('%4d  %s' % (v, k))
    hit = sum(v for k, v in count.items() if not k.endswith('fixed=-1'))
    print('%d distinct problems, %d launches, %d of them on a fixed instantiation' % (len(count), sum(count.values()), hit))


if __name__ == '__main__':
    run() if sys.argv[1] == 'run' else report(sys.argv[2])

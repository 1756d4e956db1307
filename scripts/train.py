#!/usr/bin/env python
"""Session-less training runner with the reference's command line (scripts/train.py of alexlee-gk/video_prediction).

Preserved from the reference (file:line under /root/reference/scripts/train.py):
  * every flag, default and help string of :30-61, the output-directory naming from --model / --model_hparams (:68-83),
    --resume / --checkpoint with options.json + dataset_hparams.json + model_hparams.json read back from the checkpoint
    directory (:85-118) and written to the output directory (:193-200);
  * dataset / model construction: the dataset's context_frames / sequence_length / time_shift override the model hparams
    (:151-160), batch size from the model hparams (:162);
  * the step loop: steps run from -1 (log without training) to max_steps - start_step, timing skips steps -1 and 0 (:241-245),
    the progress block every --progress_freq steps (:322-345, same lines: "progress  global step", "image/sec", d_loss / g_loss and
    their terms, learning_rate), checkpoints every --save_freq steps as <output_dir>/model-<global_step> (:347-350, max_to_keep 2).
What TensorFlow did implicitly is explicit here: one `model.train_step(inputs)` is one `sess.run(model.train_op)`.
Summaries (:247-321) go to two places.  <output_dir>/summaries.jsonl gets JSON lines: the training scalars every --summary_freq steps and
one best-of-N row per --eval_summary_freq on a validation batch.  <output_dir>/events.out.tfevents.<time>.<host> is a TensorBoard event
file (video_prediction_amd/summaries.py), opened at the first write: at --summary_freq the scalars of the training batch (losses, psnr /
mse / ssim / lpips of a prior unroll, ground_truth_sampling_mean) and of a validation batch (tag suffix _1; its losses -- g_loss_1,
d_loss_1, gen_l1_loss_1, gen_kl_loss_1, ... -- come from a forward-only pass at the current weights, SAVPEngine.eval_losses: the
reference's summary_op run with the validation handle, train.py:270-289); at --image_summary_freq the GIF boards of images, gen_images, transformed_images, masks and
gen_flows_rgb (+ _enc) for both batches, built on the GPU (csrc/summary.hip) and copied out as uint8 through a pinned buffer; at
--eval_summary_freq the best / mean / worst GIF boards and metric scalars of eval_num_samples prior samples for both batches; at the
multiples of --accum_eval_summary_freq the eval metrics averaged over num_examples_per_epoch() // batch_size validation batches
(accum_..._1; unlike the reference not also at the last iteration, see should_accum_eval) and, when the validation dataset's
long_sequence_length differs from its sequence_length (BAIR 12 / 30, KTH 20 / 40; see long_eval_length), the same for a second,
test-mode model of that length that reads the training model's variables (build_graph(share_with=model); tags accum_..._2,
train.py:136-145,176-191,301-318).  The long model and its dataset iterator both run at a per-GPU batch of max(1, per_gpu // 2), so one
accumulated evaluation walks the validation set once; the reference feeds the full batch into a model whose hparams say half and so
walks the set twice: that quirk is not reproduced.  The summaries.jsonl rows carry neither the validation losses nor the long model.
Not written: the pr_curve-hack plots, boards of gen_images_samples, histograms, graph defs, losses for the training batch at step -1.
A summary pass changes no variable, Adam moment or noise stream, so a run's checkpoints do not depend on the frequencies.
Multi-GPU: launch under `python -m torch.distributed.run --nproc-per-node N` (one process per GPU,
RCCL gradient exchange = --aggregate_nccl 1 of the reference; the per-GPU batch is batch_size / N like tf.split, base_model.py:523-527).
Every replica runs the summary passes, the validation losses and the long model's traversal included, without a collective; the chief
writes the values of its own shard where the reference averages the towers.
SAVP_GUARD=1 (no flag: the flag set is the reference's) trains with the engine's guard: an optimiser group whose gradient holds a NaN or
Inf skips its Adam update.  The progress block then adds both groups' gradient norms and skipped-step counts, the scalar summaries gain
grad_norm_d / grad_norm_g / skipped_steps_d / skipped_steps_g (summaries.jsonl and the event file), and when a group has skipped
SAVP_GUARD_MAX_SKIPS (default 10) steps in a row at a progress check the run prints that group's per-variable report, worst first, saves
the still-finite state as model-<global_step> and exits with a non-zero status.  Without SAVP_GUARD output and files are unchanged.
`--dataset synthetic` (not in the reference) feeds seeded uniform video of --synthetic_shape without record files.
"""
from __future__ import absolute_import, division, print_function

import argparse
import collections
import errno
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--input_dir", type=str, required=True, help="either a directory containing subdirectories "
                                                                     "train, val, test, etc, or a directory containing "
                                                                     "the tfrecords")
    parser.add_argument("--val_input_dir", type=str, help="directories containing the tfrecords. default: input_dir")
    parser.add_argument("--logs_dir", default='logs', help="ignored if output_dir is specified")
    parser.add_argument("--output_dir", help="output directory where json files, summary, model, gifs, etc are saved. "
                                             "default is logs_dir/model_fname, where model_fname consists of "
                                             "information from model and model_hparams")
    parser.add_argument("--output_dir_postfix", default="")
    parser.add_argument("--checkpoint", help="directory with checkpoint or checkpoint name (e.g. checkpoint_dir/model-200000)")
    parser.add_argument("--resume", action='store_true', help='resume from lastest checkpoint in output_dir.')

    parser.add_argument("--dataset", type=str, help="dataset class name")
    parser.add_argument("--dataset_hparams", type=str, help="a string of comma separated list of dataset hyperparameters")
    parser.add_argument("--dataset_hparams_dict", type=str, help="a json file of dataset hyperparameters")
    parser.add_argument("--model", type=str, help="model class name")
    parser.add_argument("--model_hparams", type=str, help="a string of comma separated list of model hyperparameters")
    parser.add_argument("--model_hparams_dict", type=str, help="a json file of model hyperparameters")

    parser.add_argument("--summary_freq", type=int, default=1000, help="save frequency of summaries (except for image and eval summaries) for train/validation set")
    parser.add_argument("--image_summary_freq", type=int, default=5000, help="save frequency of image summaries for train/validation set")
    parser.add_argument("--eval_summary_freq", type=int, default=25000, help="save frequency of eval summaries for train/validation set")
    parser.add_argument("--accum_eval_summary_freq", type=int, default=100000, help="save frequency of accumulated eval summaries for validation set only")
    parser.add_argument("--progress_freq", type=int, default=100, help="display progress every progress_freq steps")
    parser.add_argument("--save_freq", type=int, default=5000, help="save frequence of model, 0 to disable")

    parser.add_argument("--aggregate_nccl", type=int, default=0, help="whether to use nccl or cpu for gradient aggregation in multi-gpu training")
    parser.add_argument("--gpu_mem_frac", type=float, default=0, help="fraction of gpu memory to use")
    parser.add_argument("--seed", type=int)
    # not in the reference: a record-free input for smoke runs
    parser.add_argument("--synthetic_shape", type=str, default='64,64,3', help="H,W,C of --dataset synthetic")
    return parser


def model_fname_from(model, model_hparams):
    """train.py:68-83: 'model=savp,lr=0.1,a=[1,2]' -> 'model.savp.lr.0.1.a.1..2'."""
    list_depth = 0
    out = ''
    for t in ('model=%s,%s' % (model, model_hparams)):
        if t == '[':
            list_depth += 1
        if t == ']':
            list_depth -= 1
        if list_depth and t == ',':
            t = '..'
        if t in '=,':
            t = '.'
        if t in '[]':
            t = ''
        out += t
    return out


def resolve_options(args):
    """train.py:68-118: output directory, --resume, hparams dicts from files and from the checkpoint directory."""
    if args.output_dir is None:
        args.output_dir = os.path.join(args.logs_dir, model_fname_from(args.model, args.model_hparams)) + args.output_dir_postfix
    if args.resume:
        if args.checkpoint:
            raise ValueError('resume and checkpoint cannot both be specified')
        args.checkpoint = args.output_dir
    dataset_hparams_dict, model_hparams_dict = {}, {}
    if args.dataset_hparams_dict:
        with open(args.dataset_hparams_dict) as f:
            dataset_hparams_dict.update(json.loads(f.read()))
    if args.model_hparams_dict:
        with open(args.model_hparams_dict) as f:
            model_hparams_dict.update(json.loads(f.read()))
    if args.checkpoint:
        checkpoint_dir = os.path.normpath(args.checkpoint)
        if not os.path.isdir(args.checkpoint):
            checkpoint_dir, _ = os.path.split(checkpoint_dir)
        if not os.path.exists(checkpoint_dir):
            raise FileNotFoundError(errno.ENOENT, os.strerror(errno.ENOENT), checkpoint_dir)
        with open(os.path.join(checkpoint_dir, "options.json")) as f:
            print("loading options from checkpoint %s" % args.checkpoint)
            options = json.loads(f.read())
            args.dataset = args.dataset or options['dataset']
            args.model = args.model or options['model']
        try:
            with open(os.path.join(checkpoint_dir, "dataset_hparams.json")) as f:
                dataset_hparams_dict.update(json.loads(f.read()))
        except FileNotFoundError:
            print("dataset_hparams.json was not loaded because it does not exist")
        try:
            with open(os.path.join(checkpoint_dir, "model_hparams.json")) as f:
                model_hparams_dict.update(json.loads(f.read()))
        except FileNotFoundError:
            print("model_hparams.json was not loaded because it does not exist")
    return dataset_hparams_dict, model_hparams_dict


class SyntheticVideoDataset(object):
    """Seeded uniform[0,1) video with the dataset-class surface the runner touches (SURVEY.md 8(d) synthetic inputs)."""

    def __init__(self, input_dir, mode='train', num_epochs=None, seed=None, hparams_dict=None, hparams=None, shape=(64, 64, 3)):
        from video_prediction_amd.hparams import HParams
        self.mode, self.seed, self.image_shape = mode, seed or 0, tuple(shape)
        hp = HParams(context_frames=2, sequence_length=12, long_sequence_length=12, time_shift=2, frame_skip=0, force_time_shift=False,
                     shuffle_on_val=False, use_state=False, crop_size=0, scale_size=0)
        hp.override_from_dict(hparams_dict or {})
        if hparams:
            hp.parse(hparams)
        self.hparams = hp

    def num_examples_per_epoch(self):
        return 256

    def set_sequence_length(self, sequence_length):
        self.hparams.sequence_length = sequence_length

    def make_batch(self, batch_size, device='cuda:0', rank=0, world=1):
        import torch
        g = torch.Generator().manual_seed(1234 + 7919 * rank + (0 if self.mode == 'train' else 1))
        T = self.hparams.sequence_length
        while True:
            batch = {'images': torch.rand((batch_size, T) + self.image_shape, generator=g).to(device)}
            if self.hparams.use_state:          # the robot datasets' extra inputs (softmotion_dataset.py:62-64): 3-d end-effector states, 4-d actions
                batch['states'] = torch.randn(batch_size, T, 3, generator=g).cumsum(1).mul(0.1).to(device)
                batch['actions'] = torch.randn(batch_size, T - 1, 4, generator=g).to(device)
            yield batch


def get_dataset_class(name, synthetic_shape):
    if name == 'synthetic':
        import functools
        return functools.partial(SyntheticVideoDataset, shape=tuple(int(v) for v in synthetic_shape.split(',')))
    from video_prediction_amd import datasets
    return datasets.get_dataset_class(name)


def long_length_given(hparams_dict, hparams):
    """Was long_sequence_length set explicitly, in the --dataset_hparams_dict file / the checkpoint's dataset_hparams.json or in the
    --dataset_hparams string(s)?"""
    if 'long_sequence_length' in (hparams_dict or {}):
        return True
    strings = [] if not hparams else (list(hparams) if isinstance(hparams, (list, tuple)) else [hparams])
    return any(kv.split('=')[0].strip() == 'long_sequence_length' for text in strings for kv in text.split(','))


def long_eval_length(dataset, explicit):
    """The sequence length of the second, long model of the accumulated evaluation (train.py:136-145), or None when the dataset has no
    long version: its long_sequence_length where that differs from its sequence_length.  The dataset classes of the reference carry
    their recipe's pair (softmotion 12 / 30, KTH 20 / 40).  SyntheticVideoDataset carries a constant that has nothing to do with the
    sequence_length asked for, so it has a long version only when long_sequence_length was given explicitly (long_length_given).
    Records of a fixed number of frames that is too small for the long version (a dataset written at 12 frames and read with the BAIR
    class and its default of 30) have none either: the reference's long dataset would deliver nothing."""
    if isinstance(dataset, SyntheticVideoDataset) and not explicit:
        return None
    hp = dataset.hparams
    long_length = int(getattr(hp, 'long_sequence_length', 0) or 0)
    if not long_length or long_length == hp.sequence_length:
        return None
    frames = getattr(dataset, '_max_sequence_length', 0)          # 0: the length is per example (KTH), short ones are filtered out
    if frames and not getattr(dataset, 'var_len', False) and (long_length - 1) * (getattr(hp, 'frame_skip', 0) + 1) + 1 > frames:
        return None
    return long_length


def long_eval_batch(per_gpu):
    """Per-GPU batch of the long model: half the training batch (train.py:139, batch_size // 2), at least one sequence."""
    return max(1, per_gpu // 2)


def accum_eval_updates(dataset, per_gpu, world):
    """Updates of one accumulated evaluation: (roughly, up to rounding by the batch size) one traversal of the validation set."""
    return dataset.num_examples_per_epoch() // (per_gpu * world)


def should(step, freq, max_steps, start_step):
    """train.py:232-236."""
    if freq is None:
        return (step + 1) == (max_steps - start_step)
    return bool(freq and ((step + 1) % freq == 0 or (step + 1) in (0, max_steps - start_step)))


def should_eval(step, freq, max_steps, start_step):
    """train.py:236-238: never run eval summaries at the beginning since it's expensive, unless it's the last iteration."""
    return should(step, freq, max_steps, start_step) and (step >= 0 or (step + 1) == (max_steps - start_step))


def should_accum_eval(step, freq):
    """The accumulated evaluation traverses the whole validation set with eval_num_samples draws per batch.  The reference also runs
    it at the last iteration whatever the frequency (should_eval, train.py:301); here it runs only at the multiples of
    --accum_eval_summary_freq: with the default of 100000 a run of a few steps would otherwise spend its time in that traversal.  A run
    whose max_steps is a multiple of the frequency (the reference's recipes: 300000 / 100000) behaves the same."""
    return bool(freq and step >= 0 and (step + 1) % freq == 0)


def prune_checkpoints(output_dir, keep=2):
    """tf.train.Saver(max_to_keep=2), train.py:207."""
    import glob
    import re
    found = {}
    for f in glob.glob(os.path.join(output_dir, 'model-*.index')):
        m = re.search(r'model-(\d+)\.index$', f)
        if m:
            found[int(m.group(1))] = f[:-len('.index')]
    for step in sorted(found)[:-keep]:
        for f in glob.glob(found[step] + '.*'):
            os.remove(f)


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    if args.seed is not None:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
        random.seed(args.seed)
    dataset_hparams_dict, model_hparams_dict = resolve_options(args)

    rank, world, local_rank = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('LOCAL_RANK', '0'))
    chief = rank == 0
    if chief:
        print('----------------------------------- Options ------------------------------------')
        for k, v in args._get_kwargs():
            print(k, "=", v)
        print('------------------------------------- End --------------------------------------')
    if not torch.cuda.is_available():
        raise SystemExit('scripts/train.py needs an MI355X: the SAVP hot path has no CPU fallback')
    torch.cuda.set_device(local_rank)
    device = 'cuda:%d' % local_rank
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        dist_mod.init_process_group(backend='nccl', rank=rank, world_size=world)       # "nccl" is RCCL on ROCm
        dist = dist_mod

    from video_prediction_amd import models
    VideoDataset = get_dataset_class(args.dataset, args.synthetic_shape)
    train_dataset = VideoDataset(args.input_dir, mode='train', seed=args.seed, hparams_dict=dataset_hparams_dict, hparams=args.dataset_hparams)
    val_dataset = VideoDataset(args.val_input_dir or args.input_dir, mode='val', seed=args.seed, hparams_dict=dataset_hparams_dict,
                               hparams=args.dataset_hparams)

    VideoPredictionModel = models.get_model_class(args.model)
    hparams_dict = dict(model_hparams_dict)
    hparams_dict.update({'context_frames': train_dataset.hparams.context_frames,
                         'sequence_length': train_dataset.hparams.sequence_length,
                         'repeat': train_dataset.hparams.time_shift})                  # train.py:151-156
    model = VideoPredictionModel(hparams_dict=hparams_dict, hparams=args.model_hparams, aggregate_nccl=args.aggregate_nccl)
    batch_size = model.hparams.batch_size
    if batch_size % world:
        raise ValueError('batch_size %d is not divisible by %d GPUs' % (batch_size, world))
    per_gpu = batch_size // world                                                       # tf.split over the towers (base_model.py:523-527)
    train_iter = iter(train_dataset.make_batch(per_gpu, device=device, rank=rank, world=world))
    val_iter = iter(val_dataset.make_batch(per_gpu, device=device, rank=rank, world=world))
    inputs = next(train_iter)
    model.build_graph(inputs, device=device)
    if dist is not None:
        model.engine.attach_process_group(dist)

    # the long model of the accumulated evaluation (train.py:136-145,176-191): test mode, sequence_length = the validation dataset's
    # long_sequence_length, the training model's variables (share_with = the reference's reuse_variables()), half the per-GPU batch
    long_model, long_dataset, long_per_gpu, long_iter = None, None, 0, [None]
    long_length = long_eval_length(val_dataset, long_length_given(dataset_hparams_dict, args.dataset_hparams))
    if long_length is not None:
        long_dataset = VideoDataset(args.val_input_dir or args.input_dir, mode='val', seed=args.seed, hparams_dict=dataset_hparams_dict,
                                    hparams=args.dataset_hparams)
        long_dataset.set_sequence_length(long_length)
        long_per_gpu = long_eval_batch(per_gpu)
        long_model = VideoPredictionModel(mode='test', hparams_dict=dict(hparams_dict, sequence_length=long_length),
                                          hparams=args.model_hparams, aggregate_nccl=args.aggregate_nccl)
        long_iter[0] = iter(long_dataset.make_batch(long_per_gpu, device=device, rank=rank, world=world))
        long_model.build_graph(next(long_iter[0]), device=device, share_with=model)
        long_iter[0] = None                         # the first evaluation starts at the head of the set

    if chief:
        if not os.path.exists(args.output_dir):
            os.makedirs(args.output_dir)
        with open(os.path.join(args.output_dir, "options.json"), "w") as f:
            f.write(json.dumps(vars(args), sort_keys=True, indent=4))
        with open(os.path.join(args.output_dir, "dataset_hparams.json"), "w") as f:
            f.write(json.dumps(train_dataset.hparams.values(), sort_keys=True, indent=4))
        with open(os.path.join(args.output_dir, "model_hparams.json"), "w") as f:
            f.write(json.dumps(model.hparams.values(), sort_keys=True, indent=4))
        store = model.engine.store
        print("parameter_count =", sum(int(np.prod(store[n].shape)) for n in store.names() if store.group_of[n] != 'aux'))
    if args.checkpoint:
        model.restore(args.checkpoint)
        if dist is not None:                                                            # every replica continues from rank 0's state
            for g in model.engine.store.groups.values():
                dist.broadcast(g.p, src=0)
    summaries = open(os.path.join(args.output_dir, 'summaries.jsonl'), 'a') if chief else None

    def scalars(info):
        out = {'d_loss': float(info['d_loss']), 'g_loss': float(info['g_loss'])}
        for k, (l, w) in list(info['d_losses'].items()) + list(info['g_losses'].items()):
            out[k] = float(l)
        out.update((k, float(v)) for k, v in model.health_scalars(info).items())      # the guard's four (SAVP_GUARD=1), else nothing
        return out

    GROUP_NAMES = {'d': 'discriminator', 'g': 'generator'}
    guard_max_skips = int(os.environ.get('SAVP_GUARD_MAX_SKIPS', '10'))

    def guard_tripped(info):
        """The group ('d' or 'g') whose last `guard_max_skips` Adam updates were all skipped, or None (synchronises: progress checks only)."""
        health = (info or {}).get('health') or {}
        for grp in ('d', 'g'):
            if 'consecutive_' + grp in health and int(health['consecutive_' + grp]) >= guard_max_skips:
                return grp
        return None

    # TensorBoard summaries (video_prediction_amd/summaries.py).  Every replica runs the summary passes (they touch no variable and no
    # collective, so the replicas stay bit-identical); only the chief opens the event file, at its first write.  The validation batches
    # of these summaries come from an iterator of their own: val_iter above keeps feeding the rows of summaries.jsonl as before.
    from video_prediction_amd import summaries as S
    event_writer, transfer, summary_iter = [None], S.BoardTransfer(), [None]

    def next_summary_batch():
        for _ in range(2):
            if summary_iter[0] is None:
                summary_iter[0] = iter(val_dataset.make_batch(per_gpu, device=device, rank=rank, world=world))
            batch = next(summary_iter[0], None)
            if batch is not None:
                return batch
            summary_iter[0] = None                  # a finite validation set ran out: start over
        raise RuntimeError('the validation dataset delivers no batch')

    def next_long_batch():
        for _ in range(2):
            if long_iter[0] is None:
                long_iter[0] = iter(long_dataset.make_batch(long_per_gpu, device=device, rank=rank, world=world))
            batch = next(long_iter[0], None)
            if batch is not None:
                return batch
            long_iter[0] = None
        raise RuntimeError('the long validation dataset delivers no batch')

    def writer():
        if event_writer[0] is None:
            event_writer[0] = S.EventFileWriter(args.output_dir)
        return event_writer[0]

    def write_scalars(values, global_step, suffix=None):
        if chief:
            writer().add_scalars(collections.OrderedDict((k, float(v)) for k, v in values.items()), global_step, tag_suffix=suffix)

    def write_gifs(boards, global_step, suffix=None):
        if chief:                                   # uint8 boards, through the pinned staging buffer
            writer().add_gifs(transfer.to_host(boards), global_step, tag_suffix=suffix)

    max_steps = model.hparams.max_steps
    start_step = model.global_step
    start_time = time.time()
    info = None
    # start at one step earlier to log everything without doing any training; step is relative to start_step (train.py:240-242)
    def have_batch(it_inputs):
        """End of data (finite num_epochs) must be a collective decision: replicas read different file shards and may run dry at
        different steps -- a rank that left the loop alone would leave the others blocked in the gradient all-reduce."""
        ok = it_inputs is not None
        if dist is not None and getattr(train_dataset, 'num_epochs', None) is not None:     # endless data: no per-step collective / sync
            flag = torch.tensor([1 if ok else 0], device=device, dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            ok = bool(int(flag.item()))
        return ok

    for step in range(-1, max_steps - start_step):
        if step == 1:
            start_time = time.time()            # skip step -1 and 0 for timing purposes (train.py:243-245)
        global_step = model.global_step
        if step >= 0:
            if step > 0:                        # the batch of step 0 was fetched for build_graph; later ones at the top of their own step,
                inputs = next(train_iter, None)  # so that the summary / progress / save blocks below always run for the step just trained
            if not have_batch(inputs):
                break
            run_start_time = time.time()
            info = model.train_step(inputs)
            if should(step, args.progress_freq, max_steps, start_step):
                torch.cuda.synchronize()
            run_elapsed_time = time.time() - run_start_time
            if run_elapsed_time > 1.5 and step > 0 and not should(step, args.progress_freq, max_steps, start_step):
                print('running train_op took too long (%0.1fs)' % run_elapsed_time)
        if chief and info is not None and should(step, args.summary_freq, max_steps, start_step):
            print("recording summary")
            summaries.write(json.dumps(dict(scalars(info), global_step=global_step, tag='summary')) + '\n')
            summaries.flush()
            print("done")
        if step >= 0 and should(step, args.eval_summary_freq, max_steps, start_step):
            # eval summary (train.py:264-265,301-305): best / mean / worst of eval_num_samples prior samples on a validation batch
            print("recording eval summary")
            _, metrics = model.eval_outputs_and_metrics_fn(next(val_iter))
            model.engine.set_images(inputs)                     # back to the training batch (images and, if the model has them, actions / states)
            if chief:
                summaries.write(json.dumps(dict({k: float(v.mean()) for k, v in metrics.items()}, global_step=global_step,
                                                tag='eval_summary_1')) + '\n')
                summaries.flush()
            print("done")
        # TensorBoard event file (train.py:257-321): the training batch, then a validation batch with the tag suffix _1
        do_summary = should(step, args.summary_freq, max_steps, start_step)
        do_image = should(step, args.image_summary_freq, max_steps, start_step)
        do_eval = should_eval(step, args.eval_summary_freq, max_steps, start_step)
        do_accum = should_accum_eval(step, args.accum_eval_summary_freq)
        if do_summary or do_image or do_eval:
            val_inputs = next_summary_batch()        # one validation batch for the three, like the reference's single sess.run
            if do_summary:
                write_scalars(model.scalar_summary_fn(inputs, info), global_step)
                write_scalars(model.scalar_summary_fn(val_inputs, losses=True), global_step, '_1')
            if do_image:
                print("recording image summary")
                write_gifs(model.image_summary_fn(inputs), global_step)
                write_gifs(model.image_summary_fn(val_inputs), global_step, '_1')
                print("done")
            if do_eval:
                for batch, suffix in ((inputs, None), (val_inputs, '_1')):
                    boards, values = model.eval_summary_fn(batch)
                    write_gifs(boards, global_step, suffix)
                    write_scalars(values, global_step, suffix)
        if do_accum:
            # both models (train.py:301-318): reset, then traverse (roughly up to rounding based on the batch size) all the validation
            # dataset; the main model's tags get the suffix _1, the long model's _2
            passes = [(model, val_dataset, next_summary_batch, per_gpu, '_1')]
            if long_model is not None:
                passes.append((long_model, long_dataset, next_long_batch, long_per_gpu, '_2'))
            for eval_model, eval_dataset, next_batch, eval_per_gpu, suffix in passes:
                eval_model.accum_eval_reset()
                num_updates = accum_eval_updates(eval_dataset, eval_per_gpu, world)
                for update_step in range(num_updates):
                    print('evaluating %d / %d' % (update_step + 1, num_updates))
                    eval_model.accum_eval_update(next_batch())
                print("recording accum eval summary")
                write_scalars(eval_model.accum_eval_summary_fn(), global_step, suffix)
                print("done")
        if do_summary or do_image or do_eval or do_accum:
            model.inputs = inputs
            model.engine.set_images(inputs)                     # back to the training batch, as after the eval summary above
            if event_writer[0] is not None:
                event_writer[0].flush()
        if chief and should(step, args.progress_freq, max_steps, start_step):
            # global_step will have the correct step count if we resume from a checkpoint; it is read before it's incremented
            steps_per_epoch = train_dataset.num_examples_per_epoch() / batch_size
            train_epoch = global_step / steps_per_epoch
            print("progress  global step %d  epoch %0.1f" % (global_step + 1, train_epoch))
            if step > 0:
                elapsed_time = time.time() - start_time
                average_time = elapsed_time / step
                images_per_sec = batch_size / average_time
                remaining_time = (max_steps - (start_step + step + 1)) * average_time
                print("          image/sec %0.1f  remaining %dm (%0.1fh) (%0.1fd)" %
                      (images_per_sec, remaining_time / 60, remaining_time / 60 / 60, remaining_time / 60 / 60 / 24))
            if info is not None:
                if info['d_losses']:
                    print("d_loss", float(info["d_loss"]))
                for name, (loss, _) in info['d_losses'].items():
                    print("  ", name, float(loss))
                if info['g_losses']:
                    print("g_loss", float(info["g_loss"]))
                for name, (loss, _) in info['g_losses'].items():
                    print("  ", name, float(loss))
                print("learning_rate", info["learning_rate"])
                health = info.get('health')
                if health:
                    print("grad_norm", "  ".join("%s %g (skipped %d)" % (GROUP_NAMES[grp], float(health['grad_norm_' + grp]),
                                                                          int(health['skipped_' + grp]))
                                                 for grp in ('d', 'g') if 'grad_norm_' + grp in health))
        if step >= 0 and should(step, args.progress_freq, max_steps, start_step):
            # every replica sees the same reduced gradient, hence the same counters: all of them leave together
            bad = guard_tripped(info)
            if bad is not None:
                reason = ('stopping at global step %d: the %s gradient was non-finite in %d consecutive steps (SAVP_GUARD_MAX_SKIPS=%d); '
                          'its updates were skipped' % (model.global_step, GROUP_NAMES[bad], int(info['health']['consecutive_' + bad]),
                                                        guard_max_skips))
                if chief:
                    print("gradient report of the %s group, worst first (variable, norm, non-finite elements)" % GROUP_NAMES[bad])
                    for name, norm, count in sorted(model.engine.health_report(bad), key=lambda r: (-r[2], -r[1])):
                        print("   %s  %g  %d" % (name, norm, count))
                    print("saving model to", args.output_dir)
                    model.save(os.path.join(args.output_dir, "model-%d" % model.global_step))
                    prune_checkpoints(args.output_dir)
                    print("done")
                    summaries.close()
                    if event_writer[0] is not None:
                        event_writer[0].close()
                if dist is not None:
                    dist.destroy_process_group()
                raise SystemExit(reason)
        if chief and step >= 0 and should(step, args.save_freq, max_steps, start_step):
            print("saving model to", args.output_dir)
            model.save(os.path.join(args.output_dir, "model-%d" % model.global_step))
            prune_checkpoints(args.output_dir)
            print("done")
    if summaries:
        summaries.close()
    if event_writer[0] is not None:
        event_writer[0].close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

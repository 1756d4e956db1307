#!/usr/bin/env python
"""Best-of-N evaluation runner with the reference's command line (scripts/evaluate.py of alexlee-gk/video_prediction).

Preserved from the reference (evaluate.py of the reference): every flag and default of :144-172, options / hparams read back from the
checkpoint directory (:181-208), the output directory naming, the three side JSONs (:246-252), the size checks (:232-239), and
save_prediction_eval_results (:77-113): per subtask (max / avg / min) and metric a `prediction_eval_<metric>_<subtask>` tree of
`inputs/context_image_%05d_%02d.png`, `outputs/gen_image_%05d_%02d.png` (future frames only) and the tab-separated
`metrics/<metric>.csv`, which the reference's combine_results.py / plot_results.py read; then the closing psnr / ssim table (:266-285).

The samples are drawn by SAVPVideoPredictionModel.eval_outputs_and_metrics_fn with the model's eval_parallel_iterations: S prior
samples per generator unroll, folded on the GPU (SAVPEngine.eval_outputs_and_metrics).  psnr, ssim and mse are always produced; lpips and
eval_diversity need the AlexNet / LPIPS weights, which the user brings: a file written by scripts/convert_lpips_weights.py, named by the
SAVP_LPIPS_WEIGHTS environment variable (video_prediction_amd/lpips.py).  Without it they are not computed and a line says so.
"""
from __future__ import absolute_import, division, print_function

import argparse
import csv
import json
import os
import random
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.generate import read_checkpoint_options, write_png  # noqa: E402

_NO_EFFECT = ' (accepted for compatibility; has no effect here)'

# (flag, keyword arguments) in the reference's order, evaluate.py:144-172; --synthetic_shape is this repository's addition
_FLAGS = (
    ('input_dir', dict(type=str, required=True, help="either a directory containing subdirectories train, val, test, etc, or a directory "
                                                     "containing the tfrecords")),
    ('results_dir', dict(type=str, default='results', help="ignored if output_dir is specified")),
    ('output_dir', dict(help="output directory where results are saved. default is results_dir/model_fname, where model_fname is the "
                             "directory name of checkpoint")),
    ('checkpoint', dict(help="directory with checkpoint or checkpoint name (e.g. checkpoint_dir/model-200000)")),
    ('mode', dict(type=str, choices=['val', 'test'], default='val', help='mode for dataset, val or test.')),
    ('dataset', dict(type=str, help="dataset class name")),
    ('dataset_hparams', dict(type=str, help="a string of comma separated list of dataset hyperparameters")),
    ('model', dict(type=str, help="model class name")),
    ('model_hparams', dict(type=str, help="a string of comma separated list of model hyperparameters")),
    ('batch_size', dict(type=int, default=8, help="number of samples in batch")),
    ('num_samples', dict(type=int, help="number of samples in total (all of them by default)")),
    ('num_epochs', dict(type=int, default=1)),
    ('eval_substasks', dict(type=str, nargs='+', default=['max', 'avg', 'min'], help='subtasks to evaluate (e.g. max, avg, min)')),
    ('only_metrics', dict(action='store_true')),
    ('num_stochastic_samples', dict(type=int, default=100)),
    ('gt_inputs_dir', dict(type=str, help="directory containing input ground truth images for simple dataset" + _NO_EFFECT)),
    ('gt_outputs_dir', dict(type=str, help="directory containing output ground truth images for simple dataset" + _NO_EFFECT)),
    ('eval_parallel_iterations', dict(type=int, default=10, help="prior samples drawn per generator unroll")),
    ('gpu_mem_frac', dict(type=float, default=0, help="fraction of gpu memory to use" + _NO_EFFECT)),
    ('seed', dict(type=int, default=7)),
    ('synthetic_shape', dict(type=str, default='64,64,3', help="H,W,C of --dataset synthetic (not in the reference)")),
)

UNAVAILABLE_METRICS = ('lpips', 'eval_diversity')      # without LPIPS weights (SAVP_LPIPS_WEIGHTS unset)


def build_parser():
    parser = argparse.ArgumentParser()
    for name, kw in _FLAGS:
        parser.add_argument('--' + name, **kw)
    return parser


def output_dir_of(args, leaf):
    """evaluate.py:206,213: --output_dir, else results_dir/<checkpoint directory name> or results_dir/model.<model>."""
    return args.output_dir or os.path.join(args.results_dir, leaf)


# ---------------------------------------------------------------------------------------------------------------------------------
# host-only writers (evaluate.py:19-113): numpy in, files out
# ---------------------------------------------------------------------------------------------------------------------------------
def to_uint8(image):
    """(x * 255).astype(uint8) -- truncation, as the reference's save_image_sequence; 1-channel frames tiled to RGB."""
    image = (np.asarray(image, dtype=np.float32) * 255.0).astype(np.uint8)
    if image.shape[-1] == 1:
        image = np.tile(image, (1, 1, 3))
    return image


def save_image_sequence(prefix_fname, images, time_start_ind=0):
    head, _ = os.path.split(prefix_fname)
    if head and not os.path.exists(head):
        os.makedirs(head)
    for t, image in enumerate(images):
        write_png('%s_%02d.png' % (prefix_fname, time_start_ind + t), to_uint8(image))


def save_image_sequences(prefix_fname, images, sample_start_ind=0, time_start_ind=0):
    head, _ = os.path.split(prefix_fname)
    if head and not os.path.exists(head):
        os.makedirs(head)
    for i, images_ in enumerate(images):
        save_image_sequence('%s_%05d' % (prefix_fname, sample_start_ind + i), images_, time_start_ind=time_start_ind)


def save_metrics(prefix_fname, metrics, sample_start_ind=0):
    """metrics [sequences, time] -> <prefix>.csv: header `sample_ind 0 .. F-1 mean`, written for the first batch and appended after."""
    head, _ = os.path.split(prefix_fname)
    if head and not os.path.exists(head):
        os.makedirs(head)
    assert metrics.ndim == 2
    file_mode = 'w' if sample_start_ind == 0 else 'a'
    with open('%s.csv' % prefix_fname, file_mode, newline='') as csvfile:
        writer = csv.writer(csvfile, delimiter='\t', quotechar='|', quoting=csv.QUOTE_MINIMAL)
        if sample_start_ind == 0:
            writer.writerow(map(str, ['sample_ind'] + list(range(metrics.shape[1])) + ['mean']))
        for i, metrics_row in enumerate(metrics):
            writer.writerow(map(str, [sample_start_ind + i] + list(metrics_row) + [np.mean(metrics_row)]))


def load_metrics(prefix_fname):
    with open('%s.csv' % prefix_fname, newline='') as csvfile:
        rows = list(csv.reader(csvfile, delimiter='\t', quotechar='|'))
    return np.array(rows)[1:, 1:-1].astype(np.float32)        # without the header, the indices and the means


def save_prediction_eval_results(task_dir, results, model_hparams, sample_start_ind=0, only_metrics=False, subtasks=None):
    """evaluate.py:77-113.  results: batch-major numpy arrays -- 'images' [B, T, H, W, C], 'eval_<metric>/<subtask>' [B, F] and
    'eval_gen_images_<metric>/<subtask>' [B, T-1, H, W, C] (or one 'eval_gen_images' for every metric)."""
    future_length = model_hparams.sequence_length - model_hparams.context_frames
    context_images = results['images'][:, :model_hparams.context_frames]
    if 'eval_diversity' in results:
        save_metrics(os.path.join(task_dir + '_diversity', 'metrics', 'diversity'), results['eval_diversity'],
                     sample_start_ind=sample_start_ind)
    for subtask in subtasks or ['max']:
        metric_names = []
        for k in results.keys():
            m = re.match(r'eval_(\w+)/%s' % subtask, k)
            if m and not re.match(r'eval_gen_images_(\w+)/%s' % subtask, k):
                metric_names.append(m.group(1))
        for metric_name in metric_names:
            subtask_dir = task_dir + '_%s_%s' % (metric_name, subtask)
            gen_images = results.get('eval_gen_images_%s/%s' % (metric_name, subtask), results.get('eval_gen_images'))
            gen_images = gen_images[:, -future_length:]                     # only the future frames
            save_metrics(os.path.join(subtask_dir, 'metrics', metric_name), results['eval_%s/%s' % (metric_name, subtask)],
                         sample_start_ind=sample_start_ind)
            if only_metrics:
                continue
            save_image_sequences(os.path.join(subtask_dir, 'inputs', 'context_image'), context_images, sample_start_ind=sample_start_ind)
            save_image_sequences(os.path.join(subtask_dir, 'outputs', 'gen_image'), gen_images, sample_start_ind=sample_start_ind)


def batch_results(inputs, eval_outputs, eval_metrics):
    """The model's time-major device tensors -> the reference's batch-major numpy fetches (evaluate.py:262-264)."""
    res = {'images': inputs['images'].detach().cpu().numpy()}
    for k, v in list(eval_outputs.items()) + list(eval_metrics.items()):
        if k == 'eval_images':
            continue
        res[k] = v.detach().transpose(0, 1).cpu().numpy()
    return res


def print_metric_tables(output_dir, metric_names=('psnr', 'ssim', 'lpips'), subtasks=('max',)):
    """evaluate.py:266-285 for the tables whose CSV exists."""
    for metric_name in metric_names:
        for subtask in subtasks:
            metric_fname = os.path.join(output_dir, 'prediction_eval_%s_%s' % (metric_name, subtask), 'metrics', metric_name)
            if not os.path.exists(metric_fname + '.csv'):
                continue
            task_name, _, name = metric_fname.split(os.sep)[-3:]
            metric = load_metrics(metric_fname)
            print('=' * 31)
            print(task_name, name)
            print('-' * 31)
            metric_header_format = '{:>10} {:>20}'
            metric_row_format = '{:>10} {:>10.4f} ({:>7.4f})'
            print(metric_header_format.format('time step', name))
            for t, (metric_mean, metric_std) in enumerate(zip(metric.mean(axis=0), metric.std(axis=0))):
                print(metric_row_format.format(t, metric_mean, metric_std))
            print(metric_row_format.format('mean (std)', metric.mean(), metric.std()))
            print('=' * 31)


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    if args.seed is not None:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
        random.seed(args.seed)
    dataset_hparams_dict, model_hparams_dict, leaf = read_checkpoint_options(args)
    args.output_dir = output_dir_of(args, leaf)
    print('----------------------------------- Options ------------------------------------')
    for k, v in args._get_kwargs():
        print(k, "=", v)
    print('------------------------------------- End --------------------------------------')
    if not torch.cuda.is_available():
        raise SystemExit('scripts/evaluate.py needs an MI355X: the SAVP hot path has no CPU fallback')
    device = 'cuda:0'

    from scripts.train import get_dataset_class
    from video_prediction_amd import models
    VideoDataset = get_dataset_class(args.dataset, args.synthetic_shape)
    dataset = VideoDataset(args.input_dir, mode=args.mode, num_epochs=args.num_epochs, seed=args.seed,
                           hparams_dict=dataset_hparams_dict, hparams=args.dataset_hparams)
    VideoPredictionModel = models.get_model_class(args.model)
    hparams_dict = dict(model_hparams_dict)
    hparams_dict.update({'context_frames': dataset.hparams.context_frames, 'sequence_length': dataset.hparams.sequence_length,
                         'repeat': dataset.hparams.time_shift})
    # the model is built for inference for both dataset modes (the reference passes 'val' through and the model rejects it)
    model = VideoPredictionModel(mode='test', hparams_dict=hparams_dict, hparams=args.model_hparams,
                                 eval_num_samples=args.num_stochastic_samples, eval_parallel_iterations=args.eval_parallel_iterations)

    if args.num_samples:
        if args.num_samples > dataset.num_examples_per_epoch():
            raise ValueError('num_samples cannot be larger than the dataset')
        num_examples_per_epoch = args.num_samples
    else:
        num_examples_per_epoch = dataset.num_examples_per_epoch()
    if num_examples_per_epoch % args.batch_size != 0:
        raise ValueError('batch_size should evenly divide the dataset size %d' % num_examples_per_epoch)

    batches = iter(dataset.make_batch(args.batch_size, device=device))
    inputs = next(batches, None)
    if inputs is None:
        raise ValueError('the dataset yielded no batch of %d sequences' % args.batch_size)
    model.build_graph(inputs, device=device)

    output_dir = args.output_dir
    os.makedirs(output_dir, exist_ok=True)
    for fname, content in (("options.json", vars(args)), ("dataset_hparams.json", dataset.hparams.values()),
                           ("model_hparams.json", model.hparams.values())):
        with open(os.path.join(output_dir, fname), "w") as f:
            f.write(json.dumps(content, sort_keys=True, indent=4))
    if args.checkpoint:
        model.restore(args.checkpoint)
    if model.engine.lpips is None:
        print('%s are not computed: they need external AlexNet weights' % ' and '.join(UNAVAILABLE_METRICS))

    sample_ind = 0
    while inputs is not None and not (args.num_samples and sample_ind >= args.num_samples):
        print("evaluation samples from %d to %d" % (sample_ind, sample_ind + args.batch_size))
        eval_outputs, eval_metrics = model.eval_outputs_and_metrics_fn(inputs)
        results = batch_results(inputs, eval_outputs, eval_metrics)
        save_prediction_eval_results(os.path.join(output_dir, 'prediction_eval'), results, model.hparams, sample_ind, args.only_metrics,
                                     args.eval_substasks)
        sample_ind += args.batch_size
        inputs = next(batches, None)
    print_metric_tables(output_dir)


if __name__ == '__main__':
    main()

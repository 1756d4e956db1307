"""TensorBoard summaries on the GPU (pytest -m gpu): the board kernel and flow_to_rgb (csrc/summary.hip) against the numpy references of
tests/oracle_summaries.py, the model's image summary against generator_fn's outputs, and scripts/train.py writing an event file without
touching the training it reports on."""
import functools
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

from tests import oracle_summaries as OS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = 'cuda:0'

# max |kernel - float64 reference| of flow_to_rgb on the inputs of test_flow_to_rgb_against_float64, measured on an MI355X
# (profiles/summaries.md).  The gate is 4x that, and never looser than 1e-5 (200x below half a uint8 step); the margin covers the
# atan2f / sqrtf differences between inputs.
FLOW_MEASURED = 4.76e-7         # 4.757e-07 with rows of 4 channels, 3.886e-07 with rows of 8
FLOW_TOL = min(4 * FLOW_MEASURED, 1e-5)

PLANTED = [0.0, -0.0, 1.0, 1.0 - 2.0 ** -24] + [k / 255.5 for k in (1, 127, 254, 255)] + [1e9, -1e9]


def _board_source(C, M, layout, seed):
    """float32 source with batch 5 as the kernel's caller would hold it, and the [T, 5, H, W, C(, M)] view of it."""
    T, N, H, W = 3, 5, 4, 5
    g = torch.Generator().manual_seed(seed)
    if layout == 'contiguous':
        shape = (T, N, H, W, C) + ((M,) if M > 1 else ())
        buf = torch.rand(shape, generator=g) * 1.5 - 0.25
        flat = buf.reshape(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:3 * len(PLANTED)]
        flat[idx] = torch.tensor(PLANTED * 3, dtype=torch.float32)
        buf = buf.to(DEV)
        return buf, buf
    rowc = 8 + M * C                                             # the mask convolution's input rows: [h_masks (8) | M images of C channels]
    buf = torch.rand(T, N, H, W, rowc, generator=g) * 1.5 - 0.25
    flat = buf[..., 8:].reshape(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:3 * len(PLANTED)]
    flat[idx] = torch.tensor(PLANTED * 3, dtype=torch.float32)
    buf[..., 8:] = flat.reshape(T, N, H, W, M * C)
    buf = buf.to(DEV)
    view = buf[..., 8:8 + M * C].unflatten(-1, (M, C)).transpose(-1, -2)          # [T, N, H, W, C, M]
    return buf, (view if M > 1 else view[..., 0])


@pytest.mark.parametrize('layout', ['contiguous', 'maskin'])
@pytest.mark.parametrize('C,M', [(3, 1), (1, 1), (3, 3), (1, 4)])
@pytest.mark.parametrize('n', [2, 3])
def test_board_kernel_equals_the_numpy_board(C, M, n, layout):
    from video_prediction_amd import kernels as K
    lo = 2
    _, view = _board_source(C, M, layout, seed=100 * C + 10 * M + n)
    src = view[:, lo:lo + n]
    out = K.summary_board_u8(src)
    torch.cuda.synchronize()
    want = OS.board_index(src.cpu().numpy())
    assert tuple(out.shape) == want.shape == (3, M * 4, n * 5, C)             # n * W * C is odd for n = 3, C = 1, 3: the byte tail
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_board_kernel_refusals_leave_out_untouched():
    from video_prediction_amd import kernels as K, lib
    src = torch.rand(3, 2, 4, 5, 2, device=DEV)
    out = torch.full((3, 4, 10, 2), 0xA5, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        K.summary_board_u8(src, out)                                          # C = 2: a feature map
    L = lib.get()
    ok = torch.rand(3, 2, 4, 5, 3, device=DEV)
    out3 = torch.full((3, 4, 10, 3), 0xA5, dtype=torch.uint8, device=DEV)
    st = ok.stride() + (0,)
    assert L.savp_summary_board_u8(lib.stream(), None, *st, 3, 2, 4, 5, 3, 1, out3.data_ptr()) == -1
    assert L.savp_summary_board_u8(lib.stream(), ok.data_ptr(), *st, 3, 2, 4, 5, 3, 1, None) == -1
    for dims in ((0, 2, 4, 5, 3, 1), (3, 0, 4, 5, 3, 1), (3, 2, -1, 5, 3, 1), (3, 2, 4, 0, 3, 1), (3, 2, 4, 5, 0, 1), (3, 2, 4, 5, 3, 0)):
        assert L.savp_summary_board_u8(lib.stream(), ok.data_ptr(), *st, *dims, out3.data_ptr()) == -1, dims
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((out3 == 0xA5).all())


def _flow_inputs(row):
    """Standard-normal flows, T1 = 2, N = 4 = two halves of 2, 4 x 5 pixels, K = 2; every (step, half) scaled differently, so the magnitude
    ranges of the halves (and of the steps) differ by at least 2x and a shared min / max cannot pass."""
    g = torch.Generator().manual_seed(11)
    f = torch.randn(2, 4, 4, 5, row, generator=g)
    scale = torch.tensor([[1.0, 3.0], [0.4, 1.6]]).repeat_interleave(2, dim=1)          # [T1, N]
    f = f * scale.reshape(2, 4, 1, 1, 1)
    assert not bool(((f[..., 2:4] == 0) & (f[..., 0:2] < 0)).any())                    # no y = +0 with x < 0: the one discontinuity (h = 1)
    return f


@pytest.mark.parametrize('row', [4, 8])
def test_flow_to_rgb_against_float64(row):
    """row: the channel count of a flow row (2K = 4, or 8 with four channels of padding the kernel must not read as flows)."""
    from video_prediction_amd import kernels as K
    f = _flow_inputs(row)
    want = OS.flow_to_rgb64(f.numpy(), 2, 2)
    mag = np.sqrt(f.numpy()[..., 0:2].astype(np.float64) ** 2 + f.numpy()[..., 2:4].astype(np.float64) ** 2)
    spans = [mag[t, 2 * h:2 * h + 2].max() - mag[t, 2 * h:2 * h + 2].min() for t in range(2) for h in range(2)]
    assert max(spans[0], spans[1]) / min(spans[0], spans[1]) >= 2 and max(spans[0], spans[2]) / min(spans[0], spans[2]) >= 2
    out = K.flow_to_rgb(f.to(DEV), 2, groups=2)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape == (2, 4, 4, 5, 3, 2)
    err = float(np.abs(got - want).max())
    print('flow_to_rgb row=%d: max abs error %.3e (gate %.3e)' % (row, err, FLOW_TOL))
    shared = OS.flow_to_rgb64(f.numpy(), 2, 1)                                           # one range for both halves: must NOT match
    assert float(np.abs(shared - want).max()) > 0.1
    one_step = OS.flow_to_rgb64(f.numpy().reshape(1, 8, 4, 5, row), 2, 1).reshape(want.shape)      # one range for both steps: neither
    assert float(np.abs(one_step - want).max()) > 0.1
    assert err <= FLOW_TOL, err
    # every (step, half) reaches value 0 and 1 exactly: both passes take the magnitude from the same expression
    v = got.max(axis=4)                                                                  # value = max(r, g, b) at saturation 1
    for t in range(2):
        for h in range(2):
            assert v[t, 2 * h:2 * h + 2].min() == 0.0 and v[t, 2 * h:2 * h + 2].max() == 1.0


@pytest.mark.parametrize('transformation', ['cdna', 'flow'])
def test_image_summary_boards_equal_the_generator_outputs(transformation):
    from video_prediction_amd.models import get_model_class
    from video_prediction_amd.models import savp_model as SM
    Model = get_model_class('savp')
    B, T, H, W = 2, 4, 32, 32
    hp = dict(context_frames=2, sequence_length=T, nz=4, transformation=transformation)
    images = torch.rand(B, T, H, W, 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    m = Model(mode='test', hparams_dict=hp)
    m.build_graph({'images': images})
    noise = m.engine.default_noise()
    boards = m.image_summary_fn({'images': images}, noise=noise)
    boards = {k: v.cpu().numpy() for k, v in boards.items()}
    tm = {'images': images.transpose(0, 1).contiguous()}
    outs = SM.generator_fn(tm, 'test', m.hparams, engine=m.engine, noise=noise)
    names = ['gen_images', 'transformed_images', 'masks'] + (['gen_flows_rgb'] if transformation == 'flow' else [])
    assert set(boards) == {'images'} | set(names) | {k + '_enc' for k in names}
    assert ('gen_flows' in outs) == ('gen_flows_rgb' in outs) == ('gen_flows_enc' in outs) == (transformation == 'flow')
    Mk = m.engine.gen.M
    if transformation == 'flow':
        Kf = m.engine.gen.nk
        assert tuple(outs['gen_flows'].shape) == (T - 1, B, H, W, 2, Kf) and tuple(outs['gen_flows_rgb'].shape) == (T - 1, B, H, W, 3, Kf)
        assert tuple(outs['gen_flows_rgb_enc'].shape) == (T - 1, B, H, W, 3, Kf)
        assert boards['gen_flows_rgb'].shape == (T - 1, Kf * H, B * W, 3)
    assert boards['images'].shape == (T, H, B * W, 3) and boards['masks'].shape == (T - 1, Mk * H, B * W, 1)
    assert boards['transformed_images_enc'].shape == (T - 1, Mk * H, B * W, 3)
    assert np.array_equal(boards['images'], OS.board_index(tm['images'].cpu().numpy()))
    for k in set(boards) - {'images'}:
        want = OS.board_index(outs[k].cpu().numpy())
        assert np.array_equal(boards[k], want), (k, int((boards[k] != want).sum()))


@pytest.mark.parametrize('C,HW', [(4, 64), (8, 100), (16, 1024)])
def test_narrow_all_row_column_sum_repeats_bit_for_bit(C, HW):
    """savp_colsum over all rows of a narrow channel slice (the bias gradients of the 4- and 8-channel head convolutions): the sum equals the
    float64 sum within (n - 1) 2^-24 sum|x| (the bound of any fp32 summation order of n terms), it is ADDED to what `out` holds, and twelve
    repeats give the same bits (partial rows in scratch, added in a fixed order; the earlier atomic adds arrived in any order)."""
    from video_prediction_amd import kernels as K
    R = 6
    g = torch.Generator().manual_seed(C + HW)
    wide = torch.randn(R, HW, C + 8, generator=g).to(DEV)
    x = wide[..., 4:4 + C]                                      # a slice of wider rows, 16-byte aligned
    base = torch.randn(C, generator=g).to(DEV)
    want = base.double().cpu() + x.double().sum(dim=(0, 1)).cpu()
    tol = (R * HW - 1) * 2.0 ** -24 * float(x.abs().double().sum(dim=(0, 1)).max()) + 2.0 ** -23 * float(want.abs().max())
    outs = []
    for _ in range(12):
        out = base.clone()
        K.colsum(x, out)
        outs.append(out)
    torch.cuda.synchronize()
    assert float((outs[0].double().cpu() - want).abs().max()) <= tol
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32))


def _run_train(out, freqs, monkeypatch):
    sys.path.insert(0, ROOT)
    from scripts import train as T
    from video_prediction_amd import models
    orig = models.get_model_class
    monkeypatch.setattr(models, 'get_model_class', lambda name: functools.partial(orig(name), eval_num_samples=2))
    monkeypatch.setattr(T.SyntheticVideoDataset, 'num_examples_per_epoch', lambda self: 8)
    T.main(['--input_dir', 'none', '--dataset', 'synthetic', '--synthetic_shape', '32,32,3', '--model', 'savp', '--output_dir', out,
            '--progress_freq', '0', '--seed', '3', '--dataset_hparams', 'sequence_length=4',
            '--model_hparams', 'batch_size=2,max_steps=3,nz=4,clip_length=3',
            '--summary_freq', str(freqs[0]), '--image_summary_freq', str(freqs[1]), '--eval_summary_freq', str(freqs[2]),
            '--accum_eval_summary_freq', str(freqs[3])])
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def train_runs(tmp_path_factory):
    """scripts/train.py three times, in this process, three steps each on the synthetic dataset at 32x32, batch 2, sequence 4, two evaluation
    samples, a validation set of four batches: run `a` with summary / image / eval / accumulated-eval frequencies 1 / 2 / 3 / 3, run `b` with
    all four 0, run `c` with 1 / 0 / 3 / 0 (the frequencies that write rows of summaries.jsonl as in `a`, the others off)."""
    import contextlib
    import io
    root = tmp_path_factory.mktemp('summaries_train')
    out = {}
    for name, freqs in (('a', (1, 2, 3, 3)), ('b', (0, 0, 0, 0)), ('c', (1, 0, 3, 0))):
        buf = io.StringIO()
        with pytest.MonkeyPatch.context() as mp, contextlib.redirect_stdout(buf):
            _run_train(str(root / name), freqs, mp)
        out[name] = (str(root / name), buf.getvalue())
    return out


def test_train_script_writes_the_event_file(train_runs):
    a, printed = train_runs['a']
    for line in ('recording image summary', 'recording accum eval summary', 'evaluating 1 / 4', 'evaluating 4 / 4', 'done'):
        assert line in printed, line
    ev_files = [f for f in os.listdir(a) if f.startswith('events.out.tfevents.')]
    assert len(ev_files) == 1
    events = OS.read_events(os.path.join(a, ev_files[0]))
    assert events[0].file_version == 'brain.Event:2'
    scalars, images = {}, {}
    for e in events[1:]:
        for v in e.summary.value:
            if v.HasField('image'):
                images[(e.step, v.tag)] = v.image
            else:
                scalars[(e.step, v.tag)] = v.simple_value
    stags, itags = {t for _, t in scalars}, {t for _, t in images}
    for t in ('psnr/psnr', 'psnr_1/psnr', 'ssim/ssim', 'mse_1/mse', 'g_loss/g_loss', 'd_loss/d_loss', 'loss/loss', 'gen_l1_loss/gen_l1_loss',
              'ground_truth_sampling_mean/ground_truth_sampling_mean', 'ground_truth_sampling_mean_enc_1/ground_truth_sampling_mean_enc',
              'eval_psnr/eval_psnr/max', 'eval_ssim_1/eval_ssim/avg', 'accum_eval_psnr_1/accum_eval_psnr/min', 'accum_eval_mse_1/accum_eval_mse/avg'):
        assert t in stags, (t, sorted(stags))
    assert not [t for t in stags if t.startswith('accum_') and not t.split('/')[0].endswith('_1')]
    H = W = 32
    sizes = {t: (im.height, im.width, im.colorspace) for (_, t), im in images.items()}
    assert sizes['images/images/gif'] == (H, 2 * W, 3) and sizes['gen_images_1/gen_images/gif'] == (H, 2 * W, 3)
    assert sizes['masks/masks/gif'][1:] == (2 * W, 1) and sizes['masks/masks/gif'][0] % H == 0 and sizes['masks/masks/gif'][0] > H
    assert sizes['transformed_images_enc_1/transformed_images_enc/gif'] == (sizes['masks/masks/gif'][0], 2 * W, 3)
    assert sizes['eval_gen_images_psnr/eval_gen_images_psnr/min/gif'] == (H, 2 * W, 3) and 'eval_images_1/eval_images/gif' in itags
    frames, durations = OS.decode_gif(images[[k for k in images if k[1] == 'images/images/gif'][0]].encoded_image_string)
    assert frames.shape == (4, H, 2 * W, 3) and set(durations) == {250}
    # the training scalars of the event file are the rows of summaries.jsonl, rounded to float32
    rows = [json.loads(l) for l in open(os.path.join(a, 'summaries.jsonl'))]
    train_rows = [r for r in rows if r['tag'] == 'summary']
    assert len(train_rows) == 3 and any(r['tag'] == 'eval_summary_1' for r in rows)
    for r in train_rows:
        for k, v in r.items():
            if k in ('tag', 'global_step'):
                continue
            got = scalars[(r['global_step'], k + '/' + k)]
            assert struct.pack('<f', got) == struct.pack('<f', v), (k, got, v)
    # no frequency, no event file
    assert not [f for f in os.listdir(train_runs['b'][0]) if f.startswith('events.out.tfevents.')]


def test_final_checkpoint_and_jsonl_equal_those_of_a_run_without_summaries(train_runs):
    """Training does not notice the summaries: the final checkpoint of run `a` (all four frequencies on) is bit-identical, in every variable
    and Adam moment, to that of run `b` (all four frequencies 0) and of run `c`.  summaries.jsonl: a run with --summary_freq 0 and
    --eval_summary_freq 0 writes no row at all, before this change and after it, so `b`'s file is empty and cannot equal `a`'s; the
    comparison is therefore made against `c`, whose row-writing frequencies are `a`'s while the image and accumulated passes (and their
    extra validation batches) are off: byte for byte, except the ssim entries of the evaluation row (see below).
    This needs a train step that repeats bit for bit in the exact-fp32 datapath scripts/train.py uses: the all-row column sums of narrow
    channel slices (the bias gradients of masks/conv2d and scratch_image/conv2d) are added in a fixed order for that (savp_colsum)."""
    from video_prediction_amd import checkpoint as CK
    a, b, c = (train_runs[k][0] for k in 'abc')
    va = CK.read_checkpoint(os.path.join(a, 'model-3'))
    assert any('Adam' in k for k in va)
    for other in (b, c):
        vo = CK.read_checkpoint(os.path.join(other, 'model-3'))
        assert set(va) == set(vo)
        diff = [k for k in va if np.asarray(va[k]).tobytes() != np.asarray(vo[k]).tobytes()]
        print('checkpoint tensors that differ from %s: %d of %d' % (os.path.basename(other), len(diff), len(va)))
        assert not diff, (len(diff), diff[:3])
    assert open(os.path.join(b, 'summaries.jsonl'), 'rb').read() == b''
    la, lc = (open(os.path.join(d, 'summaries.jsonl'), 'rb').read().splitlines() for d in (a, c))
    assert len(la) == len(lc) == 4
    for ra, rc in zip(la, lc):
        if b'"eval_summary_1"' not in ra:
            assert ra == rc                                       # the training rows: byte for byte
            continue
        # The evaluation row: savp_frame_ssim adds a frame's three channel shares with fp32 atomics in arrival order, so the same frames give
        # values a rounding apart from one call to the next ("Not covered"; tests/test_gpu_evaluate.py bounds that
        # effect by rtol 4e-7 per frame, and a mean of frames inherits the bound).  psnr and mse have a single writer per frame: exact.
        da, dc = json.loads(ra), json.loads(rc)
        assert list(da) == list(dc)
        for k in da:
            if 'ssim' in k:
                assert abs(da[k] - dc[k]) <= 4e-7 * abs(dc[k]), (k, da[k], dc[k])
            else:
                assert da[k] == dc[k], (k, da[k], dc[k])


def test_summary_passes_leave_the_training_state_untouched():
    """A model in training (one eager and one captured + replayed step), then every summary pass on the training batch and on another batch:
    every variable, both Adam moments of both optimisers, the spectral-norm vectors, the step counters and the draws of the next train
    step are bit for bit what they were, and the batch staged for the next step is the training batch again once the caller has put it back."""
    from video_prediction_amd.models import get_model_class
    Model = get_model_class('savp')
    B, T = 2, 4
    g = torch.Generator().manual_seed(9)
    train = {'images': torch.rand(B, T, 32, 32, 3, generator=g).to(DEV)}
    val = {'images': torch.rand(B, T, 32, 32, 3, generator=g).to(DEV)}
    m = Model(mode='train', hparams_dict=dict(context_frames=2, sequence_length=T, nz=4, clip_length=3, batch_size=B), eval_num_samples=2)
    m.build_graph(train)
    for _ in range(3):
        info = m.train_step(train)
    eng = m.engine

    def state():
        G_ = eng.store.groups
        s = {'aux.p': G_['aux'].p.clone(), 'images': eng.images_tm.clone()}
        for grp in ('g', 'd'):
            s[grp + '.p'], s[grp + '.m'], s[grp + '.v'] = G_[grp].p.clone(), G_[grp].m.clone(), G_[grp].v.clone()
        return s, (eng.step, G_['g'].t, G_['d'].t), eng.default_noise()
    s0, c0, n0 = state()
    m.scalar_summary_fn(train, info)
    m.scalar_summary_fn(val)
    m.image_summary_fn(train)
    m.image_summary_fn(val)
    m.eval_summary_fn(train)
    m.eval_summary_fn(val)
    m.accum_eval_reset()
    m.accum_eval_update(val)
    m.accum_eval_summary_fn()
    m.inputs = train
    eng.set_images(train)
    torch.cuda.synchronize()
    s1, c1, n1 = state()
    assert c0 == c1
    for k in s0:
        assert torch.equal(s0[k].view(torch.int32), s1[k].view(torch.int32)), k
    assert set(n0) == set(n1)
    for k in n0:
        a_, b_ = n0[k], n1[k]
        if isinstance(a_, dict):
            assert all(torch.equal(a_[j][i], b_[j][i]) for j in a_ for i in (0, 1)), k
        else:
            assert torch.equal(a_, b_), k
    assert eng.graph is not None                     # the step stays captured; the next one replays
    m.train_step(train)
    torch.cuda.synchronize()

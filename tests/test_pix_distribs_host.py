"""Host side of the pix_distribs feature, no GPU: the C ABI entry is declared, exported and mirrored field for field; the opt-in is
parsed from the keyword and the environment; without it every entry point refuses the key and the dataset emits none."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import tfrecord as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('savp_pix_distribs_fwd', 'savp_pix_distribs_lds_resident', 'savp_pixel_distribution')


def test_header_declares_and_library_exports_the_entries(hip_lib):
    from video_prediction_amd import lib
    header = open(os.path.join(ROOT, 'include', 'savp_hip.h')).read()
    declared = set(re.findall(r'\b(savp_[a-z0-9_]+)\s*\(', header))
    raw = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, '%s is not declared in include/savp_hip.h' % name
        assert hasattr(raw, name), 'libsavp_hip.so does not export %s' % name
        assert name in lib.EXPORTS
    assert '} SavpPixDistribArgs;' in header
    assert lib.PIX_MAX_SLOTS == int(re.search(r'#define SAVP_PIX_MAX_SLOTS (\d+)', header).group(1))
    for name, value in (('CDNA', lib.PIX_TF['cdna']), ('DNA', lib.PIX_TF['dna']), ('FLOW', lib.PIX_TF['flow'])):
        assert int(re.search(r'SAVP_PIX_TF_%s = (\d+)' % name, header).group(1)) == value
    for name, value in (('TRANSFORMED', lib.PIX_SLOT_TRANSFORMED), ('CURRENT', lib.PIX_SLOT_CURRENT), ('FIXED', lib.PIX_SLOT_FIXED),
                        ('LAST_CONTEXT', lib.PIX_SLOT_LAST_CONTEXT)):
        assert int(re.search(r'SAVP_PIX_SLOT_%s = (\d+)' % name, header).group(1)) == value


def test_args_struct_layout_matches_the_header(tmp_path):
    """Size and every field offset of SavpPixDistribArgs as gcc lays the header's struct out against the ctypes mirror."""
    from video_prediction_amd import lib
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    c = lib.SavpPixDistribArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "savp_hip.h"', 'int main() {',
             'printf("%zu", sizeof(SavpPixDistribArgs));']
    lines += ['printf(" %%zu", offsetof(SavpPixDistribArgs, %s));' % f[0] for f in c._fields_]
    lines += ['printf("\\n");', 'return 0; }']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(c)] + [getattr(c, f[0]).offset for f in c._fields_]
    assert len(c._fields_) == 35


def _args(lib, H, W, L, **over):
    a = lib.SavpPixDistribArgs()
    a.T1, a.N, a.H, a.W, a.P = 3, 2, H, W, 1
    a.tf, a.kh, a.kw, a.nsrc, a.K = lib.PIX_TF['cdna'], 5, 5, L, 1
    a.context_frames, a.T_in, a.M = 2, 3, L + 1
    for m in range(L):
        a.slot_kind[m], a.slot_arg[m] = lib.PIX_SLOT_TRANSFORMED, m
    a.slot_kind[L] = lib.PIX_SLOT_CURRENT
    a.pix_in = a.gt_mask = a.tfp = a.logits = a.gen = 0x100000
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_lds_residency_predicate_and_argument_checks(hip_lib):
    """Host-side answers, nothing is launched: 64 x 64 with four sources fits the 160 KB of LDS, 128 x 128 fits with one source and not
    with two; the entry refuses what the kernel cannot index before it launches anything."""
    from video_prediction_amd import lib
    fits = lambda a: hip_lib.savp_pix_distribs_lds_resident(ctypes.byref(a))
    assert fits(_args(lib, 64, 64, 4)) == 1 and fits(_args(lib, 128, 128, 1)) == 1
    assert fits(_args(lib, 128, 128, 2)) == 0 and fits(_args(lib, 8, 8, 1, force_global=1)) == 0
    assert hip_lib.savp_pix_distribs_lds_resident(None) == 0
    bad = [dict(nsrc=5), dict(M=17), dict(M=0), dict(T_in=2), dict(tf=3), dict(gen=None), dict(P=0), dict(kh=17, kw=17),
           dict(context_frames=0)]
    for over in bad:
        a = _args(lib, 8, 8, 1, **over)
        if 'context_frames' in over:
            a.slot_kind[1] = lib.PIX_SLOT_LAST_CONTEXT
        assert hip_lib.savp_pix_distribs_fwd(None, ctypes.byref(a)) == -1, over
    a = _args(lib, 8, 8, 1)
    a.slot_arg[0] = 1                                                    # transformation 1 of 1
    assert hip_lib.savp_pix_distribs_fwd(None, ctypes.byref(a)) == -1
    a = _args(lib, 8, 8, 1)
    a.slot_kind[1], a.slot_arg[1] = lib.PIX_SLOT_FIXED, 3                # frame 3 of a 3-frame input
    assert hip_lib.savp_pix_distribs_fwd(None, ctypes.byref(a)) == -1
    assert hip_lib.savp_pixel_distribution(None, None, 1, 1, 4, 4, 0x1000) == -1
    assert hip_lib.savp_pixel_distribution(None, 0x1000, 1, 0, 4, 4, 0x1000) == -1


def test_opt_in_is_parsed_from_the_keyword_and_the_environment(monkeypatch):
    from video_prediction_amd.models import get_model_class
    from video_prediction_amd.models import savp_model as M
    hpd = dict(context_frames=2, sequence_length=4)
    monkeypatch.delenv('SAVP_PIX_DISTRIBS', raising=False)
    assert M.pix_distribs_opt_in() is False and M.pix_distribs_opt_in(True) is True
    assert get_model_class('savp')(mode='test', hparams_dict=hpd).pix_distribs is False
    assert get_model_class('savp')(mode='test', hparams_dict=hpd, pix_distribs=True).pix_distribs is True
    monkeypatch.setenv('SAVP_PIX_DISTRIBS', '1')
    assert M.pix_distribs_opt_in() is True and M.pix_distribs_opt_in(False) is False
    assert get_model_class('savp')(mode='test', hparams_dict=hpd).pix_distribs is True
    assert get_model_class('savp')(mode='test', hparams_dict=hpd, pix_distribs=False).pix_distribs is False
    monkeypatch.setenv('SAVP_PIX_DISTRIBS', '0')
    assert M.pix_distribs_opt_in() is False


def test_without_the_opt_in_the_key_is_refused_everywhere(monkeypatch):
    from video_prediction_amd.models import get_model_class
    from video_prediction_amd.models import savp_model as M
    monkeypatch.delenv('SAVP_PIX_DISTRIBS', raising=False)
    images = np.zeros((2, 4, 64, 64, 3), np.float32)
    inputs = {'images': images, 'pix_distribs': np.zeros((2, 4, 64, 64, 2), np.float32)}
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        M.refuse_conditioning_inputs(inputs)
    model = get_model_class('savp')(mode='test', hparams_dict=dict(context_frames=2, sequence_length=4))
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        model.build_graph(inputs)
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        M.generator_fn(inputs, 'test', model.hparams)

    class NoPix(object):                                                 # an engine built with pix_distribs = 0 changes nothing
        P = 0
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        M.generator_fn(inputs, 'test', model.hparams, engine=NoPix())
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        M.SAVPEngine.set_images(NoPix(), inputs)
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        model._refuse(inputs)
    # the environment variable opts the scripts' model classes in, never the module-level functions: they need an engine built for it
    monkeypatch.setenv('SAVP_PIX_DISTRIBS', '1')
    with pytest.raises(NotImplementedError, match='pix_distribs'):
        M.generator_fn(inputs, 'test', model.hparams)


def test_engine_refuses_a_negative_count_and_a_plain_engine_has_no_pix_state():
    from video_prediction_amd.models import get_model_class
    from video_prediction_amd.models import savp_model as M
    hp = get_model_class('savp')(mode='test', hparams_dict=dict(context_frames=2, sequence_length=4)).hparams
    with pytest.raises(ValueError, match='pix_distribs'):
        M.SAVPEngine(hp, (64, 64, 3), 2, mode='test', device='cpu', pix_distribs=-1)
    eng = M.SAVPEngine(hp, (64, 64, 3), 2, mode='test', device='cpu')
    assert eng.P == 0 and eng.pix_tm is None and eng.pix_n is None and eng.gen.P == 0 and not hasattr(eng.gen, 'gen_pix')
    with pytest.raises(ValueError, match='built without it'):
        eng.set_pix_distribs(np.zeros((2, 4, 64, 64, 1), np.float32))
    eng = M.SAVPEngine(hp, (64, 64, 3), 2, mode='test', device='cpu', pix_distribs=2)
    assert tuple(eng.pix_tm.shape) == (3, 2, 64, 64, 2) and tuple(eng.pix_n.shape) == (3, 4, 64, 64, 2)
    assert tuple(eng.gen.gen_pix.shape) == (3, 4, 64, 64, 2)
    # the slot table in the reference's order: 4 CDNA kernels, previous image, first image, scratch
    from video_prediction_amd import lib
    assert eng.gen.pix_slots == [(lib.PIX_SLOT_TRANSFORMED, m) for m in range(4)] + \
        [(lib.PIX_SLOT_CURRENT, 0), (lib.PIX_SLOT_FIXED, 0), (lib.PIX_SLOT_CURRENT, 0)]
    with pytest.raises(KeyError):
        eng.set_images({'images': np.zeros((2, 4, 64, 64, 3), np.float32)})          # built with the key: a batch without it
    import torch
    for shape in ((2, 4, 64, 64, 3), (2, 4, 32, 64, 2), (2, 4, 64, 32, 2), (2, 2, 64, 64, 2)):      # wrong P, H, W, too few steps
        with pytest.raises(ValueError, match='pix_distribs'):
            eng.set_pix_distribs(torch.zeros(shape))
    eng.set_pix_distribs(torch.ones(2, 5, 64, 64, 2))                     # longer than T1: sliced
    assert float(eng.pix_n.min()) == 1.0


H = W = 16
FRAMES = 6


def _records(tmp_path, with_pos=True):
    d = tmp_path / 'train'
    d.mkdir()
    rng = np.random.default_rng(0)
    exs = []
    for i in range(4):
        feats = {}
        for t in range(FRAMES):
            feats['%d/image_aux1/encoded' % t] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8).tobytes()
            if with_pos:
                feats['%d/object_pos' % t] = [float(i), t / 8.0, 3.5, float(t)]
        exs.append(R.encode_example(feats))
    R.write_records(str(d / 'traj_0_to_3.tfrecords'), exs)
    return str(d)


def test_dataset_reads_object_pos_only_with_the_opt_in(tmp_path, monkeypatch):
    from video_prediction_amd.datasets import SoftmotionVideoDataset
    monkeypatch.delenv('SAVP_PIX_DISTRIBS', raising=False)
    root = _records(tmp_path)
    hpd = dict(sequence_length=4, time_shift=0)
    ds = SoftmotionVideoDataset(root, mode='train', num_epochs=1, hparams_dict=hpd)
    assert ds.pix_distribs is False and ds.num_designated_pixels == 0 and ds._float_keys() == []
    _, floats = ds.make_pipeline(2).next()
    assert floats == []                                                  # nothing for _float_outputs to turn into a key
    assert list(ds._float_outputs(floats, {}, None, 'cpu')) == []
    ds = SoftmotionVideoDataset(root, mode='val', num_epochs=1, hparams_dict=hpd, pix_distribs=True)
    assert ds.num_designated_pixels == 2 and ds._float_keys() == [('%d/object_pos', 4, 0)]
    _, floats = ds.make_pipeline(2).next()
    assert floats[0].shape == (2, 4, 4)
    assert np.array_equal(floats[0][1], np.array([[1.0, t / 8.0, 3.5, float(t)] for t in range(4)], np.float32))
    monkeypatch.setenv('SAVP_PIX_DISTRIBS', '1')
    assert SoftmotionVideoDataset(root, mode='train', num_epochs=1, hparams_dict=hpd).num_designated_pixels == 2
    with pytest.raises(NotImplementedError, match='crop_size / scale_size'):
        SoftmotionVideoDataset(root, mode='train', num_epochs=1, hparams_dict=dict(hpd, scale_size=8)).make_pipeline(2)


def test_dataset_without_object_pos_emits_no_key_even_with_the_opt_in(tmp_path):
    from video_prediction_amd.datasets import SoftmotionVideoDataset
    ds = SoftmotionVideoDataset(_records(tmp_path, with_pos=False), mode='train', num_epochs=1, hparams_dict=dict(sequence_length=4),
                                pix_distribs=True)
    assert ds.pix_distribs is True and ds.num_designated_pixels == 0 and ds._float_keys() == []

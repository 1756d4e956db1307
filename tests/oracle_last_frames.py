"""SAVPCell with last_frames > 1 for the fp64 oracle (oracle/savp.py refuses it and stays as it is).

install(monkeypatch) replaces oracle.savp.savp_cell_call by multi_frame_cell_call; generator_given_z_fn looks the name up at call time
(oracle/savp.py:550), so generator_fn and oracle.train.train_step then unroll the multi-frame cell.  The cell itself is the oracle's:
it is called with an hparams proxy whose last_frames = 1 and num_transformed_images = L * nti (shapes, kernel / flow counts and the mask
count come out as the reference's), while apply_cdna_kernels / apply_dna_kernels / apply_flows are swapped for the reference's list
branches (savp_model.py:926-965) over the whole last_images list for the duration of the call.

Reference semantics (savp_model.py): last_images starts as [images[0]] * L (:281,349) and becomes last_images[1:] + [image] every step,
image being the step's input after the scheduled-sampling select (:406-407); the L * nti kernels / flows are split into L groups with
tf.split, group j is applied to last_images[j] and the outputs are concatenated oldest frame first (:926-965)."""
import torch

import oracle.savp as OS

_cell_call = OS.savp_cell_call
_apply_cdna = OS.apply_cdna_kernels
_apply_dna = OS.apply_dna_kernels
_apply_flows = OS.apply_flows


def _split(params, L):
    """tf.split(params, L, axis=-1): L equal groups of the last axis."""
    n = params.shape[-1]
    assert n % L == 0, (n, L)
    return torch.split(params, n // L, dim=-1)


def apply_cdna_multi(last_images, kernels):
    """apply_kernels, list branch (savp_model.py:937-944), CDNA kernels [B, kh, kw, L*nti]."""
    out = []
    for image, k in zip(last_images, _split(kernels, len(last_images))):
        out.extend(_apply_cdna(image, k))
    return out


def apply_dna_multi(last_images, kernels):
    """apply_kernels, list branch, DNA kernels [B, H, W, kh, kw, L*nti]."""
    out = []
    for image, k in zip(last_images, _split(kernels, len(last_images))):
        out.extend(_apply_dna(image, k))
    return out


def apply_flows_multi(last_images, flows):
    """apply_flows, list branch (savp_model.py:955-965), flows [B, H, W, 2, L*nti]."""
    out = []
    for image, f in zip(last_images, _split(flows, len(last_images))):
        out.extend(_apply_flows(image, f))
    return out


class _SingleFrameView(object):
    """hparams as the oracle's single-frame cell must see them: one source frame carrying all L * nti transformations."""

    def __init__(self, hp):
        self._hp = hp

    def __getattr__(self, name):
        if name == 'last_frames':
            return 1
        if name == 'num_transformed_images':
            return self._hp.last_frames * self._hp.num_transformed_images
        return getattr(self._hp, name)


def multi_frame_cell_call(vs, inputs, states, all_images, ground_truth_t, hp):
    """SAVPCell.call for any last_frames >= 1 (the signature of oracle.savp.savp_cell_call)."""
    B = inputs['images'].shape[0]
    image = torch.where(ground_truth_t.reshape(B, 1, 1, 1), inputs['images'], states['gen_image'])       # :406
    last_images = states['last_images'][1:] + [image]                                                   # :407
    assert len(last_images) == hp.last_frames

    def bind(multi):
        def apply(img, params):
            assert torch.equal(img, last_images[-1])          # the single-frame cell hands over its own copy of the newest image
            return multi(last_images, params)
        return apply
    saved = OS.apply_cdna_kernels, OS.apply_dna_kernels, OS.apply_flows
    OS.apply_cdna_kernels, OS.apply_dna_kernels, OS.apply_flows = bind(apply_cdna_multi), bind(apply_dna_multi), bind(apply_flows_multi)
    try:
        outputs, new_states = _cell_call(vs, inputs, dict(states, last_images=[image]), all_images, ground_truth_t, _SingleFrameView(hp))
    finally:
        OS.apply_cdna_kernels, OS.apply_dna_kernels, OS.apply_flows = saved
    new_states['last_images'] = last_images
    return outputs, new_states


def install(monkeypatch):
    monkeypatch.setattr(OS, 'savp_cell_call', multi_frame_cell_call)

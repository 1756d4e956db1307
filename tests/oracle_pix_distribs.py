"""inputs['pix_distribs'] of SAVPCell for the fp64 oracle (oracle/savp.py does not carry it and stays as it is).  Not a test.

Reference semantics (savp_model.py): the state starts as gen_pix_distrib = zeros, last_pix_distribs = [pix_distribs[0]] * last_frames
(:252-255,288-290,350-351); every step
    pix_distrib = where(ground_truth[t], inputs['pix_distribs'], states['gen_pix_distrib'])                        (:408-409)
    last_pix_distribs = last_pix_distribs[1:] + [pix_distrib]                                                       (:410)
    transformed_pix_distribs = apply_kernels / apply_flows(last_pix_distribs, this step's kernels / flows)          (:598-605)
        + [pix_distrib] (prev_image_background) + [pix_distribs[0]] (first_) + [pix_distribs[context_frames - 1]] (last_)
        + [pix_distribs[min(t, context_frames - 1)]] (last_context_) -- the three suppressed by context_images_background --
        + pix_distribs[:context_frames] (context_images_background) + [pix_distrib] (generate_scratch_image)        (:606-621)
    gen_pix_distrib = sum_m transformed_m * mask_m, divided by its sum over (H, W), no epsilon                      (:648-653)
with the masks of the image path.  The designated pixels P ride where the colour channels do: every transformation is per channel.

step() is one cell call on explicit kernels / flows / masks; recurrence() unrolls it; install() hooks oracle.savp.savp_cell_call so that a
full model's generator_fn returns gen_pix_distribs / transformed_pix_distribs (and their '_enc' twins).  pixel_distribution() is
tf_utils.pixel_distribution (tf_utils.py:562-585) in numpy float32."""
import numpy as np
import torch

import oracle.savp as OS
from tests import oracle_last_frames as OLF


def slot_names(hp):
    """The slots of transformed_pix_distribs in the reference's order (:598-621), as (kind, argument)."""
    cf = hp.context_frames
    names = [('transformed', m) for m in range(hp.last_frames * hp.num_transformed_images)]
    if hp.prev_image_background:
        names.append(('current', 0))
    if hp.first_image_background and not hp.context_images_background:
        names.append(('fixed', 0))
    if hp.last_image_background and not hp.context_images_background:
        names.append(('fixed', cf - 1))
    if hp.last_context_image_background and not hp.context_images_background:
        names.append(('last_context', 0))
    if hp.context_images_background:
        names += [('fixed', k) for k in range(cf)]
    if hp.generate_scratch_image:
        names.append(('current', 0))
    return names


def initial_state(pix_in, hp):
    return {'gen_pix_distrib': torch.zeros_like(pix_in[0]), 'last_pix_distribs': [pix_in[0]] * hp.last_frames}


def step(pix_in, state, t, ground_truth_t, hp, masks, kernels=None, flows=None):
    """One cell call.  pix_in [T, B, H, W, P] (self.inputs['pix_distribs']); ground_truth_t bool [B]; masks [B, H, W, M]; kernels
    [B, kh, kw, L * nti] (cdna) or [B, H, W, kh, kw, L * nti] (dna), normalised; flows [B, H, W, 2, L * nti].
    Returns (gen_pix_distrib [B, H, W, P], transformed_pix_distribs [B, H, W, P, M], new state)."""
    B = pix_in.shape[1]
    cf = hp.context_frames
    pix = torch.where(ground_truth_t.reshape(B, 1, 1, 1), pix_in[t], state['gen_pix_distrib'])
    last = state['last_pix_distribs'][1:] + [pix]
    tr = []
    if hp.transformation == 'flow':
        tr += OLF.apply_flows_multi(last, flows)
    elif hp.transformation == 'cdna':
        tr += OLF.apply_cdna_multi(last, kernels)
    else:
        tr += OLF.apply_dna_multi(last, kernels)
    if hp.prev_image_background:
        tr.append(pix)
    if hp.first_image_background and not hp.context_images_background:
        tr.append(pix_in[0])
    if hp.last_image_background and not hp.context_images_background:
        tr.append(pix_in[cf - 1])
    if hp.last_context_image_background and not hp.context_images_background:
        tr.append(pix_in[t] if t < cf else pix_in[cf - 1])
    if hp.context_images_background:
        tr += list(torch.unbind(pix_in[:cf], dim=0))
    if hp.generate_scratch_image:
        tr.append(pix)
    assert len(tr) == masks.shape[-1], (len(tr), masks.shape)
    gen = sum(tr[m] * masks[..., m:m + 1] for m in range(len(tr)))
    gen = gen / gen.sum(dim=(1, 2), keepdim=True)
    return gen, torch.stack(tr, dim=-1), {'gen_pix_distrib': gen, 'last_pix_distribs': last}


def recurrence(pix_in, ground_truth, hp, masks, kernels=None, flows=None):
    """The unroll over T1 = len(masks) steps on explicit per-step parameters (lists or tensors indexed by t).
    Returns (gen_pix_distribs [T1, B, H, W, P], transformed_pix_distribs [T1, B, H, W, P, M])."""
    state = initial_state(pix_in, hp)
    gens, trs = [], []
    for t in range(len(masks)):
        gen, tr, state = step(pix_in, state, t, ground_truth[t], hp, masks[t], None if kernels is None else kernels[t],
                              None if flows is None else flows[t])
        gens.append(gen)
        trs.append(tr)
    return torch.stack(gens), torch.stack(trs)


def install(monkeypatch, pix_in):
    """Hook oracle.savp.savp_cell_call (after oracle_last_frames.install when last_frames > 1): every unroll of generator_fn also
    carries pix_in [>= T1, B, H, W, P] float64 through the cell's own kernels / flows / masks."""
    inner = OS.savp_cell_call

    def cell_call(vs, inputs, states, all_images, ground_truth_t, hp):
        outputs, new_states = inner(vs, inputs, states, all_images, ground_truth_t, hp)
        t = states['time']
        state = {k: states[k] for k in ('gen_pix_distrib', 'last_pix_distribs')} if 'gen_pix_distrib' in states else initial_state(pix_in, hp)
        gen, tr, state = step(pix_in, state, t, ground_truth_t, hp, outputs['masks'].squeeze(-2), outputs.get('_kernels'), outputs.get('gen_flows'))
        outputs['gen_pix_distribs'], outputs['transformed_pix_distribs'] = gen, tr
        new_states.update(state)
        return outputs, new_states
    monkeypatch.setattr(OS, 'savp_cell_call', cell_call)


def pixel_distribution(pos, height, width):
    """tf_utils.pixel_distribution: pos [B, 2] = (y, x) -> [B, height, width] float32.  tf.one_hot on the flat index y * width + x: an
    index outside [0, height * width) gives a zero row; arithmetic in float32 like the reference's graph."""
    pos = np.asarray(pos, np.float32)
    y, x = pos[:, 0], pos[:, 1]
    x0 = np.floor(x).astype(np.int32)
    y0 = np.floor(y).astype(np.int32)
    x1, y1 = x0 + 1, y0 + 1

    def one_hot(idx):
        out = np.zeros((pos.shape[0], height * width), np.float32)
        ok = (idx >= 0) & (idx < height * width)
        out[np.nonzero(ok)[0], idx[ok]] = 1.0
        return out.reshape(pos.shape[0], height, width)
    f = np.float32
    wa = ((x1.astype(f) - x) * (y1.astype(f) - y))[:, None, None]
    wb = ((x1.astype(f) - x) * (y - y0.astype(f)))[:, None, None]
    wc = ((x - x0.astype(f)) * (y1.astype(f) - y))[:, None, None]
    wd = ((x - x0.astype(f)) * (y - y0.astype(f)))[:, None, None]
    return wa * one_hot(y0 * width + x0) + wb * one_hot(y1 * width + x0) + wc * one_hot(y0 * width + x1) + wd * one_hot(y1 * width + x1)


def pix_distribs_of(object_pos, height, width):
    """softmotion_dataset.py:62-68: object_pos [T, 2P] -> [T, height, width, P]."""
    object_pos = np.asarray(object_pos, np.float32)
    pos = object_pos.reshape(object_pos.shape[0], -1, 2)
    return np.stack([pixel_distribution(pos[:, p], height, width) for p in range(pos.shape[1])], axis=-1)

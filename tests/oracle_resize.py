"""float64 numpy restatement of the reference's per-frame image preprocessing with crop_size / scale_size
(video_prediction/datasets/base_dataset.py:159-184 decode_and_preprocess_image), for the tests of the fused HIP resize kernel.

UNPINNED: TensorFlow is not available to this project's tests, so nothing here was compared with tf.image itself.  It is written from the
documented semantics of the three TF ops the reference calls; tests/test_oracle_resize.py checks it against known answers that do not
depend on this restatement being right (block means, the 2x ramp, weight rows that sum to one, constants, the crop / pad offsets).

  1. crop = crop_size or min(H, W)                                                       (base_dataset.py:166-169)
  2. tf.image.resize_image_with_crop_or_pad(image, crop, crop): per axis with d = crop - dim: d < 0 -> the window starts at (-d) // 2
     (the odd pixel is dropped at the far end); d > 0 -> d // 2 zeros in front, d - d // 2 behind.  The zeros are resized with the image.
  3. scale_size and crop < scale_size: tf.image.resize_images(BILINEAR), the TF1 legacy kernel with align_corners=False and NO half-pixel
     offset: output index y reads position y * crop / S; top = floor(pos), bottom = min(top + 1, crop - 1), lerp = pos - top.
  4. scale_size and crop > scale_size: ResizeMethod.AREA (resize_area, align_corners=False): with s = crop / S output cell y covers
     [y * s, (y + 1) * s); source index i contributes the length of its overlap with the cell (index clamped to crop - 1); the 2-D weight
     is the product of the axes', the sum is divided by s * s.
  5. crop == scale_size or scale_size == 0: the cropped image unchanged.
  6. tf.image.convert_image_dtype(float32).

Both resize methods are separable and linear, so each is one [S, crop] weight matrix per axis: out = Wy @ image @ Wx^T.

Two decisions of this project (video_prediction_amd/datasets/softmotion_dataset.py): the result is resize(image) / 255, in [0, 1] in every
case (the reference leaves a resized batch in [0, 255]: steps 3 / 4 return float32 and step 6 then does nothing); and positions / weights
come from the integers (y * crop) / S and (y * crop) % S, not from TF's float32-rounded scale, so they are exact rationals here too
(fractions.Fraction, converted to float64 once).
"""
from fractions import Fraction

import numpy as np


def crop_or_pad_offsets(dim, crop):
    """(start, before): first source index of the window, zeros in front of it (one of the two is 0)."""
    d = crop - dim
    if d < 0:
        return (-d) // 2, 0
    return 0, d // 2


def crop_or_pad(image, crop):
    """tf.image.resize_image_with_crop_or_pad(image, crop, crop) for image [..., H, W, C]."""
    H, W = image.shape[-3:-1]
    (sy, py), (sx, px) = crop_or_pad_offsets(H, crop), crop_or_pad_offsets(W, crop)
    out = np.zeros(image.shape[:-3] + (crop, crop, image.shape[-1]), dtype=image.dtype)
    h, w = min(H, crop), min(W, crop)
    out[..., py:py + h, px:px + w, :] = image[..., sy:sy + h, sx:sx + w, :]
    return out


def bilinear_weights(n_in, n_out):
    """[n_out, n_in] weights of TF1's legacy bilinear resize (align_corners=False, no half-pixel centres)."""
    w = np.zeros((n_out, n_in), dtype=np.float64)
    for y in range(n_out):
        pos = Fraction(y * n_in, n_out)
        top = pos.numerator // pos.denominator
        bottom = min(top + 1, n_in - 1)
        lerp = pos - top
        w[y, top] += float(1 - lerp)
        w[y, bottom] += float(lerp)
    return w


def area_weights(n_in, n_out):
    """[n_out, n_in] weights of tf.image.resize_area (align_corners=False), already divided by the scale."""
    s = Fraction(n_in, n_out)
    w = np.zeros((n_out, n_in), dtype=np.float64)
    for y in range(n_out):
        lo, hi = y * s, (y + 1) * s
        first = lo.numerator // lo.denominator                       # floor(y * s)
        last = -((-hi.numerator) // hi.denominator)                  # ceil((y + 1) * s)
        for i in range(first, last):
            if i < lo:
                wt = s if i + 1 > hi else i + 1 - lo
            else:
                wt = hi - i if i + 1 > hi else Fraction(1)
            w[y, min(i, n_in - 1)] += float(wt / s)
    return w


def resize_weights(crop, size):
    if crop < size:
        return bilinear_weights(crop, size)
    if crop > size:
        return area_weights(crop, size)
    return np.eye(crop, dtype=np.float64)


def resolve(shape, crop_size=0, scale_size=0):
    """(crop, S) of a record frame [H, W, C] under the two hyper-parameters (steps 1 and 3-5)."""
    crop = crop_size or min(shape[0], shape[1])
    return crop, (scale_size or crop)


def preprocess(frames_u8, crop_size=0, scale_size=0):
    """uint8 [..., H, W, C] -> float64 [..., S, S, C] in [0, 1]."""
    crop, S = resolve(frames_u8.shape[-3:], crop_size, scale_size)
    img = crop_or_pad(frames_u8, crop).astype(np.float64)
    w = resize_weights(crop, S)
    out = np.einsum('yi,...ijc,xj->...yxc', w, img, w)
    return out / 255.0


def taps(crop, size):
    """Source values per output pixel that the issue's error bound counts: 4 for bilinear, (ceil(s) + 1)^2 for area, 1 for a copy."""
    if crop < size:
        return 4
    if crop > size:
        return (-(-crop // size) + 1) ** 2
    return 1

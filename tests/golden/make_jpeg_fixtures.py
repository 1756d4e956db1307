"""Generate tests/golden/jpeg_fixtures.npz (run once where Pillow with libjpeg-turbo is installed: `python tests/golden/make_jpeg_fixtures.py`):
JPEG byte strings written by Pillow and the pixels Pillow (libjpeg-turbo, its default islow IDCT and fancy upsampling -- what
tf.image.decode_jpeg defaults to) decodes from them.  They pin tests/oracle_jpeg.py, the host entropy decoder (libsavp_io.so) and the HIP
IDCT / colour kernel (savp_jpeg_decode_u8) to EQUALITY with libjpeg-turbo; the tests that read the file need no Pillow.

Keys: names (the list below), jpeg_<i> (uint8 bytes), pixels_<i> (uint8 [H, W, C]), refuse_progressive / refuse_cmyk (bytes only),
versions (Pillow and libjpeg-turbo)."""
import io
import os

import numpy as np
from PIL import Image, features
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
SUB = {'444': 0, '422': 1, '420': 2}


def content(kind, h, w, c, rng):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == 'smooth':
        ch = [127.5 + 127.5 * np.sin(0.11 * xx * (k + 1) + 0.07 * yy + k) * np.cos(0.05 * yy * (k + 1)) for k in range(c)]
        img = np.stack(ch, -1)
    elif kind == 'noise':
        img = rng.integers(0, 256, (h, w, c)).astype(np.float64)
    elif kind == 'photo':                                            # smooth + edges + a little noise
        img = np.stack([127.5 + 100 * np.sin(0.09 * xx + k) * np.cos(0.06 * yy) + 60 * ((xx + 2 * yy + 7 * k) % 23 > 11) for k in range(c)], -1)
        img = img + rng.normal(0, 6, img.shape)
    elif kind == 'checker':                                          # black / white, one-pixel period: saturates every clamp
        img = np.repeat((((yy + xx) % 2) * 255)[:, :, None], c, -1)
    elif kind == 'checker3':
        img = np.repeat(((((yy // 3) + (xx // 3)) % 2) * 255)[:, :, None], c, -1)
    elif kind == 'primaries':                                        # saturated colour patches with hard edges
        pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [0, 0, 0], [255, 255, 255]])
        idx = ((yy // 5).astype(int) * 3 + (xx // 7).astype(int)) % 8
        img = pal[idx][:, :, :c].astype(np.float64)
    else:
        raise ValueError(kind)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# (kind, H, W, sampling or 'grey', quality, optimize, restart blocks)
CASES = [
    ('smooth', 64, 64, '420', 50, False, 0), ('photo', 64, 64, '420', 75, False, 0), ('noise', 64, 64, '420', 90, False, 0),
    ('photo', 64, 64, '420', 100, True, 0), ('smooth', 64, 64, '420', 95, False, 3),
    ('smooth', 64, 64, '444', 50, False, 0), ('photo', 64, 64, '444', 85, True, 0), ('noise', 64, 64, '444', 100, False, 5),
    ('smooth', 48, 80, '422', 60, False, 0), ('photo', 48, 80, '422', 95, False, 0), ('noise', 48, 80, '422', 75, True, 2),
    ('photo', 48, 80, 'grey', 50, False, 0), ('noise', 48, 80, 'grey', 100, False, 0), ('smooth', 48, 80, 'grey', 80, True, 4),
    ('photo', 70, 50, '420', 75, False, 0), ('noise', 70, 50, '420', 95, False, 7), ('photo', 70, 50, '422', 90, False, 0),
    ('photo', 70, 50, '444', 75, False, 1), ('photo', 70, 50, 'grey', 90, False, 0),
    ('photo', 9, 17, '420', 90, False, 0), ('noise', 9, 17, '422', 100, False, 0), ('photo', 9, 17, '444', 50, False, 0),
    ('noise', 9, 17, 'grey', 75, False, 1),
    ('photo', 5, 3, '420', 95, False, 0), ('photo', 5, 3, '422', 95, False, 0), ('noise', 20, 7, '420', 90, False, 0),
    ('noise', 6, 20, '420', 90, False, 0), ('photo', 7, 6, '422', 100, False, 0), ('noise', 1, 1, '420', 90, False, 0),
    ('noise', 33, 5, '420', 80, False, 1), ('photo', 3, 4, 'grey', 90, False, 0),
    ('checker', 32, 32, '420', 100, False, 0), ('checker', 32, 32, '444', 100, False, 0), ('checker', 32, 32, 'grey', 100, False, 0),
    ('checker3', 40, 56, '420', 100, False, 0), ('checker3', 40, 56, '422', 50, False, 0),
    ('primaries', 40, 56, '420', 100, False, 0), ('primaries', 40, 56, '444', 100, True, 0), ('primaries', 40, 56, '422', 100, False, 2),
    ('primaries', 96, 80, '420', 75, False, 0), ('photo', 96, 80, '420', 90, True, 10),
]


def encode(img, sampling, quality, optimize, restart, **extra):
    buf = io.BytesIO()
    kw = dict(quality=quality, optimize=optimize, **extra)
    if sampling != 'grey':
        kw['subsampling'] = SUB[sampling]
    if restart:
        kw['restart_marker_blocks'] = restart
    Image.fromarray(img[:, :, 0] if sampling == 'grey' else img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def main():
    assert features.check('libjpeg_turbo'), 'the fixtures pin libjpeg-turbo arithmetic'
    rng = np.random.default_rng(1807)
    out = {}
    names = []
    for i, (kind, h, w, sampling, q, opt, rst) in enumerate(CASES):
        c = 1 if sampling == 'grey' else 3
        data = encode(content(kind, h, w, c, rng), sampling, q, opt, rst)
        pix = np.asarray(Image.open(io.BytesIO(data)))
        pix = pix[:, :, None] if pix.ndim == 2 else pix
        assert pix.shape == (h, w, c)
        names.append('%s %dx%d %s q%d%s%s' % (kind, h, w, sampling, q, ' opt' if opt else '', ' rst%d' % rst if rst else ''))
        out['jpeg_%d' % i] = np.frombuffer(data, np.uint8)
        out['pixels_%d' % i] = pix
    img = content('photo', 32, 32, 3, rng)
    out['refuse_progressive'] = np.frombuffer(encode(img, '420', 80, False, 0, progressive=True), np.uint8)
    buf = io.BytesIO()
    Image.fromarray(np.concatenate([img, img[:, :, :1]], -1), 'CMYK').save(buf, 'JPEG', quality=80)
    out['refuse_cmyk'] = np.frombuffer(buf.getvalue(), np.uint8)
    out['names'] = np.array(names)
    out['versions'] = np.array(['Pillow %s' % PIL.__version__, 'libjpeg-turbo %s' % features.version('jpg')])
    path = os.path.join(HERE, 'jpeg_fixtures.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(names), 'streams')


if __name__ == '__main__':
    main()

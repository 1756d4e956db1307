"""NumPy restatement of baseline JPEG decoding with the integer arithmetic of libjpeg / libjpeg-turbo (what tf.image.decode_jpeg
defaults to: dct_method default = jidctint "islow", fancy_upscaling=True).  Test infrastructure: the product never imports it.

Two halves, like the product:
  * parse / entropy_decode   marker walk + Huffman decoding (ITU T.81 annex F) -> geometry, int16 coefficients [total_blocks, 64]
                             (component-major, blocks in raster order padded to whole MCUs, row-major inside a block, not dequantised)
                             and the quantisation tables [components, 64] in the same order: the hand-off format of
                             savp_jpeg_entropy_decode (include/savp_io.h) to savp_jpeg_decode_u8 (include/savp_hip.h).
  * pixels                   dequantise, jidctint IDCT, crop the planes, fancy upsampling, YCbCr -> RGB: uint8 [H, W, C].

One rule beyond the formulas: libjpeg selects the "fancy" (triangle) upsampler only for a component whose downsampled width exceeds 2
(jdsample.c: `do_fancy && compptr->downsampled_width > 2`); a narrower chroma plane is replicated (box filter) in both directions.
test_jpeg_host.py::test_oracle_equals_pillow pins all of it against pixels recorded from Pillow."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])        # ZIGZAG[k] = row-major position of the k-th coefficient of the stream


class Unsupported(ValueError):
    pass


class Corrupt(ValueError):
    pass


def _u16(d, i):
    if i + 2 > len(d):
        raise Corrupt('truncated')
    return (d[i] << 8) | d[i + 1]


def parse(data):
    """Headers up to and including SOS.  Returns a dict: width, height, components, h, v, tq, blocks_w, blocks_h, block_offset,
    total_blocks, mcus_x, mcus_y, qt {id: uint16[64] row-major}, dc / ac {id: (counts[16], values)}, scan [(comp, td, ta)], restart,
    pos (offset of the entropy-coded data)."""
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Corrupt('no SOI')
    i = 2
    qt, dc, ac = {}, {}, {}
    frame = None
    restart = 0
    adobe = None
    while True:
        if i >= len(d):
            raise Corrupt('truncated')
        if d[i] != 0xFF:
            raise Corrupt('marker expected')
        while i < len(d) and d[i] == 0xFF:                       # fill bytes
            i += 1
        if i >= len(d):
            raise Corrupt('truncated')
        m = d[i]
        i += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Corrupt('EOI before SOS')
        n = _u16(d, i)
        if n < 2 or i + n > len(d):
            raise Corrupt('truncated segment')
        seg = d[i + 2:i + n]
        i += n
        if m in (0xC0, 0xC1):
            if frame is not None:
                raise Corrupt('two frames')
            if len(seg) < 6:
                raise Corrupt('short SOF')
            if seg[0] != 8:
                raise Unsupported('%d-bit precision' % seg[0])
            H, W, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc == 4:
                raise Unsupported('4 components')
            if nc not in (1, 3):
                raise Unsupported('%d components' % nc)
            if len(seg) != 6 + 3 * nc or H == 0 or W == 0:
                raise Corrupt('bad SOF')
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
            frame = (H, W, comps)
        elif m == 0xC2:
            raise Unsupported('progressive')
        elif m in (0xC3, 0xC7, 0xCB, 0xCF):
            raise Unsupported('lossless')
        elif m in (0xC9, 0xCA, 0xCD, 0xCE, 0xCC):
            raise Unsupported('arithmetic coding')
        elif m in (0xC5, 0xC6):
            raise Unsupported('hierarchical')
        elif m == 0xC4:
            j = 0
            while j < len(seg):
                if j + 17 > len(seg):
                    raise Corrupt('short DHT')
                tc, th = seg[j] >> 4, seg[j] & 15
                counts = list(seg[j + 1:j + 17])
                tot = sum(counts)
                if tc > 1 or th > 3 or tot > 256 or j + 17 + tot > len(seg):
                    raise Corrupt('bad DHT')
                (ac if tc else dc)[th] = (counts, list(seg[j + 17:j + 17 + tot]))
                j += 17 + tot
        elif m == 0xDB:
            j = 0
            while j < len(seg):
                pq, tq = seg[j] >> 4, seg[j] & 15
                if pq == 1:
                    raise Unsupported('16-bit DQT')
                if pq > 1 or tq > 3 or j + 65 > len(seg):
                    raise Corrupt('bad DQT')
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[j + 1:j + 65], np.uint8)
                qt[tq] = t
                j += 65
        elif m == 0xDD:
            if len(seg) != 2:
                raise Corrupt('bad DRI')
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b'Adobe':
            adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Corrupt('SOS before SOF')
            break
        # APPn, COM and anything else with a length: skipped
    H, W, comps = frame
    nc = len(comps)
    if adobe is not None and nc == 3 and adobe != 1:
        raise Unsupported('Adobe transform %d' % adobe)
    hs, vs = [c[1] for c in comps], [c[2] for c in comps]
    if nc == 1:
        hs, vs = [1], [1]                                         # a single-component scan is never interleaved: sampling factors are moot
    elif not (hs[1] == vs[1] == hs[2] == vs[2] == 1 and (hs[0], vs[0]) in ((1, 1), (2, 1), (2, 2))):
        raise Unsupported('sampling %s' % 'x'.join('%d%d' % hv for hv in zip(hs, vs)))
    if len(seg) < 1 or seg[0] != nc or len(seg) != 4 + 2 * nc:
        if len(seg) >= 1 and 1 <= seg[0] < nc and len(seg) == 4 + 2 * seg[0]:
            raise Unsupported('non-interleaved scans')
        raise Corrupt('bad SOS')
    scan = []
    for k in range(nc):
        cid, t = seg[1 + 2 * k], seg[2 + 2 * k]
        if cid != comps[k][0]:
            raise Corrupt('scan component order')
        scan.append((k, t >> 4, t & 15))
    hmax, vmax = max(hs), max(vs)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    bw, bh = [mx * h for h in hs], [my * v for v in vs]
    off = [0]
    for c in range(nc):
        off.append(off[-1] + bw[c] * bh[c])
    for c in range(nc):
        if comps[c][3] not in qt:
            raise Corrupt('missing DQT')
    for _, td, ta in scan:
        if td not in dc or ta not in ac:
            raise Corrupt('missing DHT')
    return dict(width=W, height=H, components=nc, h=hs, v=vs, tq=[c[3] for c in comps], blocks_w=bw, blocks_h=bh, block_offset=off[:nc],
                total_blocks=off[nc], mcus_x=mx, mcus_y=my, qt=qt, dc=dc, ac=ac, scan=scan, restart=restart, pos=i)


def info(data):
    p = parse(data)
    return {k: p[k] for k in ('width', 'height', 'components', 'h', 'v', 'blocks_w', 'blocks_h', 'block_offset', 'total_blocks')}


class _Huff(object):
    """Canonical code of one DHT table: code -> value by length (T.81 annex C / F.2.2.3)."""

    def __init__(self, counts, values):
        self.table = {}
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                if code >= (1 << length):
                    raise Corrupt('over-subscribed DHT')
                self.table[(length, code)] = values[k]
                code += 1
                k += 1
            code <<= 1


class _Bits(object):
    def __init__(self, d, pos):
        self.d, self.pos, self.acc, self.n = d, pos, 0, 0

    def bit(self):
        if self.n == 0:
            d, p = self.d, self.pos
            if p >= len(d):
                raise Corrupt('truncated scan')
            b = d[p]
            p += 1
            if b == 0xFF:
                if p >= len(d):
                    raise Corrupt('truncated scan')
                if d[p] != 0:
                    raise Corrupt('marker inside the scan')
                p += 1
            self.pos, self.acc, self.n = p, b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def receive(self, s):
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def decode(self, h):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            v = h.table.get((length, code))
            if v is not None:
                return v
        raise Corrupt('bad Huffman code')

    def marker(self):
        """Drop the padding bits and read the marker that follows (fill bytes allowed)."""
        self.n = 0
        d, p = self.d, self.pos
        if p >= len(d) or d[p] != 0xFF:
            raise Corrupt('marker expected')
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Corrupt('truncated')
        self.pos = p + 1
        return d[p]


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def entropy_decode(data):
    """(parsed header dict, coef int16 [total_blocks, 64], qtab uint16 [components, 64])."""
    d = bytes(data)
    p = parse(d)
    nc = p['components']
    coef = np.zeros((p['total_blocks'], 64), np.int16)
    qtab = np.stack([p['qt'][t] for t in p['tq']])
    hd = {k: _Huff(*v) for k, v in p['dc'].items()}
    ha = {k: _Huff(*v) for k, v in p['ac'].items()}
    br = _Bits(d, p['pos'])
    pred = [0] * nc
    mcu, rst = 0, 0
    for my in range(p['mcus_y']):
        for mx in range(p['mcus_x']):
            if p['restart'] and mcu and mcu % p['restart'] == 0:
                if br.marker() != 0xD0 + rst:
                    raise Corrupt('restart marker expected')
                rst = (rst + 1) & 7
                pred = [0] * nc
            for c, td, ta in p['scan']:
                for v in range(p['v'][c]):
                    for h in range(p['h'][c]):
                        blk = coef[p['block_offset'][c] + (my * p['v'][c] + v) * p['blocks_w'][c] + mx * p['h'][c] + h]
                        s = br.decode(hd[td])
                        if s > 15:
                            raise Corrupt('bad DC size')
                        pred[c] += _extend(br.receive(s), s)
                        if not -32768 <= pred[c] <= 32767:
                            raise Corrupt('DC out of range')
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = br.decode(ha[ta])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise Corrupt('AC run past the block')
                            blk[ZIGZAG[k]] = _extend(br.receive(s), s)
                            k += 1
            mcu += 1
    if br.marker() != 0xD9:
        raise Corrupt('EOI expected')
    return p, coef, qtab


# ---- pixels -------------------------------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(i0, i1, i2, i3, i4, i5, i6, i7):
    z1 = (i2 + i6) * 4433
    tmp2 = z1 - i6 * 15137
    tmp3 = z1 + i2 * 6270
    tmp0 = (i0 + i4) << 13
    tmp1 = (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    return [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]


def idct(blocks):
    """Dequantised int blocks [..., 8, 8] -> samples 0..255 [..., 8, 8] (jidctint.c jpeg_idct_islow)."""
    x = np.asarray(blocks, np.int64)
    ws = np.stack([_descale(o, 11) for o in _idct_1d(*[x[..., k, :] for k in range(8)])], axis=-2)        # columns
    out = np.stack([_descale(o, 18) for o in _idct_1d(*[ws[..., :, k] for k in range(8)])], axis=-1)      # rows
    return np.clip(out + 128, 0, 255)


def planes(p, coef, qtab):
    """Component planes cropped to ceil(W * h / hmax) x ceil(H * v / vmax)."""
    hmax, vmax = max(p['h']), max(p['v'])
    out = []
    for c in range(p['components']):
        bw, bh = p['blocks_w'][c], p['blocks_h'][c]
        blk = coef[p['block_offset'][c]:p['block_offset'][c] + bw * bh].astype(np.int64) * qtab[c].astype(np.int64)
        pix = idct(blk.reshape(bh, bw, 8, 8)).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)
        out.append(pix[:-(-p['height'] * p['v'][c] // vmax), :-(-p['width'] * p['h'][c] // hmax)])
    return out


def _h2v1(s):
    if s.shape[1] <= 2:
        return np.repeat(s, 2, axis=1)
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + left + 1) >> 2
    out[:, 1::2] = (3 * s + right + 2) >> 2
    return out


def _h2v2(s):
    if s.shape[1] <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    up = np.concatenate([s[:1], s[:-1]], axis=0)
    down = np.concatenate([s[1:], s[-1:]], axis=0)
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), np.int64)
    for par, nb in ((0, up), (1, down)):
        cs = 3 * s + nb
        left = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        right = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        out[par::2, 0::2] = (3 * cs + left + 8) >> 4
        out[par::2, 1::2] = (3 * cs + right + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def pixels(p, coef, qtab):
    """uint8 [H, W, C] from the hand-off format."""
    H, W = p['height'], p['width']
    pl = [x.astype(np.int64) for x in planes(p, coef, qtab)]
    if p['components'] == 1:
        return pl[0].astype(np.uint8)[:, :, None]
    up = {(1, 1): lambda s: s, (2, 1): _h2v1, (2, 2): _h2v2}[(p['h'][0], p['v'][0])]
    y, cb, cr = pl[0], up(pl[1])[:H, :W] - 128, up(pl[2])[:H, :W] - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, window=None, size=None):
    """uint8 [H, W, C]; window (y0, x0) + size (h, w) select a sub-image of the full decode."""
    p, coef, qtab = entropy_decode(data)
    img = pixels(p, coef, qtab)
    if window is not None:
        img = img[window[0]:window[0] + size[0], window[1]:window[1] + size[1]]
    return img

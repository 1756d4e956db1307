"""The CDNA / DNA pixel transformation for any kernel size, written from its definition in float64 (no oracle/ code):

    out[n, y, x, k*C + c] = sum_{u, v} kern[..., u, v, k] * img[n, m(y + u - pt, H), m(x + v - pl, W), c]

with pt = (kh - 1) // 2, pl = (kw - 1) // 2 (the SAME pad before; the rest, kh - 1 - pt, comes after) and m the single SYMMETRIC mirror
(q < 0 -> -q - 1, q >= n -> 2n - 1 - q).  A pad larger than the image has no single mirror and is refused, as tf.pad refuses it.
kern is [N, kh, kw, K] (CDNA: one kernel per sample) or [N, H, W, kh, kw, K] (DNA: one per pixel).  Plain torch ops, so autograd gives
the gradients.  tests/test_kernel_size_reference.py holds this against oracle.savp's pad2d-based statement of the same rule."""
import torch

RELU_SHIFT = 1e-12


def mirror(q, n):
    """Source index of padded coordinate q (un-padded origin) on an axis of n pixels: one reflection about the edge, edge pixel included."""
    s = -q - 1 if q < 0 else (2 * n - 1 - q if q >= n else q)
    if not 0 <= s < n:
        raise ValueError('SYMMETRIC pad larger than the image: coordinate %d on an axis of %d' % (q, n))
    return s


def pads(k):
    """(before, after) of a SAME pad at stride 1."""
    return (k - 1) // 2, k - 1 - (k - 1) // 2


def identity(kh, kw):
    """The kernel that leaves the image alone: weight 1 on the centre tap of an odd side, 0.5 / 0.5 on the two centre taps of an even one."""
    def side(k):
        f = torch.zeros(k, dtype=torch.float64)
        if k % 2:
            f[k // 2] = 1.0
        else:
            f[k // 2 - 1] = f[k // 2] = 0.5
        return f
    return side(kh)[:, None] * side(kw)[None, :]


def normalise(raw):
    """raw [..., kh, kw, K] -> relu(raw + identity - 1e-12) + 1e-12, divided by its sum over the taps."""
    kh, kw = raw.shape[-3], raw.shape[-2]
    k = torch.relu(raw + identity(kh, kw)[:, :, None] - RELU_SHIFT) + RELU_SHIFT
    return k / k.sum(dim=(-3, -2), keepdim=True)


def apply_kernels(img, kern):
    """img [N, H, W, C] float64; kern [N, kh, kw, K] or [N, H, W, kh, kw, K] -> [N, H, W, K*C] with channel k*C + c."""
    N, H, W, C = img.shape
    kh, kw, K = kern.shape[-3:]
    per_pixel = kern.dim() == 6
    pt, pl = pads(kh)[0], pads(kw)[0]
    out = torch.zeros(N, H, W, K, C, dtype=torch.float64)
    for u in range(kh):
        rows = torch.tensor([mirror(y + u - pt, H) for y in range(H)])
        for v in range(kw):
            cols = torch.tensor([mirror(x + v - pl, W) for x in range(W)])
            patch = img[:, rows][:, :, cols]                                        # [N, H, W, C]
            w = kern[:, :, :, u, v, :] if per_pixel else kern[:, u, v, :][:, None, None, :]
            out = out + w[..., :, None] * patch[..., None, :]
    return out.reshape(N, H, W, K * C)


def centre_mean(img, kh, kw):
    """What an identity kernel of an even side computes: the mean of the 2 or 4 centre taps of the mirrored image (rows y and y + 1 for an
    even kh, columns x and x + 1 for an even kw; y for an odd one)."""
    N, H, W, C = img.shape
    ys = [0] if kh % 2 else [0, 1]
    xs = [0] if kw % 2 else [0, 1]
    out = torch.zeros_like(img)
    for dy in ys:
        rows = torch.tensor([mirror(y + dy, H) for y in range(H)])
        for dx in xs:
            cols = torch.tensor([mirror(x + dx, W) for x in range(W)])
            out = out + img[:, rows][:, :, cols]
    return out / (len(ys) * len(xs))


# the shapes tests/test_gpu_kernel_sizes.py runs the HIP kernels at
# (kh, kw, K, C, N, H, W)
CDNA_CASES = [
    (3, 3, 4, 3, 2, 8, 12),
    (7, 7, 4, 3, 2, 19, 35),       # 665 pixels: three blocks and a ragged tail; 49 taps fill the accumulator array
    (7, 7, 8, 4, 1, 8, 8),         # MAXK and MAXC together
    (4, 4, 4, 3, 2, 8, 12),        # even sizes
    (2, 2, 4, 1, 2, 19, 35),
    (3, 5, 4, 3, 2, 8, 12),        # non-square; C = 2
    (4, 3, 2, 2, 2, 19, 35),
    (7, 7, 4, 3, 1, 3, 4),         # image height equal to the pad: the last legal size
    (5, 5, 4, 3, 2, 2, 5),         # H < 3 / W < 3: out of the tiled 5 x 5 kernels
    (5, 5, 4, 1, 2, 5, 2),
    (5, 5, 4, 2, 2, 8, 12),        # C of 2 and 4 at the recipe's kernel size
    (5, 5, 4, 4, 2, 8, 12),
    (1, 1, 4, 3, 2, 8, 12),        # a lone tap: kernel exactly 1, every slot the image bit for bit, draw exactly 0
]
DNA_SIZES = [(3, 3), (7, 7), (4, 4), (2, 2), (3, 5), (4, 3), (5, 5), (1, 1)]
DNA_IMAGES = [(2, 8, 12), (1, 19, 35)]

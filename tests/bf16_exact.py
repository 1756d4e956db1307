"""Bounds for the bf16 datapath (bf16 operands, fp32 accumulation) against an fp64 reference evaluated on the SAME bf16-rounded
operands the kernel multiplies.  Compared that way, the only error left is the kernel's own fp32 accumulation (~1e-6 relative),
so the bounds can be the fp32 datapath's: an intermediate rounded to bf16, a truncating conversion or a small systematic scale
on a tile fails them, where the 1e-2 rule against the unrounded operands lets all of those through.

torch only (no HIP library): the CPU self-test (tests/test_bf16_exact_reference.py) imports it too."""
import math

import torch

TOL_EXACT = 2e-5          # fp32 destination, FPROP / DGRAD and statistics epilogues (the fp32 datapath's TOL_OP)
RNE_MISMATCH = 1e-2       # bf16 destination: largest fraction of elements allowed to differ from rne(exact result)


def rel_err(got, ref):
    """max|got - ref| / max|ref| in fp64 (fp32 destinations)."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    denom = max(ref.abs().max().item(), 1e-30)
    return (got - ref).abs().max().item() / denom


def rne(t):
    """The value the bf16 datapath multiplies: fp32 -> bf16 round-to-nearest-even -> back, in t's dtype (an fp64 tensor is first
    taken to fp32, as the kernel receives it)."""
    if t.dtype == torch.bfloat16:
        return t
    return t.detach().to(torch.float32).to(torch.bfloat16).to(t.dtype)


def wgrad_tol(N, Do, Ho, Wo):
    """Weight-gradient bound: the reduction runs over every output pixel, so the accumulation error grows with sqrt of that count."""
    return TOL_EXACT * max(1.0, math.sqrt(N * Do * Ho * Wo / 65536.0))


def _key(t):
    """Integer key of bf16-representable values, monotone in the value, 0x10000 per bf16 ulp (+0 and -0 both map to 0)."""
    b = t.detach().to(torch.bfloat16).to(torch.float32).view(torch.int32).to(torch.int64)
    mag = b & 0x7fffffff
    return torch.where(b < 0, -mag, mag)


def _spacing(t):
    """bf16 spacing just above |t| (t bf16-representable)."""
    a = t.detach().to(torch.bfloat16).abs()
    up = (a.float().view(torch.int32) + 0x10000).view(torch.float32)
    return up.double() - a.double()


def window(ref):
    """Absolute half-width of the exact result's window: the fp32 accumulator a correct kernel rounds is within the fp32 datapath's
    bound (TOL_EXACT of max|ref|) of the exact result.  Far below the bf16 spacing except for elements near zero (cancellation), where
    a bracket of the exact value alone would hold the fp32 sum to a fraction of its own rounding error."""
    return TOL_EXACT * float(ref.detach().abs().max().item()) if ref.numel() else 0.0


def bf16_bracket(got, ref, atol=None):
    """bf16 destination vs the exact result `ref`: (number of elements of `got` outside the two bf16 values bracketing [ref - atol,
    ref + atol] -- must be 0 --, fraction of elements with got != rne(ref) -- at most RNE_MISMATCH: fp32 accumulation moves a sum across
    a rounding midpoint only rarely, a truncating conversion misses on about half of them).  atol defaults to window(ref); with 0 the
    window is ref itself: got must be one of the two bf16 neighbours of ref."""
    ref = ref.detach().double()
    got = got.detach().to(ref.device)
    atol = window(ref) if atol is None else atol

    def edge(v, up):                     # key of the bf16 value next to v on the side `up` (v itself if representable)
        c = v.to(torch.float32).to(torch.bfloat16)          # one of v's two bracketing values (both roundings are monotone)
        cd = c.double()
        k = _key(c)
        return k + 0x10000 * (cd < v) if up else k - 0x10000 * (cd > v)

    lo, hi, kg = edge(ref - atol, False), edge(ref + atol, True), _key(got)
    ok = (kg >= lo) & (kg <= hi) & torch.isfinite(got.float())
    n_out = float((~ok).sum().item())
    frac = float((kg != _key(ref.to(torch.float32))).double().mean().item()) if got.numel() else 0.0
    return n_out, frac


def bf16_ulps_apart(a, b):
    """Largest elementwise distance between two bf16 tensors in bf16 ulps (inf if either holds a non-finite value)."""
    if not (bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all())):
        return float('inf')
    return float(((_key(a) - _key(b.to(a.device))).abs().max().item()) / 0x10000) if a.numel() else 0.0


def bf16_apart(a, b, atol=0.0):
    """Number of elements where two bf16 results of the same exact sums are more than `atol` + 1 bf16 ulp apart (non-finite: apart).
    Two correct kernels round fp32 sums that are each within window(ref) of the exact value: atol = 2 * window(ref)."""
    b = b.to(a.device)
    ad, bd = a.double(), b.double()
    lim = atol + torch.maximum(_spacing(a), _spacing(b))
    bad = ~((ad - bd).abs() <= lim)
    return float(bad.sum().item())


def bracket_rows(tag, got, ref):
    """(name, err, tol) rows of a bf16 destination against its exact result (window(ref) wide)."""
    n_out, frac = bf16_bracket(got, ref)
    return [(tag + '_bracket', n_out, 0.0), (tag + '_rne_mismatch', frac, RNE_MISMATCH)]

"""Op-level GPU checks of the entry points that gpu_checks.py reaches only through whole-model parity: the ConvGRU gate blocks, the
sequence RNNs, the GAN / KL / TV losses, sigmoid_bwd, the robot-state recurrence, the float64 gradient fold, the ConvLSTM gate block
without a normaliser, every option of the instance norm + activation, and the fused conv + norm host calls.  Each check returns
(name, err, tol) rows in the style of gpu_checks (err = max|hip - ref| / max|ref| against the float64 references of tests/aux_refs.py,
gradients from autograd on them).  No check changes a library option."""
import numpy as np
import torch

from tests import aux_refs as R
from tests.bf16_exact import RNE_MISMATCH, bf16_bracket, bracket_rows, rel_err
from tests.gpu_checks import DEV, TOL_OP, dev, pack_wd, pack_wt, rnd
from video_prediction_amd import kernels as K
from video_prediction_amd import lib

TOL_GRAD = 1e-4


def refused(fn):
    """0.0 when the call returns SAVP_EINVAL (lib.check raises with code -1), inf when it runs or fails otherwise."""
    try:
        fn()
    except RuntimeError as e:
        return 0.0 if 'code -1' in str(e) else float('inf')
    return float('inf')


def bits_equal(a, b):
    """0.0 when the two tensors hold the same bits."""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return float('inf')
    iv = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}[a.dtype]
    return float((a.view(iv) != b.to(a.device).view(iv)).sum().item())


def untouched(t, fill):
    """Elements of the guard band t that no longer hold `fill`."""
    return float((t != fill).sum().item())


def fp32_tol(tol, e32):
    """Long recurrences: 20x the error of the same buffer (value or gradient) of the reference evaluated in fp32 on the CPU, never below
    the per-op bound."""
    return max(tol, 20.0 * e32)


# ---------------------------------------------------------------------------------------------------------------
# 1. instance norm + activation: both paths, the HW boundary, ranges, bf16 destinations, several dy, dx_beta, refusals
# ---------------------------------------------------------------------------------------------------------------
INORM_CASES = [
    # N, H, W, C, act, alpha
    (1, 7, 9, 12, 'relu', 0.0),          # single-kernel path (HW < 64), C/4 does not divide 256
    (32, 5, 7, 40, 'lrelu', 0.2),
    (2, 6, 7, 264, 'none', 0.0),         # C > 256: single-kernel path at any HW
    (1, 7, 7, 512, 'relu', 0.0),
    (32, 16, 16, 4, 'lrelu', 0.2),       # coalesced stats + apply path; N = 32 clamps the chunk at its lower end
    (1, 33, 31, 32, 'relu', 0.0),        # one plane: the chunk clamps at 256; 1023 pixels are not a whole number of chunks
    (2, 9, 9, 128, 'none', 0.0),
    (2, 64, 66, 256, 'relu', 0.0),
    (3, 7, 9, 32, 'relu', 0.0),          # HW 63 / 64 / 65
    (3, 8, 8, 32, 'lrelu', 0.2),
    (3, 5, 13, 32, 'none', 0.0),
]


def _ranges(C):
    """Disjoint (first, count) slices covering [0, C) in up to 3 pieces, multiples of 4."""
    if C < 12:
        return [(0, C)]
    a = (C // 3) // 4 * 4
    b = (2 * C // 3) // 4 * 4
    return [(0, a), (a, b - a), (b, C - b)]


def check_inorm_options(seed=101):
    out = []
    rng = np.random.default_rng(seed)
    for (N, H, W, C, act, alpha) in INORM_CASES:
        tag = 'inorm_%s_N%d_%dx%dx%d' % (act, N, H, W, C)
        x = rnd(rng, N, H, W, C) * 2 + 0.7
        x[..., 1] = 0.3 + 1e-3 * rnd(rng, N, H, W)        # std ~1e-3: eps = 1e-6 moves this channel by ~50%
        x.requires_grad_(True)
        g = (rnd(rng, C) * 0.5 + 1).requires_grad_(True)
        b = rnd(rng, C).requires_grad_(True)
        y = R.inorm_act(x, g, b, act, alpha)
        xd, gd, bd = dev(x), dev(g), dev(b)
        mean, rstd = torch.empty(N, C, device=DEV), torch.empty(N, C, device=DEV)
        # forward: a full fp32 output in a wider view, and the ranges split over fp32 / bf16 slots of a wide strided buffer (the heads)
        rgs = _ranges(C)
        full = torch.full((N, H, W, C + 8), 7.0, device=DEV)
        wide = torch.full((N, H, W, C + 16), 7.0, device=DEV)
        wide16 = torch.full((N, H, W, C + 16), 7.0, device=DEV, dtype=torch.bfloat16)
        outs, ranges, where = [full[..., 4:4 + C]], [None], []
        for k, (c0, nc) in enumerate(rgs):
            buf = wide16 if k == 1 else wide
            outs.append(buf[..., 4 + c0 + 4 * k:4 + c0 + 4 * k + nc])
            ranges.append((c0, nc))
            where.append((buf, 4 + c0 + 4 * k, c0, nc))
        K.instnorm_act_fwd(xd, gd, bd, outs, mean, rstd, act=act, alpha=alpha, out_ranges=ranges)
        out.append((tag + '/fwd', rel_err(outs[0], y), TOL_OP))
        guard_w, guard_16 = torch.ones_like(wide, dtype=torch.bool), torch.ones_like(wide16, dtype=torch.bool)
        for k, (buf, at, c0, nc) in enumerate(where):
            got = buf[..., at:at + nc]
            if buf.dtype == torch.bfloat16:
                out += bracket_rows(tag + '/fwd_range%d_bf16' % k, got, y[..., c0:c0 + nc])
                guard_16[..., at:at + nc] = False
            else:
                out.append((tag + '/fwd_range%d' % k, rel_err(got, y[..., c0:c0 + nc]), TOL_OP))
                guard_w[..., at:at + nc] = False
        full_guard = torch.ones_like(full, dtype=torch.bool)
        full_guard[..., 4:4 + C] = False
        out.append((tag + '/fwd_guard', untouched(full[full_guard], 7.0) + untouched(wide[guard_w], 7.0)
                    + untouched(wide16[guard_16].float(), 7.0), 0.0))
        # backward: up to 4 dy sources on channel ranges (one spans the others); for C >= 12 the last 4 channels have no source at all
        dys, dyr, dyref = [], [], torch.zeros(N, H, W, C, dtype=torch.float64)
        top = C - 4 if C >= 12 else C
        for (c0, nc) in [(0, top)] + [(c0, min(c0 + nc, top) - c0) for (c0, nc) in rgs]:
            if nc <= 0 or len(dys) == 4:
                continue
            d = rnd(rng, N, H, W, nc)
            dys.append(d), dyr.append((c0, nc))
            dyref[..., c0:c0 + nc] += d
        (y * dyref).sum().backward()
        dbuf = [torch.full((N, H, W, d.shape[-1] + 8), 3.0, device=DEV) for d in dys]
        dviews = [bb[..., 4:4 + d.shape[-1]] for bb, d in zip(dbuf, dys)]
        for v, d in zip(dviews, dys):
            v.copy_(d.float())
        pre = rnd(rng, N, H, W, C)
        dxb = torch.full((N, H, W, C + 8), 5.0, device=DEV)
        dx = dxb[..., 4:4 + C]
        dx.copy_(pre.float())
        dg64 = torch.zeros(C, dtype=torch.float64, device=DEV)
        db64 = torch.zeros(C, dtype=torch.float64, device=DEV)
        K.instnorm_act_bwd(xd, gd, bd, outs[0], mean, rstd, dviews, dx, dg64, db64, dx_beta=1, act=act, alpha=alpha, dy_ranges=dyr)
        out.append((tag + '/dx_beta1', rel_err(dx, pre.float().double() + x.grad), 5e-5))
        dxg = torch.ones_like(dxb, dtype=torch.bool)
        dxg[..., 4:4 + C] = False
        out.append((tag + '/dx_guard', untouched(dxb[dxg], 5.0), 0.0))
        # second call into a bf16 dx: dgamma / dbeta accumulate over the two calls
        dx16 = torch.empty(N, H, W, C, device=DEV, dtype=torch.bfloat16)
        K.instnorm_act_bwd(xd, gd, bd, outs[0], mean, rstd, dviews, dx16, dg64, db64, act=act, alpha=alpha, dy_ranges=dyr)
        # the fp32 gradient the kernel rounds is within the dx rows' 5e-5 of the exact one: bracket [ref -+ that bound]
        n_out, frac = bf16_bracket(dx16, x.grad, atol=5e-5 * float(x.grad.abs().max()))
        out += [(tag + '/dx_bf16_bracket', n_out, 0.0), (tag + '/dx_bf16_rne_mismatch', frac, RNE_MISMATCH)]
        out.append((tag + '/dgamma_2calls', rel_err(dg64, 2 * g.grad), 5e-5))
        out.append((tag + '/dbeta_2calls', rel_err(db64, 2 * b.grad), 5e-5))
        out.append((tag + '/dy_guard', sum(untouched(bb[..., :4], 3.0) + untouched(bb[..., 4 + d.shape[-1]:], 3.0)
                                           for bb, d in zip(dbuf, dys)), 0.0))
    # refusals: bf16 dx with dx_beta, ranges that are not multiples of 4
    N, H, W, C = 2, 8, 8, 32
    xd, gd, bd = dev(rnd(rng, N, H, W, C)), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    mean, rstd, o = torch.empty(N, C, device=DEV), torch.empty(N, C, device=DEV), torch.empty(N, H, W, C, device=DEV)
    K.instnorm_act_fwd(xd, gd, bd, [o], mean, rstd)
    dy = torch.ones(N, H, W, C, device=DEV)
    z = [torch.zeros(C, dtype=torch.float64, device=DEV) for _ in range(2)]
    out.append(('inorm_refuse/bf16_dx_beta', refused(lambda: K.instnorm_act_bwd(
        xd, gd, bd, o, mean, rstd, [dy], torch.empty(N, H, W, C, device=DEV, dtype=torch.bfloat16), z[0], z[1], dx_beta=1)), 0.0))
    out.append(('inorm_refuse/out_range_c0', refused(lambda: K.instnorm_act_fwd(
        xd, gd, bd, [o[..., :8]], mean, rstd, out_ranges=[(2, 8)])), 0.0))
    out.append(('inorm_refuse/out_range_nc', refused(lambda: K.instnorm_act_fwd(
        xd, gd, bd, [o[..., :6]], mean, rstd, out_ranges=[(4, 6)])), 0.0))
    out.append(('inorm_refuse/dy_range', refused(lambda: K.instnorm_act_bwd(
        xd, gd, bd, o, mean, rstd, [dy[..., :6]], torch.empty(N, H, W, C, device=DEV), z[0], z[1], dy_ranges=[(0, 6)])), 0.0))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------
# 2. ConvGRU gate blocks (gru.hip)
# ---------------------------------------------------------------------------------------------------------------
# N, H, W, F, number of outputs / dy sources; HW = 1024 (MAXPPT x NT) is the shipped 32x32 layer
GRU_BLOCK_CASES = [(1, 1, 1, 4, 1), (2, 5, 7, 8, 2), (16, 16, 16, 32, 3), (2, 1, 257, 128, 4), (1, 25, 40, 4, 1), (2, 32, 32, 32, 2)]


def check_convgru_blocks(seed=103):
    out = []
    rng = np.random.default_rng(seed)
    for (N, H, W, F, nio) in GRU_BLOCK_CASES:
        HW = H * W
        tag = 'convgru_N%d_HW%d_F%d' % (N, HW, F)
        Cx = 8
        pre_g = (rnd(rng, N, H, W, 2 * F) * 1.5 + 0.3).requires_grad_(True)
        pre_c = (rnd(rng, N, H, W, F) * 1.5 - 0.2).requires_grad_(True)
        h = rnd(rng, N, H, W, F).requires_grad_(True)
        g1, b1 = (rnd(rng, 2 * F) * 0.3 + 1).requires_grad_(True), (rnd(rng, 2 * F) * 0.3).requires_grad_(True)
        g2, b2 = (rnd(rng, F) * 0.3 + 1).requires_grad_(True), (rnd(rng, F) * 0.3).requires_grad_(True)
        u, rh = R.gru_gates(pre_g, h, g1, b1)
        hn = R.gru_out(pre_c, h, u, g2, b2)
        dys = [rnd(rng, N, H, W, F) for _ in range(nio)]
        drh = rnd(rng, N, H, W, F)
        ((hn * sum(dys)).sum() + (rh * drh).sum()).backward()
        # the candidate conv's input buffer [x | h | r*h] with a guard band; h and r*h are strided slices of it
        buf = torch.full((N, H, W, Cx + 2 * F + 4), 9.0, device=DEV)
        hv, rhv = buf[..., Cx:Cx + F], buf[..., Cx + F:Cx + 2 * F]
        hv.copy_(h.detach().float())
        pgd, pcd = dev(pre_g), dev(pre_c)
        p = [dev(t) for t in (g1, b1, g2, b2)]
        m1, r1 = torch.empty(N, 2 * F, device=DEV), torch.empty(N, 2 * F, device=DEV)
        m2, r2 = torch.empty(N, F, device=DEV), torch.empty(N, F, device=DEV)
        ud = torch.empty(N, H, W, F, device=DEV)
        K.convgru_gates_fwd(pgd, hv, p[0], p[1], m1, r1, ud, rhv)
        out.append((tag + '/u', rel_err(ud, u), TOL_OP))
        out.append((tag + '/rh', rel_err(rhv, rh), TOL_OP))
        obuf = torch.full((N, H, W, nio * (F + 4)), 9.0, device=DEV)
        outs = [obuf[..., k * (F + 4):k * (F + 4) + F] for k in range(nio)]
        K.convgru_out_fwd(pcd, hv, p[2], p[3], m2, r2, ud, outs)
        for k, o in enumerate(outs):
            out.append((tag + '/h_new%d' % k, rel_err(o, hn), TOL_OP))
        out.append((tag + '/guard', untouched(buf[..., Cx + 2 * F:], 9.0) + untouched(buf[..., :Cx], 9.0)
                    + sum(untouched(obuf[..., k * (F + 4) + F:(k + 1) * (F + 4)], 9.0) for k in range(nio)), 0.0))
        # backward: out_bwd overwrites dh (= u * dh'), gates_bwd adds d(r h) * r; dh lives in a strided slot prefilled with garbage
        dybuf = torch.zeros(N, H, W, nio * F + 4, device=DEV)
        dyv = [dybuf[..., k * F:(k + 1) * F] for k in range(nio)]
        for v, d in zip(dyv, dys):
            v.copy_(d.float())
        dhbuf = torch.full((N, H, W, F + 8), 9.0, device=DEV)
        dh = dhbuf[..., 4:4 + F]
        dh.copy_(dev(rnd(rng, N, H, W, F)))
        dpc, du = torch.empty(N, H, W, F, device=DEV), torch.empty(N, H, W, F, device=DEV)
        dpg = torch.empty(N, H, W, 2 * F, device=DEV)
        dq = [torch.zeros(c, dtype=torch.float64, device=DEV) for c in (2 * F, 2 * F, F, F)]
        K.convgru_out_bwd(pcd, hv, p[2], p[3], m2, r2, ud, dyv, dpc, du, dh, dq[2], dq[3])
        drhbuf = torch.zeros(N, H, W, F + 4, device=DEV)
        drhv = drhbuf[..., 4:]
        drhv.copy_(drh.float())
        K.convgru_gates_bwd(pgd, hv, p[0], p[1], m1, r1, du, drhv, dpg, dh, dq[0], dq[1])
        floor = float(h.grad.abs().max())      # HW = 1: the norm's input gradient is 0 exactly; measure it on the scale of dh
        out.append((tag + '/dpre_c', float((dpc.double().cpu() - pre_c.grad).abs().max()) / max(float(pre_c.grad.abs().max()),
                                                                                                   1e-6 * floor if HW == 1 else 0), TOL_GRAD))
        out.append((tag + '/dpre_g', float((dpg.double().cpu() - pre_g.grad).abs().max()) / max(float(pre_g.grad.abs().max()),
                                                                                                   1e-6 * floor if HW == 1 else 0), TOL_GRAD))
        out.append((tag + '/dh', rel_err(dh, h.grad), TOL_GRAD))
        out.append((tag + '/dh_guard', untouched(dhbuf[..., :4], 9.0) + untouched(dhbuf[..., 4 + F:], 9.0), 0.0))
        for nm, got, ref in zip(('dg1', 'db1', 'dg2', 'db2'), dq, (g1.grad, b1.grad, g2.grad, b2.grad)):
            out.append((tag + '/' + nm, rel_err(got, ref), TOL_GRAD))
    # refusals: HW above MAXPPT x NT = 1024, F not a multiple of 4
    for (HW, F, nm) in ((1025, 8, 'hw1025'), (16, 6, 'f6')):
        pre = torch.zeros(1, HW, 2 * F, device=DEV)
        hh = torch.zeros(1, HW, F, device=DEV)
        st = torch.empty(1, 2 * F, device=DEV)
        out.append(('convgru_refuse/' + nm, refused(lambda: K.convgru_gates_fwd(pre, hh, torch.ones(2 * F, device=DEV),
                                                                                torch.zeros(2 * F, device=DEV), st, st.clone(),
                                                                                torch.empty(1, HW, F, device=DEV), hh.clone())), 0.0))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------
# 3. sequence RNNs (lstm_seq, gru_seq)
# ---------------------------------------------------------------------------------------------------------------
GRU_SEQ_CASES = [
    # U, I, B, T, h0
    (1, 7, 16, 30, False), (8, 200, 16, 30, True), (8, 7, 1, 30, False), (20, 1, 16, 30, False), (33, 4096 - 33, 1, 1, True),
    (40, 7, 16, 30, True), (64, 200, 1, 30, False), (100, 1, 16, 1, True), (512, 4096 - 512, 16, 30, False),
]
LSTM_SEQ_CASES = [(16, 7, 16, 30, 1.0), (48, 1, 1, 1, 0.0), (48, 200, 16, 30, 0.0), (256, 4096 - 256, 16, 30, 1.0), (256, 7, 1, 30, 1.0)]


def _seq_weights(rng, K_, G):
    return rnd(rng, K_, G) / np.sqrt(K_) * 1.5, rnd(rng, G) * 0.3


def _gru_seq_ref(dt, xs, Wg, bg, Wc, bc, h0, dh_out):
    """gru_seq reference in dtype dt (float64: the reference; float32: the rounding a long recurrence accumulates in fp32) and the
    autograd gradients of sum(hout * dh_out) the backward kernel and the caller's GEMMs produce."""
    lv = [t_.detach().to(dt).requires_grad_(True) for t_ in (xs, Wg, bg, Wc, bc)]
    h0_ = h0.detach().to(dt).requires_grad_(True) if h0 is not None else None
    ref = R.gru_seq(*lv, h0_)
    T = xs.shape[0]
    g = torch.autograd.grad((ref['hout'] * dh_out.to(dt)).sum(), lv + ref['pg'] + ref['pc'] + ref['hin'] + ([h0_] if h0_ is not None else []))
    grads = dict(dA_x=g[0], dWg=g[1], dbg=g[2], dWc=g[3], dbc=g[4], dGg=torch.stack(g[5:5 + T]), dGc=torch.stack(g[5 + T:5 + 2 * T]),
                 dA_h=torch.stack(g[5 + 2 * T:5 + 3 * T]))
    if h0_ is not None:
        grads['dh0'] = g[-1]
    return ref, grads


def _seq_rows(out, tag, T, got, ref, ref32, tol):
    """One row per buffer.  T > 1: the bound is fp32_tol of the same buffer's fp32-CPU reference error, printed in the row name."""
    for nm, g_ in got:
        if T > 1:
            e32 = rel_err(ref32[nm], ref[nm])
            out.append(('%s/%s(fp32cpu=%.1e)' % (tag, nm, e32), rel_err(g_, ref[nm].detach()), fp32_tol(tol, e32)))
        else:
            out.append(('%s/%s' % (tag, nm), rel_err(g_, ref[nm].detach()), tol))


def check_gru_seq(seed=107):
    out = []
    rng = np.random.default_rng(seed)
    for (U, I, B, T, with_h0) in GRU_SEQ_CASES:
        tag = 'gru_seq_U%d_I%d_B%d_T%d%s' % (U, I, B, T, '_h0' if with_h0 else '')
        xs = rnd(rng, T, B, I)
        Wg, bg = _seq_weights(rng, I + U, 2 * U)
        Wc, bc = _seq_weights(rng, I + U, U)
        h0 = rnd(rng, U) * 0.5 if with_h0 else None
        dh_out = rnd(rng, T, B, U)
        ref, grads = _gru_seq_ref(torch.float64, xs, Wg, bg, Wc, bc, h0, dh_out)
        ref32, grads32 = _gru_seq_ref(torch.float32, xs, Wg, bg, Wc, bc, h0, dh_out)
        A = torch.empty(T, B, I + U, device=DEV)
        A[..., :I] = dev(xs)
        A[..., I:] = 11.0
        A2, hout = torch.empty(T, B, I + U, device=DEV), torch.empty(T, B, U, device=DEV)
        ru, cand = torch.empty(T, B, 2 * U, device=DEV), torch.empty(T, B, U, device=DEV)
        Wgd, bgd, Wcd, bcd = dev(Wg), dev(bg), dev(Wc), dev(bc)
        K.gru_seq_fwd(A, A2, Wgd, bgd, Wcd, bcd, hout, ru, cand, I, h0=dev(h0) if with_h0 else None)
        _seq_rows(out, tag, T, (('A', A), ('A2', A2), ('ru', ru), ('cand', cand), ('hout', hout)), ref, ref32, TOL_OP)
        dGg, dGc, dA = torch.empty(T, B, 2 * U, device=DEV), torch.empty(T, B, U, device=DEV), torch.empty(T, B, I + U, device=DEV)
        dh0 = torch.zeros(U, dtype=torch.float64, device=DEV) if with_h0 else None
        for _ in range(2 if with_h0 else 1):     # dh0 accumulates over calls
            K.gru_seq_bwd(A, Wgd, Wcd, ru, cand, dev(dh_out), dGg, dGc, dA, I, dh0=dh0)
        # the caller's weight-gradient GEMMs in fp64 from the kernel's buffers
        Ac, A2c, dGgc, dGcc = (t_.double().cpu().reshape(T * B, -1) for t_ in (A, A2, dGg, dGc))
        got = [('dGg', dGg), ('dGc', dGc), ('dA_x', dA[..., :I]), ('dA_h', dA[..., I:]), ('dWg', Ac.t() @ dGgc), ('dbg', dGgc.sum(0)),
               ('dWc', A2c.t() @ dGcc), ('dbc', dGcc.sum(0))]
        if with_h0:
            got.append(('dh0', dh0 / 2))          # two calls: twice the gradient
        _seq_rows(out, tag, T, got, grads, grads32, TOL_GRAD)
    # refusals at the documented bounds (1 <= U <= 512, I >= 1, I + U <= 4096)
    for (U, I, nm) in ((0, 4, 'U0'), (513, 4, 'U513'), (8, 0, 'I0'), (8, 4089, 'IU4097')):
        Uq, Iq = max(U, 1), max(I, 1)
        A = torch.zeros(1, 1, Iq + Uq + (1 if I == 0 else 0), device=DEV)
        W = torch.zeros(max(I + U, 1), 2 * Uq, device=DEV)
        v = torch.zeros(1, 1, 2 * Uq, device=DEV)
        out.append(('gru_seq_refuse/' + nm, refused(lambda: lib.check(lib.get().savp_gru_seq_fwd(
            lib.stream(), K._p(A), K._p(A), K._p(W), K._p(v), K._p(W), K._p(v), K._p(v), K._p(v), K._p(v), 1, 1, I, U),
            'savp_gru_seq_fwd')), 0.0))
        out.append(('gru_seq_refuse/bwd_' + nm, refused(lambda: lib.check(lib.get().savp_gru_seq_bwd(
            lib.stream(), K._p(A), K._p(W), K._p(W), K._p(v), K._p(v), K._p(v), K._p(v), K._p(v), K._p(A), 1, 1, I, U),
            'savp_gru_seq_bwd')), 0.0))
    torch.cuda.synchronize()
    return out


def _lstm_seq_ref(dt, xs, W, b, fb, dh_out):
    lv = [t_.detach().to(dt).requires_grad_(True) for t_ in (xs, W, b)]
    ref = R.lstm_seq(*lv, fb)
    T = xs.shape[0]
    g = torch.autograd.grad((ref['hout'] * dh_out.to(dt)).sum(), lv + ref['g'] + ref['hin'])
    return ref, dict(dA_x=g[0], dW=g[1], db=g[2], dG=torch.stack(g[3:3 + T]), dA_h=torch.stack(g[3 + T:]))


def check_lstm_seq(seed=109):
    out = []
    rng = np.random.default_rng(seed)
    for (U, I, B, T, fb) in LSTM_SEQ_CASES:
        tag = 'lstm_seq_U%d_I%d_B%d_T%d_fb%g' % (U, I, B, T, fb)
        xs = rnd(rng, T, B, I)
        W, b = _seq_weights(rng, I + U, 4 * U)
        dh_out = rnd(rng, T, B, U)
        ref, grads = _lstm_seq_ref(torch.float64, xs, W, b, fb, dh_out)
        ref32, grads32 = _lstm_seq_ref(torch.float32, xs, W, b, fb, dh_out)
        A = torch.empty(T, B, I + U, device=DEV)
        A[..., :I] = dev(xs)
        A[..., I:] = 11.0
        hout, gates, cs = torch.empty(T, B, U, device=DEV), torch.empty(T, B, 4 * U, device=DEV), torch.empty(T, B, U, device=DEV)
        Wd = dev(W)
        K.lstm_seq_fwd(A, Wd, dev(b), hout, gates, cs, I, forget_bias=fb)
        _seq_rows(out, tag, T, (('A', A), ('gates', gates), ('cs', cs), ('hout', hout)), ref, ref32, TOL_OP)
        dG, dA = torch.empty(T, B, 4 * U, device=DEV), torch.empty(T, B, I + U, device=DEV)
        K.lstm_seq_bwd(A, Wd, gates, cs, dev(dh_out), dG, dA, I, forget_bias=fb)
        Ac, dGc = A.double().cpu().reshape(T * B, -1), dG.double().cpu().reshape(T * B, -1)
        _seq_rows(out, tag, T, (('dG', dG), ('dA_x', dA[..., :I]), ('dA_h', dA[..., I:]), ('dW', Ac.t() @ dGc), ('db', dGc.sum(0))),
                  grads, grads32, TOL_GRAD)
    # refusals: 16 <= U <= 256, U % 16 == 0, I >= 1, I + U <= 4096
    for (U, I, nm) in ((8, 4, 'U8'), (24, 4, 'U24'), (272, 4, 'U272'), (32, 0, 'I0'), (32, 4065, 'IU4097')):
        A = torch.zeros(1, 1, max(I, 1) + U, device=DEV)
        W = torch.zeros(max(I, 1) + U, 4 * U, device=DEV)
        v = torch.zeros(1, 1, 4 * U, device=DEV)
        out.append(('lstm_seq_refuse/' + nm, refused(lambda: lib.check(lib.get().savp_lstm_seq_fwd(
            lib.stream(), K._p(A), K._p(W), K._p(v), K._p(v), K._p(v), K._p(v), 1, 1, I, U, 1.0), 'savp_lstm_seq_fwd')), 0.0))
        out.append(('lstm_seq_refuse/bwd_' + nm, refused(lambda: lib.check(lib.get().savp_lstm_seq_bwd(
            lib.stream(), K._p(A), K._p(W), K._p(v), K._p(v), K._p(v), K._p(v), K._p(A), 1, 1, I, U, 1.0), 'savp_lstm_seq_bwd')), 0.0))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------
# 4. losses: GAN / SNGAN, KL between two Gaussians, TV of the flows, sigmoid_bwd
# ---------------------------------------------------------------------------------------------------------------
def check_losses(seed=113):
    out = []
    rng = np.random.default_rng(seed)
    for n in (1, 255, 256, 257, 10000):
        base = rnd(rng, n) * 3
        base[:4] = torch.tensor([30.0, -30.0, 90.0, -90.0], dtype=torch.float64)[:n]
        for typ in ('GAN', 'SNGAN'):
            for label in (0.0, 1.0):
                for beta in (0, 1):
                    tag = 'gan_%s_n%d_l%g_b%d' % (typ, n, label, beta)
                    lg = base.clone().requires_grad_(True)
                    loss = R.gan_loss(lg, label, typ)
                    loss.backward()
                    w = 0.7
                    pre = rnd(rng, n)
                    dl = dev(pre)
                    lo = torch.zeros(1, dtype=torch.float64, device=DEV)
                    K.gan_loss(dev(lg), label, w, typ, loss_out=lo, dlogits=dl, beta=beta)
                    out.append((tag + '/loss', rel_err(lo, loss.detach().reshape(1)), TOL_OP))
                    out.append((tag + '/dlogits', rel_err(dl, w * lg.grad + (pre.float().double() if beta else 0)), 5e-5))
    x = dev(rnd(rng, 16))
    for typ in ('GAN', 'SNGAN'):
        out.append(('gan_refuse/%s_label0.5' % typ, refused(lambda: K.gan_loss(x, 0.5, 1.0, typ, dlogits=torch.empty_like(x))), 0.0))
    # KL: clip boundaries exactly at +-10 and beyond, |l1 - l2| on both sides of the 0.5 series switch, klw host / device,
    # gradients added into prefilled tensors, n > 1024 * 256 (grid-stride loop)
    for (rows, nz, klw_on_dev) in ((4, 16, False), (300, 1000, True), (7, 33, True)):
        tag = 'kl_gauss_%dx%d%s' % (rows, nz, '_klwdev' if klw_on_dev else '')
        mu1, mu2 = rnd(rng, rows, nz), rnd(rng, rows, nz)
        ls1 = rnd(rng, rows, nz) * 2
        ls2 = ls1 + torch.tensor(rng.choice([0.49, -0.49, 0.51, -0.51, 1e-3, -2e-3, 3.0], size=(rows, nz)))
        special = torch.tensor([10.0, -10.0, 10.5, -12.0, 9.75, -10.0, 10.0, 11.0])
        k = min(special.numel(), nz)
        ls1[0, :k] = special[:k].double()
        ls2[0, :k] = special.flip(0)[:k].double()
        if rows > 1:
            ls1[1, :k], ls2[1, :k] = special[:k].double(), special[:k].double()
        ls1 = ls1.float().double()
        ls2 = ls2.float().double()                    # the kernel's inputs, exactly: the boundary values stay exact
        leaves = [t_.clone().requires_grad_(True) for t_ in (mu1, ls1, mu2, ls2)]
        kl = R.kl_gauss(*leaves)
        kl.backward()
        klw = 0.37
        pre = [rnd(rng, rows, nz) for _ in range(4)]
        gds = [dev(p_) for p_ in pre]
        lo = torch.zeros(1, dtype=torch.float64, device=DEV)
        kwd = dict(klw_dev=torch.tensor([klw], device=DEV), klw=123.0) if klw_on_dev else dict(klw=klw)
        K.kl_gauss(*[dev(t_) for t_ in (mu1, ls1, mu2, ls2)], kl_out=lo, grads=gds, **kwd)
        out.append((tag + '/kl', rel_err(lo, kl.detach().reshape(1)), TOL_OP))
        for nm, got, p_, lf in zip(('dmu1', 'dls1', 'dmu2', 'dls2'), gds, pre, leaves):
            out.append((tag + '/' + nm, rel_err(got, p_.float().double() + klw * lf.grad), 5e-5))
    # TV of the flows: strided views, n_channels below the view's channel count, H or W = 2, dflows accumulated
    for (n, H, W, Cv, nch) in ((3, 2, 9, 8, 6), (2, 7, 2, 4, 4), (4, 16, 24, 8, 2), (2, 33, 31, 12, 8)):
        tag = 'tv_n%d_%dx%d_c%d_of%d' % (n, H, W, nch, Cv)
        f = rnd(rng, n, H, W, Cv).requires_grad_(True)
        s1, s2, w = 1.0 / (n * (H - 1) * W), 1.0 / (n * H * (W - 1)), 0.3
        loss = R.tv_loss(f, nch, s1, s2)
        loss.backward()
        fb = torch.full((n, H, W, Cv + 6), 4.0, device=DEV)
        fv = fb[..., 3:3 + Cv]
        fv.copy_(f.detach().float())
        pre = rnd(rng, n, H, W, Cv)
        db = torch.full((n, H, W, Cv + 6), 4.0, device=DEV)
        dv = db[..., 3:3 + Cv]
        dv.copy_(pre.float())
        lo = torch.zeros(1, dtype=torch.float64, device=DEV)
        K.tv_loss(fv, nch, s1, s2, w, loss_out=lo, dflows=dv)
        out.append((tag + '/loss', rel_err(lo, loss.detach().reshape(1)), TOL_OP))
        out.append((tag + '/dflows', rel_err(dv[..., :nch], pre[..., :nch].float().double() + w * f.grad[..., :nch]), 5e-5))
        out.append((tag + '/extra_channels', bits_equal(dv[..., nch:], pre[..., nch:].float().to(DEV)), 0.0))
        out.append((tag + '/guard', untouched(db[..., :3], 4.0) + untouched(db[..., 3 + Cv:], 4.0), 0.0))
    # sigmoid_bwd on strided views
    for (N, H, W, C) in ((2, 5, 7, 3), (3, 16, 16, 12)):
        yb, dyb = torch.rand(N, H, W, C + 5, device=DEV), torch.randn(N, H, W, C + 2, device=DEV)
        y, dy = yb[..., 5:], dyb[..., 1:1 + C]
        o = torch.empty(N, H, W, C, device=DEV)
        K.sigmoid_bwd(dy, y, o)
        yd = y.double().cpu()
        out.append(('sigmoid_bwd_%dx%dx%dx%d' % (N, H, W, C), rel_err(o, dy.double().cpu() * yd * (1 - yd)), TOL_OP))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------
# 5. robot-state recurrence and the float64 gradient fold
# ---------------------------------------------------------------------------------------------------------------
def check_state_pred_and_fold(seed=127):
    out = []
    rng = np.random.default_rng(seed)
    for (T, N, na, ns) in ((8, 5, 4, 3), (1, 3, 0, 5), (10, 16, 12, 20), (12, 2, 0, 32)):
        tag = 'state_pred_T%d_N%d_na%d_ns%d' % (T, N, na, ns)
        acts = rnd(rng, T, N, na) if na else None
        sts = rnd(rng, T, N, ns)
        gt = torch.tensor(rng.integers(0, 2, size=(T, N)), dtype=torch.int32)
        W = (rnd(rng, na + ns, ns) / np.sqrt(na + ns)).requires_grad_(True)
        b = (rnd(rng, ns) * 0.2).requires_grad_(True)
        sa, gen, gens = R.state_pred(acts, sts, gt, W, b)
        dgen = rnd(rng, T, N, ns)
        grads = torch.autograd.grad((gen * dgen).sum(), [W, b] + gens)
        sad, gend = torch.empty(T, N, na + ns, device=DEV), torch.empty(T, N, ns, device=DEV)
        gtd = gt.to(DEV)
        Wd = dev(W)
        K.state_pred_fwd(dev(acts) if na else None, dev(sts), gtd, Wd, dev(b), sad, gend)
        out.append((tag + '/sa', rel_err(sad, sa.detach()), TOL_OP))
        out.append((tag + '/gen', rel_err(gend, gen.detach()), TOL_OP))
        dg = dev(dgen)
        dW64 = torch.zeros(na + ns, ns, dtype=torch.float64, device=DEV)
        db64 = torch.zeros(ns, dtype=torch.float64, device=DEV)
        K.state_pred_bwd(gtd, Wd, sad, dg, dW64, db64)
        out.append((tag + '/dgen_total', rel_err(dg, torch.stack(grads[2:])), 5e-5))
        out.append((tag + '/dW', rel_err(dW64, grads[0]), 5e-5))
        out.append((tag + '/db', rel_err(db64, grads[1]), 5e-5))
    # fold64: all elements, then a permuted subset; zero accumulators leave dst's bits alone (-0.0, a NaN payload), a repeat adds nothing
    n = 5000
    src = torch.tensor(rng.standard_normal(n) * 1e-3, dtype=torch.float64)
    src[::7] = 0.0
    dst = torch.tensor(rng.standard_normal(n), dtype=torch.float32)
    dst[::14] = -0.0
    dst[7::14] = torch.tensor([0x7fc01234], dtype=torch.int32).view(torch.float32)
    for mode in ('all', 'subset'):
        s_d, d_d = src.to(DEV), dst.to(DEV)
        if mode == 'all':
            idx, listed = None, torch.ones(n, dtype=torch.bool)
        else:
            perm = torch.tensor(rng.permutation(n)[:n // 3], dtype=torch.int64)
            idx, listed = perm.to(torch.int32).to(DEV), torch.zeros(n, dtype=torch.bool)
            listed[perm] = True
        K.fold64(s_d, d_d, idx)
        exp_d = dst.clone()
        nz = listed & (src != 0)
        exp_d[nz] = dst[nz] + src[nz].float()
        exp_s = src.clone()
        exp_s[listed] = 0.0
        out.append(('fold64_%s/dst' % mode, bits_equal(d_d.cpu(), exp_d), 0.0))
        out.append(('fold64_%s/src' % mode, bits_equal(s_d.cpu(), exp_s), 0.0))
        K.fold64(s_d, d_d, idx)
        out.append(('fold64_%s/repeat_adds_nothing' % mode, bits_equal(d_d.cpu(), exp_d), 0.0))
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------
# 6. ConvLSTM gate block without a normaliser (lstm_plain_{fwd,bwd}_kernel)
# ---------------------------------------------------------------------------------------------------------------
def check_lstm_no_norm(seed=131):
    out = []
    rng = np.random.default_rng(seed)
    # N * HW * F / 4 = 1 081 344 > 4096 * 256 in the last case: the grid-stride loop runs
    for (N, H, W, F, zero_c, ndh, fb) in ((2, 8, 8, 16, True, 3, 1.0), (3, 5, 7, 8, False, 1, 0.0), (33, 32, 32, 128, False, 2, 1.0)):
        tag = 'lstm_nonorm_N%d_%dx%dx%d%s' % (N, H, W, F, '_zero' if zero_c else '')
        gates = (rnd(rng, N, H, W, 4 * F) * 1.5).requires_grad_(True)
        c = (torch.zeros(N, H, W, F, dtype=torch.float64) if zero_c else rnd(rng, N, H, W, F)).requires_grad_(True)
        cn, hn = R.lstm_plain(gates, c, fb)
        dhs = [rnd(rng, N, H, W, F) for _ in range(ndh)]
        (hn * sum(dhs)).sum().backward()
        gd = dev(gates)
        cbuf = torch.full((N, H, W, F + 4), 6.0, device=DEV)
        cv = cbuf[..., 4:]
        if not zero_c:
            cv.copy_(c.detach().float())
        c_new = torch.empty(N, H, W, F, device=DEV)
        hbuf = torch.full((N, H, W, 2 * F + 4), 6.0, device=DEV)
        hs = [hbuf[..., :F], hbuf[..., F + 4:]]
        K.convlstm_gates_fwd(gd, None if zero_c else cv, None, None, None, None, c_new, hs, None, forget_bias=fb)
        out.append((tag + '/c', rel_err(c_new, cn), TOL_OP))
        out.append((tag + '/h', max(rel_err(hs[0], hn), rel_err(hs[1], hn)), TOL_OP))
        out.append((tag + '/guard', untouched(hbuf[..., F:F + 4], 6.0), 0.0))
        dgates = torch.empty(N, H, W, 4 * F, device=DEV)
        dcp = None if zero_c else torch.empty(N, H, W, F, device=DEV)
        K.convlstm_gates_bwd(gd, None if zero_c else cv, None, None, None, None, None, [dev(d) for d in dhs], None, dgates, dcp, None,
                             forget_bias=fb)
        out.append((tag + '/dgates', rel_err(dgates, gates.grad), TOL_GRAD))
        if not zero_c:
            out.append((tag + '/dc_prev', rel_err(dcp, c.grad), TOL_GRAD))
        del gates, c, cn, hn, dhs
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------
# 7. fused host calls: one call == the two separate calls, bit for bit; every refusal returns SAVP_EINVAL
# ---------------------------------------------------------------------------------------------------------------
def _inorm_fused_case(rng, bf16):
    """An encoder ladder layer of the cell as the bf16 step runs it (savp_cell.py:197-224): conv_pool 4x4 / stride 2 from 32 to 64
    channels, 32x32 -> 16x16, instance norm + ReLU.  bf16: bf16 conv source and norm output, fp32 pre-activation, bf16 pre-activation
    gradient read by the data gradient into the fp32 input gradient (Act keeps fp32 gradients unless asked otherwise); the conv takes
    bf16 weight copies (w16) as ConvLayer does."""
    N, H, W, Cx, Cy = 4, 32, 32, 32, 64
    geom = K.ConvGeom((4, 4), (2, 2), (1, 1))
    x = dev(rnd(rng, N, H, W, Cx))
    if bf16:
        x = x.to(torch.bfloat16)
    w = rnd(rng, 4, 4, Cx, Cy) * 0.1
    wt, wd = dev(pack_wt(w)), dev(pack_wd(w))
    g, b = dev(rnd(rng, Cy) * 0.3 + 1), dev(rnd(rng, Cy) * 0.3)
    return N, H, W, Cx, Cy, geom, x, wt, wd, g, b


def check_fused_calls(seed=137):
    out = []
    rng = np.random.default_rng(seed)
    for bf16 in (False, True):
        tag = 'fused_conv_in_act_%s' % ('bf16' if bf16 else 'fp32')
        N, H, W, Cx, Cy, geom, x, wt, wd, g, b = _inorm_fused_case(rng, bf16)
        Ho, Wo = H // 2, W // 2
        adt = torch.bfloat16 if bf16 else torch.float32
        fw = dict(precision=1, w16=wt.to(torch.bfloat16)) if bf16 else {}
        bw = dict(precision=1, w16=wd.to(torch.bfloat16)) if bf16 else {}
        dy = dev(rnd(rng, N, Ho, Wo, Cy))
        res = []
        for fused in (False, True):
            pre = torch.empty(N, Ho, Wo, Cy, device=DEV)
            o = torch.empty(N, Ho, Wo, Cy, device=DEV, dtype=adt)
            mean, rstd = torch.empty(N, Cy, device=DEV), torch.empty(N, Cy, device=DEV)
            if fused:
                K.conv_in_act_fwd(K.conv(lib.CONV_FPROP, geom, x, pre, wt, defer=True, **fw),
                                  K.instnorm_act_fwd(pre, g, b, [o], mean, rstd, defer=True))
            else:
                K.conv(lib.CONV_FPROP, geom, x, pre, wt, **fw)
                K.instnorm_act_fwd(pre, g, b, [o], mean, rstd)
            dpre = torch.empty(N, Ho, Wo, Cy, device=DEV, dtype=adt)
            dx = torch.empty(N, H, W, Cx, device=DEV)
            dgb = [torch.zeros(Cy, dtype=torch.float64, device=DEV) for _ in range(2)]
            if fused:
                K.conv_in_act_bwd(K.conv(lib.CONV_DGRAD, geom, dx, dpre, wd, defer=True, **bw),
                                  K.instnorm_act_bwd(pre, g, b, o, mean, rstd, [dy], dpre, dgb[0], dgb[1], defer=True))
            else:
                K.instnorm_act_bwd(pre, g, b, o, mean, rstd, [dy], dpre, dgb[0], dgb[1])
                K.conv(lib.CONV_DGRAD, geom, dx, dpre, wd, **bw)
            res.append((pre, o, mean, rstd, dpre, dx, dgb[0], dgb[1]))
        for nm, a_, b_ in zip(('pre', 'out', 'mean', 'rstd', 'dpre', 'dx', 'dgamma', 'dbeta'), res[0], res[1]):
            out.append((tag + '/' + nm + '_bitwise', bits_equal(a_, b_), 0.0))
    # savp_convlstm_cell_bwd on the path of the bf16 step (savp_cell.py:915-930): normalised gates, coalesced kernels (ws), bf16 gate
    # gradient through its fp32 scratch, the gate convolution's bf16-operand DGRAD into the fp32 [x | h] gradient
    N, H, W, F, Cin = 2, 32, 32, 32, 64
    geom5 = K.ConvGeom((5, 5), (1, 1), (2, 2))
    gates, c = dev(rnd(rng, N, H, W, 4 * F) * 1.5), dev(rnd(rng, N, H, W, F))
    p = [dev(rnd(rng, 4 * F) * 0.3 + 1), dev(rnd(rng, 4 * F) * 0.3), dev(rnd(rng, F) * 0.3 + 1), dev(rnd(rng, F) * 0.3)]
    stats = [torch.empty(N, 4 * F, device=DEV), torch.empty(N, 4 * F, device=DEV), torch.empty(N, F, device=DEV), torch.empty(N, F, device=DEV)]
    ws = torch.empty(K.lstm_ws_floats(N, H * W, F), device=DEV)
    K.convlstm_gates_fwd(gates, c, p[0], p[1], p[2], p[3], torch.empty(N, H, W, F, device=DEV), [torch.empty(N, H, W, F, device=DEV)],
                         stats, ws=ws)
    wl = dev(pack_wd(rnd(rng, 5, 5, Cin, 4 * F) * 0.05))
    wl16 = wl.to(torch.bfloat16)
    dh, dcn = dev(rnd(rng, N, H, W, F)), dev(rnd(rng, N, H, W, F))
    res = []
    for fused in (False, True):
        dg = torch.empty(N, H, W, 4 * F, device=DEV, dtype=torch.bfloat16)
        raw = torch.empty(N, H, W, 4 * F, device=DEV)
        dcp = torch.empty(N, H, W, F, device=DEV)
        dpar = [torch.zeros(n_, dtype=torch.float64, device=DEV) for n_ in (4 * F, 4 * F, F, F)]
        da = torch.empty(N, H, W, Cin, device=DEV)
        bargs = (gates, c, p[0], p[1], p[2], p[3], stats, [dh], dcn, dg, dcp, dpar)
        if fused:
            K.convlstm_cell_bwd(K.conv(lib.CONV_DGRAD, geom5, da, dg, wl, precision=1, w16=wl16, defer=True),
                                K.convlstm_gates_bwd(*bargs, ws=ws, dgates_raw=raw, defer=True))
        else:
            K.convlstm_gates_bwd(*bargs, ws=ws, dgates_raw=raw)
            K.conv(lib.CONV_DGRAD, geom5, da, dg, wl, precision=1, w16=wl16)
        res.append([dg, dcp] + dpar + [da])
    for nm, a_, b_ in zip(('dgates', 'dc_prev', 'dg1', 'db1', 'dg2', 'db2', 'dx'), res[0], res[1]):
        out.append(('fused_convlstm_cell_bwd_bf16/' + nm + '_bitwise', bits_equal(a_, b_), 0.0))
    # refusals (fused_ops.hip): each inconsistency between the two halves returns SAVP_EINVAL
    N, H, W, Cx, Cy, geom, x, wt, wd, g, b = _inorm_fused_case(rng, False)
    Ho, Wo = H // 2, W // 2                # the conv's output plane
    pre, other = torch.empty(N, Ho, Wo, Cy, device=DEV), torch.empty(N, Ho, Wo, Cy, device=DEV)
    o = torch.empty(N, Ho, Wo, Cy, device=DEV)
    mean, rstd = torch.empty(N, Cy, device=DEV), torch.empty(N, Cy, device=DEV)
    dx, dpre = torch.empty(N, H, W, Cx, device=DEV), torch.empty(N, Ho, Wo, Cy, device=DEV)
    dgb = [torch.zeros(Cy, dtype=torch.float64, device=DEV) for _ in range(2)]

    def fwd(mod):
        ca = K.conv(lib.CONV_FPROP, geom, x, pre, wt, defer=True)
        na = K.instnorm_act_fwd(pre, g, b, [o], mean, rstd, defer=True)
        mod(ca, na)
        return lambda: K.conv_in_act_fwd(ca, na)

    def bwd(mod):
        ca = K.conv(lib.CONV_DGRAD, geom, dx, dpre, wd, defer=True)
        na = K.instnorm_act_bwd(pre, g, b, o, mean, rstd, [other], dpre, dgb[0], dgb[1], defer=True)
        mod(ca, na)
        return lambda: K.conv_in_act_bwd(ca, na)

    st = K.stats_ws(torch.device(DEV), N, Cy)

    def set_(obj, **kw):
        for k_, v_ in kw.items():
            setattr(obj, k_, v_)

    cases = [
        ('fwd_mode', fwd(lambda c, n: set_(c, mode=lib.CONV_WGRAD))),
        ('fwd_dst', fwd(lambda c, n: set_(n.x, p=other.data_ptr()))),
        ('fwd_channels', fwd(lambda c, n: set_(n, C=Cy - 4))),
        ('fwd_batch', fwd(lambda c, n: set_(n, N=N - 1))),
        ('fwd_stats_one_side', fwd(lambda c, n: set_(c, stats=st.data_ptr()))),
        ('fwd_stats_other_ws', fwd(lambda c, n: (set_(c, stats=st.data_ptr()), set_(n, stats_ready=1, ws=other.data_ptr())))),
        ('bwd_mode', bwd(lambda c, n: set_(c, mode=lib.CONV_WGRAD))),
        ('bwd_src', bwd(lambda c, n: set_(n.dx, p=other.data_ptr()))),
        ('bwd_bf16', bwd(lambda c, n: set_(n, dx_bf16=1))),
        ('bwd_batch', bwd(lambda c, n: set_(n, N=N - 1))),
    ]
    # savp_convlstm_cell_bwd: gate block without a normaliser + the gate convolution's DGRAD
    F = 16
    geom3 = K.ConvGeom((3, 3), (1, 1), (1, 1))
    gates = torch.zeros(N, Ho, Wo, 4 * F, device=DEV)
    dg = torch.empty(N, Ho, Wo, 4 * F, device=DEV)
    dxl = torch.empty(N, Ho, Wo, Cx, device=DEV)
    wl = dev(pack_wd(rnd(rng, 3, 3, Cx, 4 * F) * 0.1))
    dh = torch.zeros(N, Ho, Wo, F, device=DEV)

    def cell_bwd(mod):
        ca = K.conv(lib.CONV_DGRAD, geom3, dxl, dg, wl, defer=True)
        la = K.convlstm_gates_bwd(gates, None, None, None, None, None, None, [dh], None, dg, None, None, defer=True)
        mod(ca, la)
        return lambda: K.convlstm_cell_bwd(ca, la)

    cases += [
        ('cell_bwd_mode', cell_bwd(lambda c, l: set_(c, mode=lib.CONV_FPROP))),
        ('cell_bwd_dgates', cell_bwd(lambda c, l: set_(l, dgates=other.data_ptr()))),
        ('cell_bwd_bf16', cell_bwd(lambda c, l: set_(l, dgates_bf16=1))),
        ('cell_bwd_channels', cell_bwd(lambda c, l: set_(l, F=F + 4))),
        ('cell_bwd_batch', cell_bwd(lambda c, l: set_(l, N=N + 1))),
    ]
    for nm, call in cases:
        out.append(('fused_refuse/' + nm, refused(call), 0.0))
    torch.cuda.synchronize()
    return out


ALL_AUX_CHECKS = [('inorm_options', check_inorm_options), ('convgru_blocks', check_convgru_blocks), ('gru_seq', check_gru_seq),
                  ('lstm_seq', check_lstm_seq), ('losses', check_losses), ('state_pred_fold', check_state_pred_and_fold),
                  ('lstm_no_norm', check_lstm_no_norm), ('fused_calls', check_fused_calls)]

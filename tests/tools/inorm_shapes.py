"""Per-shape time of the instance-norm kernels inside the train step.  A kernel trace carries grid sizes but no arguments, and several
shapes of the step share one grid, so the split is taken from the call ORDER: `run` logs every K.instnorm_act_fwd / _bwd call of a bench.py
run (shape, views, dtypes), `table` predicts each call's launches from the library's dispatch rules and joins them, in order, with the
`inorm` rows of the rocprofv3 kernel trace of that same run.

usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tests/tools/inorm_shapes.py run CALLS.json <bench.py arguments>
       python tests/tools/inorm_shapes.py table CALLS.json <..._kernel_trace.csv> STEPS      (markdown on stdout)"""
import atexit, csv, json, os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _views(ts, ranges, C):
    out = []
    for i, t in enumerate(ts):
        r = (ranges or ())[i] if i < len(ranges or ()) else None
        out.append([int(r[1]) if r and r[1] else C, 2 if str(t.dtype).endswith('bfloat16') else 4])
    return out


def run(log, argv):
    from video_prediction_amd import kernels as K
    calls = []
    fwd0, bwd0 = K.instnorm_act_fwd, K.instnorm_act_bwd

    def fwd(x, gamma, beta, outs, mean, rstd, act='relu', alpha=0.0, eps=1e-6, out_ranges=None, stats=None, **kw):
        C = x.shape[-1]
        calls.append(dict(dir='fwd', N=x.shape[0], HW=x.numel() // (x.shape[0] * C), C=C, act=act, views=_views(outs, out_ranges, C),
                          ready=stats is not None))
        return fwd0(x, gamma, beta, outs, mean, rstd, act=act, alpha=alpha, eps=eps, out_ranges=out_ranges, stats=stats, **kw)

    def bwd(x, gamma, beta, out0, mean, rstd, dys, dx, dgamma, dbeta, dx_beta=0, act='relu', alpha=0.0, eps=1e-6, dy_ranges=None, stats=None, **kw):
        C = x.shape[-1]
        calls.append(dict(dir='bwd', N=x.shape[0], HW=x.numel() // (x.shape[0] * C), C=C, act=act, views=_views(dys, dy_ranges, C),
                          ready=stats is not None, dx=[2 if str(dx.dtype).endswith('bfloat16') else 4, int(dx_beta)]))
        return bwd0(x, gamma, beta, out0, mean, rstd, dys, dx, dgamma, dbeta, dx_beta=dx_beta, act=act, alpha=alpha, eps=eps,
                    dy_ranges=dy_ranges, stats=stats, **kw)

    K.instnorm_act_fwd, K.instnorm_act_bwd = fwd, bwd
    atexit.register(lambda: json.dump(calls, open(log, 'w')))
    sys.argv = [os.path.join(ROOT, 'bench.py')] + argv
    runpy.run_path(sys.argv[0], run_name='__main__')


def kind(name):
    for key, k in (('bwd_stats', 'bwd_stats'), ('bwd_apply', 'bwd_apply'), ('inorm_bwd_kernel', 'bwd_one'), ('inorm_stats', 'stats'),
                   ('inorm_apply', 'apply'), ('inorm_fwd_kernel', 'fwd_one')):
        if key in name:
            return k
    return None


def launches(c, min_hw=64):
    """savp_instnorm_act_fwd / _bwd: the kernels one call launches, with the bytes each has to move."""
    n = c['N'] * c['HW']
    x = n * c['C'] * 4
    views = sum(n * nc * b for nc, b in c['views'])
    coalesced = c['C'] % 4 == 0 and c['C'] <= 256 and 256 % (c['C'] // 4) == 0
    if c['dir'] == 'fwd':
        if c['ready'] or (coalesced and c['HW'] >= min_hw):
            return ([] if c['ready'] else [('stats', x)]) + [('apply', x + views)]
        return [('fwd_one', 3 * x + views)]
    dx = n * c['C'] * c['dx'][0] * (2 if c['dx'][1] else 1)
    if c['ready'] or (coalesced and c['HW'] >= min_hw):
        return ([] if c['ready'] else [('bwd_stats', x + views)]) + [('bwd_apply', x + views + dx)]
    return [('bwd_one', 2 * (x + views) + dx)]


def table(log, trace, steps):
    calls = json.load(open(log))
    rows = [r for r in csv.DictReader(open(trace)) if kind(r['Kernel_Name'])]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    agg, i, skipped = {}, 0, 0
    for c in calls:
        for k, nbytes in launches(c):
            while i < len(rows) and kind(rows[i]['Kernel_Name']) != k:      # e.g. the ConvLSTM block's own inorm_stats_kernel launches
                i += 1
                skipped += 1
            if i == len(rows):
                raise SystemExit('trace ended before the call log did: the order join does not hold')
            r = rows[i]
            i += 1
            key = (k, c['N'], c['HW'], c['C'], c['act'], ' + '.join('%d%s' % (nc, 'h' if b == 2 else 'f') for nc, b in c['views']) +
                   (' -> dx %s%s' % ('h' if c['dx'][0] == 2 else 'f', ' +=' if c['dx'][1] else '') if c['dir'] == 'bwd' else ''),
                   'x'.join(r[g] for g in ('Grid_Size_X', 'Grid_Size_Y')), r['Kernel_Name'].split('(')[0][:60])
            a = agg.setdefault(key, [0, 0.0, nbytes, 1e30, 0.0])
            t = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
            a[0] += 1; a[1] += t; a[3] = min(a[3], t); a[4] = max(a[4], t)
    print('%d calls, %d launches joined, %d inorm rows skipped (not from these calls), %d left over; %g steps\n' %
          (len(calls), i - skipped, skipped, len(rows) - i, steps))
    print('| kernel | N | HW | C | act | views (channels, f = fp32 / h = bf16) | grid (threads) | launches / step | MB | avg us | min - max us | GB/s | ms / step |')
    print('|---|---|---|---|---|---|---|---|---|---|---|---|---|')
    tot = {}
    for key, (cnt, us, nbytes, lo, hi) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
        print('| %s `%s` | %d | %d | %d | %s | %s | %s | %.1f | %.2f | %.1f | %.1f - %.1f | %.0f | %.3f |' %
              (key[0], key[7], key[1], key[2], key[3], key[4], key[5], key[6], cnt / steps, nbytes / 1e6, us / cnt, lo, hi,
               nbytes / (us / cnt) / 1e3, us / steps / 1e3))
        tot[key[0]] = tot.get(key[0], 0.0) + us / steps / 1e3
    print('\n' + ', '.join('%s %.3f ms / step' % kv for kv in sorted(tot.items())) + ', all %.3f ms / step' % sum(tot.values()))


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(sys.argv[2], sys.argv[3:])
    else:
        table(sys.argv[2], sys.argv[3], float(sys.argv[4]))

"""What the training guard (SAVPEngine(guard=True), csrc/health.hip) costs at the benchmarked step: c2 (B = 16, T = 30, 64 x 64 x 3,
bf16 datapath, shipped tuning table), replayed as the captured hipGraph.

    python tests/tools/time_guard.py step [--rounds 15] [--steps 20]
    python tests/tools/time_guard.py trace [--steps 12]
    python tests/tools/time_guard.py table TRACE.csv

`step` builds the guard-off and the guard-on engine in one process and alternates them: every round times `steps` replayed steps of each
with a host clock around a device synchronise; the medians over the rounds and their difference are printed as one JSON line.
`trace` runs the guard-on engine launch by launch (the kernels are the same ones the replay runs), for
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tests/tools/time_guard.py trace
and `table OUT/.../*_kernel_trace.csv` prints, per kernel of the guard and per optimiser group (told apart by the grid size: one workgroup
per work-list item), the median time and, for the items pass, the rate against the bytes of the group's gradient arena (--groups: the
'groups' object the trace run printed).  Both groups' Adam launches have the same capped grid and share a row."""
import argparse
import collections
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STREAM_YARDSTICK = (5.3e12, 6.1e12)       # bytes / s: the float4 streaming rate of cache-resident tensors (profiles/gru_large.md)


def engine(guard, graph=True):
    import torch
    from tests import gpu_model_checks as G
    from video_prediction_amd import kernels as K
    from video_prediction_amd.models.savp_model import SAVPEngine
    case = G.BENCH_CASES['c2']
    hp, vals, images, noise = G.recipe_case(**case)
    K.set_conv_precision('bf16')
    K.enable_autotune(True)
    K.load_tuning(os.path.join(ROOT, 'video_prediction_amd', 'tuning_gfx950_bf16.json'))
    eng = SAVPEngine(hp, (case['H'], case['W'], case['C']), case['B'], mode='train', values=vals, device='cuda:0', guard=guard)
    eng.use_graph = graph
    eng.set_images(images.float().cuda(), time_major=True)
    return eng, noise


def groups_of(eng):
    out = {}
    for k in ('d', 'g'):
        grp = eng.store.groups[k]
        out[k] = {'arena_bytes': 4 * grp.arena.size, 'variables': len(grp.arena.offsets),
                  'items': int(grp.health_items.shape[0]) if grp.health_state is not None else None}
    return out


def run_step(rounds, steps):
    import torch
    engines = collections.OrderedDict((name, engine(name == 'on')) for name in ('off', 'on'))
    for eng, noise in engines.values():
        for _ in range(4):                             # eager, capture + replay, two replays
            eng.train_step(noise)
        assert eng.graph is not None
    torch.cuda.synchronize()
    times = collections.defaultdict(list)
    for _ in range(rounds):
        for name, (eng, noise) in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                eng.train_step(noise)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    med = {k: sorted(v)[rounds // 2] for k, v in times.items()}
    h = engines['on'][0].store.groups
    print(json.dumps({'what': 'c2 step, bf16 datapath, replayed; guard off and on alternated in one process', 'rounds': rounds,
                      'steps_per_round': steps, 'ms_per_step_off': round(med['off'], 4), 'ms_per_step_on': round(med['on'], 4),
                      'guard_ms': round(med['on'] - med['off'], 4), 'guard_percent': round(100 * (med['on'] - med['off']) / med['off'], 3),
                      'spread_off_ms': [round(min(times['off']), 4), round(max(times['off']), 4)],
                      'spread_on_ms': [round(min(times['on']), 4), round(max(times['on']), 4)],
                      'groups': groups_of(engines['on'][0]),
                      'skipped': {k: int(h[k].health_state[2]) for k in ('d', 'g')}}), flush=True)


def run_trace(steps):
    import torch
    eng, noise = engine(True, graph=False)
    for _ in range(steps):
        eng.train_step(noise)
    torch.cuda.synchronize()
    print(json.dumps({'what': 'c2 step, bf16 datapath, guard on, launch by launch', 'steps': steps, 'groups': groups_of(eng)}), flush=True)


KERNELS = ('health_items_kernel', 'health_fold_kernel', 'adam_guarded_kernel', 'adam_kernel')


def table(path, groups):
    by = collections.defaultdict(list)
    for row in sorted(csv.DictReader(open(path)), key=lambda r: int(r['Start_Timestamp'])):
        name = next((k for k in KERNELS if k in row['Kernel_Name']), None)
        if name:
            grid = int(row.get('Grid_Size_X') or row.get('Grid_Size') or 0)
            by[(name, grid)].append((int(row['End_Timestamp']) - int(row['Start_Timestamp'])) * 1e-3)
    items = {v['items'] * 256: k for k, v in (groups or {}).items() if v.get('items')}
    print('| kernel | grid (threads) | group | launches | median us | bytes | TB/s | of %.1f - %.1f TB/s |' % (STREAM_YARDSTICK[0] * 1e-12,
                                                                                                         STREAM_YARDSTICK[1] * 1e-12))
    print('|---|---|---|---|---|---|---|---|')
    for (name, grid), d in sorted(by.items()):
        d = sorted(d[len(d) // 10:])                   # the first launches are warm-up
        med = d[len(d) // 2]
        grp = items.get(grid) if name == 'health_items_kernel' else None
        nbytes = groups[grp]['arena_bytes'] if grp else None
        rate = nbytes / med * 1e-6 if nbytes else None
        print('| %s | %d | %s | %d | %.2f | %s | %s | %s |' % (
            name, grid, grp or '', len(d), med, nbytes if nbytes else '', '%.2f' % rate if rate else '',
            '%.0f - %.0f %%' % (100 * rate * 1e12 / STREAM_YARDSTICK[1], 100 * rate * 1e12 / STREAM_YARDSTICK[0]) if rate else ''))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['step', 'trace', 'table'])
    ap.add_argument('trace', nargs='?')
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--steps', type=int, default=None)
    ap.add_argument('--groups', help="table: the 'groups' JSON object a step / trace run printed")
    args = ap.parse_args()
    if args.mode == 'step':
        run_step(args.rounds, args.steps or 20)
    elif args.mode == 'trace':
        run_trace(args.steps or 12)
    else:
        table(args.trace, json.loads(args.groups) if args.groups else None)


if __name__ == '__main__':
    main()

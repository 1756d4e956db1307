"""The fixed-problem table of the implicit-GEMM FPROP / DGRAD kernel (csrc/conv_fd_fixed.h), host side, no GPU: for every table line the
ConvP the launcher's planner produces when it is run NOW on the call the line stands for equals, field by field, the constants the line's
kernel has folded at compile time (savp_fd_fixed_probe, include/savp_hip.h); the planner keeps every line's tile and split count; no line
appears twice."""
import ctypes

FIELDS = ('mode', 'N', 'D', 'H', 'W', 'Cx', 'Do', 'Ho', 'Wo', 'Cy', 'kd', 'kh', 'kw', 'sd', 'sh', 'sw', 'pd', 'ph', 'pw', 'splitk', 'tm', 'tn',
          'bf16', 'x_sn', 'x_sd', 'x_sh', 'x_sw', 'y_sn', 'y_sd', 'y_sh', 'y_sw', 'WM', 'WN', 'phases', 'ok')
LINE = ('mode', 'N', 'D', 'H', 'W', 'Cx', 'Do', 'Ho', 'Wo', 'Cy', 'kd', 'kh', 'kw', 'sd', 'sh', 'sw', 'pd', 'ph', 'pw', 'WM', 'WN', 'splitk',
        'flags', 'rank')


def _probe(hip_lib, i, what, n):
    buf = (ctypes.c_int64 * 64)()
    got = hip_lib.savp_fd_fixed_probe(i, what, buf, 64)
    assert got == n, 'entry %d, what %d: %d values, expected %d' % (i, what, got, n)
    return list(buf[:n])


def test_planner_equals_folded_constants(hip_lib):
    count = hip_lib.savp_fd_fixed_count()
    assert count > 0
    for i in range(count):
        line = dict(zip(LINE, _probe(hip_lib, i, 0, len(LINE))))
        planned = dict(zip(FIELDS, _probe(hip_lib, i, 1, len(FIELDS))))
        folded = dict(zip(FIELDS, _probe(hip_lib, i, 2, len(FIELDS))))
        bad = [(f, planned[f], folded[f]) for f in FIELDS if planned[f] != folded[f]]
        assert not bad, 'entry %d: planner against folded constants (field, planned, folded): %s' % (i, bad)
        assert folded['ok'] == 1, 'entry %d: the planner does not keep the tile / split count of its line' % i
        for f in LINE[:19]:
            assert folded[f] == line[f], (i, f)
        assert (folded['WM'], folded['WN'], folded['splitk']) == (line['WM'], line['WN'], line['splitk']), i
        assert folded['bf16'] == (1 if line['flags'] & 2 else 0), i
        # the strides are those of the view the line names
        cx, cy = line['Cx'], line['Cy']
        dense_x = (cx * line['W'] * line['H'] * line['D'], cx * line['W'] * line['H'], cx * line['W'], cx)
        dense_y = (cy * line['Wo'] * line['Ho'] * line['Do'], cy * line['Wo'] * line['Ho'], cy * line['Wo'], cy)
        keep = {5: (1, 1, 1, 1), 4: (1, 0, 1, 1), 2: (1, 0, 0, 0)}[line['rank']]
        assert tuple(folded[f] for f in ('x_sn', 'x_sd', 'x_sh', 'x_sw')) == tuple(a * b for a, b in zip(dense_x, keep)), i
        assert tuple(folded[f] for f in ('y_sn', 'y_sd', 'y_sh', 'y_sw')) == tuple(a * b for a, b in zip(dense_y, keep)), i
        # tile counts as the kernel decodes them: row tiles of the largest output phase, column tiles of the destination channels
        dg = line['mode'] == 1
        up = lambda a, b: -(-a // b)
        mmax = line['N'] * (up(line['D'], line['sd']) * up(line['H'], line['sh']) * up(line['W'], line['sw']) if dg
                            else line['Do'] * line['Ho'] * line['Wo'])
        assert folded['tm'] == up(mmax, 64 * line['WM']) and folded['tn'] == up(cx if dg else cy, 64 * line['WN']), i
        assert folded['phases'] == (line['sd'] * line['sh'] * line['sw'] if dg else 1), i


def test_no_duplicate_lines(hip_lib):
    count = hip_lib.savp_fd_fixed_count()
    lines = [tuple(_probe(hip_lib, i, 0, len(LINE))) for i in range(count)]
    assert len(set(lines)) == len(lines), 'duplicate lines: %s' % sorted(l for l in set(lines) if lines.count(l) > 1)
    # two lines that differ in nothing the launcher compares would shadow each other: split count, tile and flags are compared too,
    # so only the full line has to be unique


def test_unknown_entry_is_refused(hip_lib):
    buf = (ctypes.c_int64 * 8)()
    assert hip_lib.savp_fd_fixed_probe(hip_lib.savp_fd_fixed_count(), 0, buf, 8) == -1
    assert hip_lib.savp_fd_fixed_probe(0, 3, buf, 8) == -1

"""Generate reference_evaluate_flags.json, the command line of the reference's scripts/evaluate.py, from its add_argument calls (run
once with the reference at hand: `python tests/golden/make_evaluate_flags.py <path of alexlee-gk/video_prediction>`).  Data only: for
every flag in declaration order its name and the literal keyword arguments that shape parsing (type, default, nargs, action, choices,
required).  tests/test_evaluate_script.py compares scripts/evaluate.py against it without the reference."""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ('type', 'default', 'nargs', 'action', 'choices', 'required')


def flags_of(source):
    out = []
    for node in ast.walk(ast.parse(source)):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'add_argument'):
            continue
        name = node.args[0].value
        entry = {'flag': name}
        for kw in node.keywords:
            if kw.arg not in KEYS:
                continue
            if kw.arg == 'type':
                entry['type'] = kw.value.id
            else:
                entry[kw.arg] = ast.literal_eval(kw.value)
        out.append((node.lineno, entry))
    return [e for _, e in sorted(out, key=lambda x: x[0])]


def main(ref):
    with open(os.path.join(ref, 'scripts', 'evaluate.py')) as fh:
        flags = flags_of(fh.read())
    if not flags:
        raise SystemExit('no add_argument calls in %s/scripts/evaluate.py' % ref)
    with open(os.path.join(HERE, 'reference_evaluate_flags.json'), 'w') as fh:
        json.dump({'evaluate.py': flags}, fh, indent=1, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main(sys.argv[1])

"""Generate the committed fixtures that stand for files of the reference checkout (run once with the reference at hand:
`python tests/golden/make_reference_fixtures.py <path of alexlee-gk/video_prediction>`):
  reference_recipes.json        hparams/<dataset>/ours_*/model_hparams.json, keyed by '<dataset>/<recipe>'
  reference_script_flags.json   the command-line flags scripts/train.py and scripts/generate.py declare
Both are data read out of the reference, so the tests that compare against it run without it."""
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref):
    recipes = {}
    for f in sorted(glob.glob(os.path.join(ref, 'hparams', '*', 'ours_*', 'model_hparams.json'))):
        with open(f) as fh:
            recipes[os.path.relpath(os.path.dirname(f), os.path.join(ref, 'hparams'))] = json.load(fh)
    if not recipes:
        raise SystemExit('no hparams/*/ours_*/model_hparams.json under %s' % ref)
    flags = {}
    for name in ('train.py', 'generate.py'):
        with open(os.path.join(ref, 'scripts', name)) as fh:
            flags[name] = sorted(set(re.findall(r'add_argument\(\s*"(--[a-z_]+)"', fh.read())))
    for fname, obj in (('reference_recipes.json', recipes), ('reference_script_flags.json', flags)):
        with open(os.path.join(HERE, fname), 'w') as fh:
            json.dump(obj, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main(sys.argv[1])

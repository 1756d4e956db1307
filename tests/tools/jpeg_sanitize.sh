#!/bin/bash
# CPU-only developer check: the host JPEG decoder built with AddressSanitizer + UBSan, run over every proper prefix of two committed
# streams (one 4:2:0 with restart markers, one 4:2:2 with optimised tables and restart markers) and over 20000 damaged copies of each.
# Usage: tests/tools/jpeg_sanitize.sh        (from the repository root; needs g++ with libasan / libubsan; never touches a GPU)
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
TMP="$(mktemp -d)"
trap 'rm -rf "$TMP"' EXIT
python - "$ROOT" "$TMP" <<'PY'
import os, sys
import numpy as np
root, tmp = sys.argv[1:3]
f = np.load(os.path.join(root, 'tests', 'golden', 'jpeg_fixtures.npz'))
names = [str(n) for n in f['names']]
for tag, start in (('a', 'smooth 64x64 420 q95 rst3'), ('b', 'noise 48x80 422')):
    i = next(k for k, n in enumerate(names) if n.startswith(start))
    open(os.path.join(tmp, tag + '.jpg'), 'wb').write(f['jpeg_%d' % i].tobytes())
PY
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -I"$ROOT/include" \
    "$ROOT/tests/tools/jpeg_prefix_driver.cpp" "$ROOT/video_prediction_amd/csrc_host/jpeg_decode.cpp" -o "$TMP/driver"
"$TMP/driver" "$TMP/a.jpg" "$TMP/b.jpg"

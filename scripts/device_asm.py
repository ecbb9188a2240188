"""Device-only assembly of every source of the library, each with its own flags -- to show that a host-side change left the
kernels alone: run it on both commits and `diff -r` the two directories (0 differing lines per file is the expected answer;
a changed ORDER of template instantiations shows as a file-wide diff of identical kernels).

    python scripts/device_asm.py OUT_DIR [JOBS]
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motion_planning_baselines_amd import build as b


def one(src, out):
    raw = os.path.join(out, src + '.raw.s')
    subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), *b.FLAGS, *b.EXTRA.get(src, []), '--cuda-device-only', '-S',
                           os.path.join(b.CSRC, src), '-o', raw], stderr=subprocess.DEVNULL)
    with open(raw) as fh, open(os.path.join(out, src + '.s'), 'w') as oh:
        oh.writelines(line for line in fh if '__hip_cuid' not in line)    # (a per-compile id: the only line two compiles of one file differ in)
    os.remove(raw)
    return src


if __name__ == '__main__':
    out = os.path.abspath(sys.argv[1])
    os.makedirs(out, exist_ok=True)
    with ThreadPoolExecutor(int(sys.argv[2]) if len(sys.argv) > 2 else 4) as ex:
        for s in ex.map(lambda s: one(s, out), b.SOURCES + b.DEBUG_SOURCES):
            print('done', s, flush=True)

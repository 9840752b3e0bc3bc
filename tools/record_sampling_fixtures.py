#!/usr/bin/env python3
"""Record tests/golden/sampling_kernels.json: digests of what the DiT sampling kernels outside the GEMMs return for the seeded cases of
tests/sampling_cases.py, with the build this is run on (BSI_HIP_LIB selects a library other than the in-tree one).

The record is the yardstick for changes to these kernels that must not change a bit: run it ONCE with the build from before such a
change (the parent commit's library), commit the file, and tests/test_hip_sampling_fixtures.py holds every later build against it.
Re-recording with a changed kernel would make the test vacuous.

    BSI_HIP_LIB=/path/to/parent/libbsi_hip.so python tools/record_sampling_fixtures.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="output file (default: tests/golden/sampling_kernels.json)")
    args = ap.parse_args()
    import torch

    from bsi_amd import _native as N
    from tests import sampling_cases as sc

    assert torch.cuda.is_available(), "recording needs the GPU"
    N.lib()
    record = {}
    for case, thunk in sc.all_cases(N):
        record[case] = {name: sc.digest(t) for name, t in thunk().items()}
        print(f"{case}: " + ", ".join(f"{n} {v['sha256'][:12]}" for n, v in record[case].items()), flush=True)
    out = args.out or sc.FIXTURE
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(record, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out} ({os.path.getsize(out)} bytes, {len(record)} cases) with {N.LIB_PATH}")


if __name__ == "__main__":
    main()

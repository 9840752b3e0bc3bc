#!/usr/bin/env python3
"""Record the bit-level yardsticks under tests/golden/ with the build and the package this is run on:

  --set sampling (default): tests/golden/sampling_kernels.json, digests of what the DiT sampling kernels outside the GEMMs return
      for the seeded cases of tests/sampling_cases.py (BSI_HIP_LIB selects a library other than the in-tree one);
  --set models: tests/golden/model_surface.json, digests of what the two native denoisers return at model level -- forward, deep
      copy, sampling, gradients, DPTrainer steps -- for the seeded cases of tests/model_cases.py.

A record is the yardstick for changes that must not change a bit: run this ONCE with the code from before such a change (the parent
commit's library for the kernels, the parent commit's bsi_amd/ for the model surface), commit the file, and
tests/test_hip_sampling_fixtures.py / tests/test_hip_model_surface.py hold every later tree against it.  Re-recording with the
changed code would make the test vacuous.

    BSI_HIP_LIB=/path/to/parent/libbsi_hip.so python tools/record_sampling_fixtures.py [--set sampling|models] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--set", choices=("sampling", "models"), default="sampling", help="which record to write")
    ap.add_argument("--out", default=None, help="output file (default: the record's place under tests/golden/)")
    args = ap.parse_args()
    import torch

    from bsi_amd import _native as N
    from tests import sampling_cases as sc

    assert torch.cuda.is_available(), "recording needs the GPU"
    N.lib()
    if args.set == "models":
        from tests import model_cases as mc
        cases, default = mc.all_cases(), mc.FIXTURE
    else:
        cases, default = sc.all_cases(N), sc.FIXTURE
    record = {}
    for case, thunk in cases:
        record[case] = {name: sc.digest(t) for name, t in thunk().items()}
        print(f"{case}: " + ", ".join(f"{n} {v['sha256'][:12]}" for n, v in record[case].items()), flush=True)
    out = args.out or default
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(record, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out} ({os.path.getsize(out)} bytes, {len(record)} cases) with {N.LIB_PATH}")


if __name__ == "__main__":
    main()

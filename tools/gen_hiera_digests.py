"""Digests, workspace sizes and launch counts of whole Hiera forwards: `python tools/gen_hiera_digests.py` on the GPU.

Runs every case of tests/test_gpu_hiera_bits.py (ovo_hiera_forward down each of its paths; inputs from integer arithmetic) with the library as built and
writes, per case, one sha256 per output level, `ovo_hiera_workspace_bytes` and the profiler's launch counts to tests/golden/hiera_digests.json.  Run it
BEFORE a change that must not move the forward's results, commit the file, then make the change: the test compares with the file.  Only digests and
counts go to disk.
"""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
os.environ["OVO_KNOBS_DYNAMIC"] = "1"       # the cases flip OVO_* knobs between forwards: set before the library is first loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hiera_digests.json"))
    a = ap.parse_args()
    import test_gpu_hiera_bits as T
    records = {T.case_id(c): T.run_case(c) for c in T.CASES}
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out} {os.path.getsize(a.out)} bytes, {len(records)} cases")


if __name__ == "__main__":
    main()

"""Digests of the fused TSDF model's outputs: `python tools/gen_tsdf_digests.py` on the GPU.

Runs every case of tests/test_gpu_tsdf_bits.py (integrate plain and with colour, the four ray-cast forms, the mesh with colours and normals, the label
vote, ray cast and mesh, the twelve sampler forms, the alignment to the volume; the cases of the other TSDF tests) with the library as it stands and writes, per case, the sha256 of every output array and the mesh's (V, T) to
tests/golden/tsdf_digests.json.  Run it BEFORE a change that must not move the model's results, commit the file, then make the change: the test compares
with the file.  Regenerate it only in a pull request that MEANS to move results (another weight, another clip, another blend order), and say so there; a
refactor never does.  Only digests and counts go to disk.
"""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
os.environ["OVO_KNOBS_DYNAMIC"] = "1"       # the cases flip the grid caps between launches: set before the library is first loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tsdf_digests.json"))
    a = ap.parse_args()
    import test_gpu_tsdf_bits as B
    records = {B.case_id(c): B.run_case(c) for c in B.CASES}
    assert len(records) == len(B.CASES)
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out} {os.path.getsize(a.out)} bytes, {len(records)} cases")


if __name__ == "__main__":
    main()

"""Digests of the row-streaming kernels' outputs: `python tools/gen_stream_digests.py` on the GPU.

Runs every case of tests/test_gpu_stream_bits.py (ovo_mlp_f32, ovo_neck_f32, ovo_gemm_f32a; inputs from integer arithmetic, see `values` there) with the
library as built and writes one sha256 per output tensor to tests/golden/stream_digests.json.  Run it BEFORE a change that must not move a bit of these
kernels, commit the file, then make the change: the test compares with the file.  Only digests go to disk.
"""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stream_digests.json"))
    a = ap.parse_args()
    import test_gpu_stream_bits as T
    digests = {T.case_id(c): T.digest_of(c) for c in T.CASES}
    with open(a.out, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out} {os.path.getsize(a.out)} bytes, {len(digests)} cases")


if __name__ == "__main__":
    main()

"""Digests and launch counts of whole SAM2 decoder forwards: `python tools/gen_sam_decoder_digests.py` on the GPU.

Runs every case of tests/test_gpu_sam_decoder_bits.py (HipSamDecoder.forward down each of its paths; inputs and weights from integer arithmetic) with the
package as it stands and writes, per case, the sha256 of the mask logits and of the predicted IoUs and the profiler's launch counts to
tests/golden/sam_decoder_digests.json.  Run it BEFORE a change that must not move the forward's results, commit the file, then make the change: the test
compares with the file.  Only digests and counts go to disk.
"""
import argparse
import json
import os
import sys

sys.dont_write_bytecode = True
os.environ["OVO_KNOBS_DYNAMIC"] = "1"       # as under the test suite: set before the library is first loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sam_decoder_digests.json"))
    a = ap.parse_args()
    import test_gpu_sam_decoder_bits as T
    records = {c.id: T.run_case(c) for c in T.CASES}
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out} {os.path.getsize(a.out)} bytes, {len(records)} cases")


if __name__ == "__main__":
    main()

"""The launch plan of HipSamDecoder.forward, per case of tests/test_sam_decoder_plan_host.py: `python tools/gen_sam_decoder_plan.py` (CPU only, no library).

Writes, per case, the sha256 of the canonical JSON of the whole call trace, the number of calls and the count per entry point to
tests/golden/sam_decoder_plan.json.  Run it BEFORE a change that must not move a launch, commit the file, then make the change: the test compares with the
file.  `--dump DIR` also writes every full trace (one call per line) to DIR/<case>.txt; after a mismatch, diff a dump of the tree at hand against a dump made
at the commit the golden was written at (`--out /dev/null --dump DIR` leaves the golden alone).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "sam_decoder_plan.json"))
    ap.add_argument("--dump", metavar="DIR", help="also write the full traces there")
    a = ap.parse_args()
    import pytest
    import test_sam_decoder_plan_host as T
    records = {}
    for case in T.CASES:
        with pytest.MonkeyPatch.context() as mp:
            trace = T.trace_case(case, mp)
        records[case.id] = T.summary(trace)
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, case.id + ".txt"), "w") as f:
                f.writelines(T.canonical(call) + "\n" for call in trace)
    with open(a.out, "w") as f:
        json.dump(records, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}, {len(records)} cases: " + ", ".join(f"{k} {v['calls']}" for k, v in records.items()))


if __name__ == "__main__":
    main()

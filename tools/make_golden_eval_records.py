#!/usr/bin/env python
"""Write tests/golden/eval_single_probe_records.json: the record `main` returns (per-epoch accuracies, per-iteration learning rate
and loss) for the single-probe frozen evals on the micro synthetic configs of the eval tests, on the GPU.

    python tools/make_golden_eval_records.py [output.json]

tests/test_eval_multihead_gpu.py holds the configs and compares a run without `optimization.multihead_kwargs` against this file.
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests.test_eval_multihead_gpu import GOLDEN, single_probe_record
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = {}
    for kind in ("video", "image"):
        with tempfile.TemporaryDirectory() as d:
            rec[kind] = single_probe_record(kind, d)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()

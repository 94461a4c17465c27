"""SHA-256 of what the fit hooks return on the inputs of tests/test_select_finish.py (medians whose buckets are runs of duplicates), one JSON line
per case.  Run on the commit BEFORE a change to the selections; the lines are that test's PARENT_SHA.

    python tests/diag/select_finish_fit_hashes.py > parent_fit_hashes.jsonl
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_select_finish as T               # noqa: E402

pkg = importlib.import_module("vistaf-roboskin-vision-integrated-multimodal-sensor_amd")

if __name__ == "__main__":
    for h, w in T.FIT_SHAPES:
        for case, sha in T.fit_hashes(pkg, h, w).items():
            print(json.dumps({"case": case, "sha256": sha}), flush=True)

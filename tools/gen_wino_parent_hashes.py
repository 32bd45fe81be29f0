#!/usr/bin/env python3
"""Record what the Winograd kernels compute NOW, as one SHA-256 of the output bytes per case of tests/wino_cases.py:

    python3 tools/gen_wino_parent_hashes.py OUT.json [commit]

Run on the GPU with the library of the commit whose results are to be pinned (before a change to csrc/ore_conv_wino.hip that must not
move a bit); the result goes to tests/golden/wino_parent_sha256.json, which tests/test_hip_wino_desc.py compares against."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "faster-orefsdet_amd"), ROOT):
    sys.path.insert(0, p)
import orehip  # noqa: E402
import wino_cases as wc  # noqa: E402

out_path = sys.argv[1]
commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"
hashes = {}
with orehip.conv_overrides((-7, 2)):
    for case in wc.CASES:
        hashes[case["id"]] = wc.digest(wc.run(orehip, case, wc.make(case)))
rec = {"ore_version": int(orehip.lib().ore_version()), "commit": commit, "what": "sha256 of the fp32 output rows (sentinel columns included)",
       "sha256": hashes}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(hashes)} cases, ore_version {rec['ore_version']} -> {out_path}")

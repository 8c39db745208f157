#!/usr/bin/env python3
"""A bit record (tools/net_hashes.py: {case: {tensor: sha256}}; GI_NORM_HASHES of tests/test_norm_ops_gpu.py: {"test|type|case
output": sha256}) condensed for committing: per case, or per test function and compute type, the number of entries and one sha256
over their sorted "key=hash" lines. Two full records are equal exactly when their condensed forms are.
usage: condense_hashes.py FULL.json OUT.json"""
import hashlib, json, sys

full = json.load(open(sys.argv[1]))
groups = {}
for k, v in full.items():
    if isinstance(v, dict):
        groups[k] = v
    else:
        groups.setdefault("|".join(k.split("|")[:2]), {})[k] = v
out = {g: {"entries": len(d), "sha256": hashlib.sha256("\n".join(f"{k}={d[k]}" for k in sorted(d)).encode()).hexdigest()}
       for g, d in groups.items()}
open(sys.argv[2], "w").write("{\n" + ",\n".join(f"{json.dumps(g)}: {json.dumps(out[g])}" for g in sorted(out)) + "\n}\n")   # one group per line
print(f"{sum(len(d) for d in groups.values())} entries in {len(out)} groups")

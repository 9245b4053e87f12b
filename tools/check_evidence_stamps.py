#!/usr/bin/env python3
"""Are profiles/query_pmc.json, mesh_pmc.json, fit_pmc.json and fit_mfma_pmc.json still the counters of the kernels in the tree?  The
last three are stamped by tools/pmc_json.py with a hash of the files that hold their kernels (its MESH_FILES, FIT_FILES, MFMA_FILES); an
edit to one of those calls for tools/mesh_pmc.sh / tools/fit_pmc_all.sh / tools/fit_mfma_pmc.sh again.  (bench.py hashes a list of its
own and shows a record's counters only when both agree.)  No GPU needed.
usage: python tools/check_evidence_stamps.py   (exit code 1 if anything is stale)"""
import hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hp-adaptive-signed-distance-field-octree_amd", "csrc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pmc_json  # noqa: E402  (the lists and the hash the records are stamped with)

bad = 0
for name, files in (("mesh_pmc.json", pmc_json.MESH_FILES), ("fit_pmc.json", pmc_json.FIT_FILES), ("fit_mfma_pmc.json", pmc_json.MFMA_FILES)):
    cur = pmc_json.source_sha16(files)
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", name))).get("source_sha16")
    except Exception:  # noqa: BLE001
        rec = None
    state = "MISSING" if rec is None else ("current" if rec == cur else "STALE")
    bad += state != "current"
    print("%-16s %s (recorded %s, tree %s)" % (name, state, rec, cur))
text = open(os.path.join(CSRC, "kernels.hip")).read()
a, b = text.index("template <int TOPD, bool DEDUPE, bool GRAD>"), text.index("// 16-byte chunks a leaf of degree d occupies")
cur = hashlib.sha256(text[a:b].encode()).hexdigest()[:16]
try:
    rec = json.load(open(os.path.join(ROOT, "profiles", "query_pmc.json"))).get("query_kernel_sha16")
except Exception:  # noqa: BLE001
    rec = None
state = "MISSING" if rec is None else ("current" if rec == cur else "STALE")
bad += state != "current"
print("%-16s %s (recorded %s, tree %s)" % ("query_pmc.json", state, rec, cur))
sys.exit(1 if bad else 0)

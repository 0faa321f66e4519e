"""Writes tests/golden/wgrad_plan.json: one sha256 per (config, classes, H, W) group over the host decisions of every weight gradient the
training engine launches in the dispatch census's input space -- kernel code, workspace bytes and the fields
ryolo_conv_wgrad_reduce_job_fill writes (tests/dispatch_census.py: wgrad_plan_groups) -- plus the bs-64 608^2 blocks under the tile bits
0x1000, 0x2000, 0x2000|0x4000 and a forced split count of 3.

The file pins the decisions of the library as it was BEFORE the weight gradient's host code was rewritten around one plan: generate it
from a library built at the PARENT of the commit under test (RYOLO_HIP_LIB=<that build's libryolo_hip.so>), never from the code the
test then checks.  tests/test_dispatch_census.py::test_wgrad_host_decisions_match_the_golden recomputes the hashes; a failure names the group.

    RYOLO_HIP_LIB=/path/to/parent/libryolo_hip.so python tests/golden/gen_wgrad_plan_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import dispatch_census as dc  # noqa: E402

if __name__ == "__main__":
    if not os.environ.get("RYOLO_HIP_LIB"):
        sys.exit("set RYOLO_HIP_LIB to a library built at the parent commit (see the docstring)")
    groups = dc.wgrad_plan_groups()
    out = {"library": dc._L().ryolo_build_id().decode(), "records": sum(len(v) for v in groups.values()), "groups": dc.wgrad_plan_hashes(groups)}
    with open(os.path.join(HERE, "wgrad_plan.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d groups, %d records, library %s" % (len(out["groups"]), out["records"], out["library"]))

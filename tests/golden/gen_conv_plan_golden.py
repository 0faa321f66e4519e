"""Writes tests/golden/conv_plan.json: one sha256 per group over the host decisions of the forward convolution and the data gradient as
the library's queries show them (tests/dispatch_census.py: conv_plan_groups) -- the kernel of every descriptor of the dispatch census's
input space, and of a base set of plans under every forced tile, tile bit, tuning switch and size guard.

The file pins the decisions of the library as it was BEFORE the convolution dispatch was rewritten around one plan: generate it from a
library built at the PARENT of the commit under test (RYOLO_HIP_LIB=<that build's libryolo_hip.so>), never from the code the test then
checks.  tests/test_dispatch_census.py::test_conv_host_decisions_match_the_golden recomputes the hashes; a failure names the group, and
--dump GROUP prints that group's rows (one JSON list per line) for a diff between two libraries.

    RYOLO_HIP_LIB=/path/to/parent/libryolo_hip.so python tests/golden/gen_conv_plan_golden.py [--dump GROUP | --dump all]
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
    groups = dc.conv_plan_groups()
    if "--dump" in sys.argv:
        want = sys.argv[sys.argv.index("--dump") + 1]
        for name in sorted(groups):
            if want in ("all", name):
                for row in groups[name]:
                    print(name, json.dumps(row))
        sys.exit(0)
    out = {"library": dc._L().ryolo_build_id().decode(), "records": sum(len(v) for v in groups.values()), "groups": dc.conv_plan_hashes(groups)}
    with open(os.path.join(HERE, "conv_plan.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("%d groups, %d records, library %s" % (len(out["groups"]), out["records"], out["library"]))

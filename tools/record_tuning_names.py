#!/usr/bin/env python3
"""Records tests/tuning_names_recorded.json: what gvom_set_tuning and gvom_get_tuning answer to every name (tests/test_tuning_names.py
has the names and the replay).  Run it on the MI355X with the production library the test is to hold later ones to -- the one of the
commit BEFORE a change to the tuning functions -- and commit the file it writes.

    tools/record_tuning_names.py [out.json]        (default: tests/tuning_names_recorded.json; GVOM_HIP_LIBRARY selects the library)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "g-vom_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def write(path, rec):
    """one case per line"""
    head = dict(rec, results=[])
    with open(path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-3].rstrip() + "\n")
        f.write(",\n".join("  " + json.dumps(r) for r in rec["results"]))
        f.write("\n ]\n}\n")


def main():
    import gvom
    import test_tuning_names as t
    import lib_identity
    path = sys.argv[1] if len(sys.argv) > 1 else t.RECORDED
    results = t.replay(gvom)
    rec = {"what": "gvom_get_tuning / gvom_set_tuning: [case, return code, value] of tests/test_tuning_names.py::replay",
           "library": lib_identity.identity(gvom.library_path()), "params": list(t.PARAMS), "values": list(t.VALUES), "results": results}
    write(path, rec)
    print("wrote %s: %d cases" % (path, len(results)))


if __name__ == "__main__":
    main()

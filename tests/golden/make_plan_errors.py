"""Generates tests/golden/plan_errors.json: what the five planner entry points answer to the refused arguments of
tests/plan_error_cases.py (return code and kao_last_error() text per case).  No GPU is needed: every planner validates first.

    python tests/golden/make_plan_errors.py [--lib PATH/libkao.so] [--only CASE_ID ...]

Record the table with the library of the commit whose answers are the reference (--lib); --only re-records the named cases alone
and leaves every other row as it is (for a change that moves a rule on purpose)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import plan_error_cases as pec  # noqa: E402
from kafka_assignment_optimizer_amd import _ffi  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    if a.lib:
        _ffi.LIB_PATH = os.path.abspath(a.lib)
    lib = _ffi.load()
    path = os.path.join(HERE, "plan_errors.json")
    rows = {}
    if a.only is not None:
        with open(path) as f:
            rows = {r["id"]: r for r in json.load(f)["cases"]}
    for cid in (a.only if a.only is not None else pec.CASES):
        rc, text, untouched = pec.call(lib, cid)
        assert rc != 0 and untouched, (cid, rc, text)
        rows[cid] = {"id": cid, "rc": rc, "error": text}
    with open(path, "w") as f:
        f.write('{"cases":[\n' + ",\n".join(json.dumps(rows[cid], separators=(",", ":")) for cid in pec.CASES) + "\n]}\n")
    print("wrote plan_errors.json:", len(rows), "cases")


if __name__ == "__main__":
    main()

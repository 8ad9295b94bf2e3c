"""The log-dir front ends on the MI355X against what they wrote before they shared one mapping, one report path and one plan writer:
for every case of tests/golden/logdirs_front, cli/kao-logdirs and the Python twin with --report in every mode the case allows (plain,
--exchange, by capacities, --plan / --evacuate with and without --rebalance, --dry-run) write the recorded plan file and the recorded
report and return the recorded status.  The planners are deterministic: the comparison is of bytes."""
import os
import subprocess

import pytest

import test_logdirs_front as front
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", front.CASES)
def test_both_programs_write_the_recorded_bytes(case, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    runs = front.load_case(case)["runs"]
    assert case == "refused" or sum(r["status"] == 0 and "logdirs: status=" in r["stderr"] for r in runs) >= 4
    front.check_runs(case, runs, tmp_path)

"""The five planner entry points (kao_balance_leaders, _cluster, _weighted, kao_failover_order, _weighted) refuse bad arguments with
the recorded return code and kao_last_error() text, before they touch a device or the rows: tests/golden/plan_errors.json
(tests/golden/make_plan_errors.py) replayed case by case.  No GPU is needed."""
import pytest

import plan_error_cases as pec
from conftest import load_golden

GOLDEN = {r["id"]: r for r in load_golden("plan_errors.json")["cases"]}


def test_table_covers_every_case():
    assert list(GOLDEN) == list(pec.CASES)
    for entry in pec.BASE:
        assert sum(1 for cid in GOLDEN if cid.startswith(entry + "/")) >= 20, entry


@pytest.mark.parametrize("cid", list(pec.CASES))
def test_refused_as_recorded(cid):
    from kafka_assignment_optimizer_amd import _ffi
    rc, text, rows_untouched = pec.call(_ffi.load(), cid)
    assert (rc, text) == (GOLDEN[cid]["rc"], GOLDEN[cid]["error"])
    assert rows_untouched

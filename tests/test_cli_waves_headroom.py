"""kao-waves --headroom end to end on the MI355X: the C++ tool and its Python twin write the same wave files, the same stuck file and
the same report, exit with status 3 when partitions are stuck and 0 when the plan completes, and take a broker's capacity from
--capacities, else the totalBytes of the kafka-log-dirs document, else --default-capacity."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _doc(rows):
    return {"version": 1, "partitions": [{"topic": "t", "partition": p, "replicas": r} for p, r in enumerate(rows)]}


def _both(tmp_path, cur, plan, sizes, flags):
    """Runs both tools; returns [(exit status, stderr text, {file name without its prefix: parsed JSON})] after asserting they agree."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    for name, doc in (("c.json", cur), ("p.json", plan), ("s.json", sizes)):
        (tmp_path / name).write_text(json.dumps(doc))
    out = []
    for tag, tool in (("cpp_", [os.path.join(ROOT, "cli", "kao-waves")]), ("py_", [sys.executable, "-m", "kafka_assignment_optimizer_amd.waves"])):
        r = subprocess.run(tool + ["--current", str(tmp_path / "c.json"), "--plan", str(tmp_path / "p.json"), "--sizes", str(tmp_path / "s.json"),
                                   "--out-prefix", str(tmp_path / tag), "--report"] + flags, capture_output=True, cwd=ROOT)
        files = {f.name[len(tag):]: json.load(open(f)) for f in sorted(tmp_path.glob(tag + "*"))}
        out.append((r.returncode, r.stderr.decode(), files))
    assert out[0] == out[1]
    return out[0]


def _plain(sizes):
    return {"partitions": [{"topic": "t", "partition": p, "size": s} for p, s in enumerate(sizes)]}


def test_both_tools_agree_on_an_input_that_gets_stuck(tmp_path):
    """Partitions 0 and 1 (60 bytes) swap between brokers 1 and 2 of 100 bytes each: stuck.  Partition 2 moves 3 -> 4 in wave 1, and
    partition 3 follows into the room it frees on broker 3 in wave 2."""
    cur = _doc([[1], [2], [3], [5]])
    plan = _doc([[2], [1], [4], [3]])
    rc, err, files = _both(tmp_path, cur, plan, _plain([60, 60, 40, 70]), ["--capacities", "1:100,2:100,3:100,4:50,5:1K"])
    assert rc == 3
    assert sorted(files) == ["-stuck.json", "1.json", "2.json"]
    assert files["1.json"] == {"version": 1, "partitions": [{"topic": "t", "partition": 2, "replicas": [4]}]}
    assert files["2.json"]["partitions"] == [{"topic": "t", "partition": 3, "replicas": [3]}]
    assert files["-stuck.json"] == {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [2]}, {"topic": "t", "partition": 1, "replicas": [1]}]}
    lines = err.strip().splitlines()
    assert lines[-1] == "stuck: 2 partitions, 120 bytes"
    # wave 1: broker 4 holds 0 + 40 of 50 = 80 %; wave 2: broker 3 holds 0 + 70 of 100
    assert lines[0] == ("waves=2 lower_bound=1 optimal=no partitions_per_wave=1,1 bytes_lower_bound=0 max_broker_bytes_per_wave=40,70 "
                        "fullest_receiver_pct_per_wave=80.00,70.00 min_free=10 min_free_wave=1 min_free_broker=4 stuck=2 stuck_bytes=120")


def test_python_api_sets_the_headroom_fields():
    """The same input through waves.plan_waves: stuck keys with their target rows, the least free bytes with a broker id, the peaks
    in ppm; an explicit `stored` replaces the derived one (broker 4 already holds 20 bytes: partition 2 no longer fits)."""
    import kafka_assignment_optimizer_amd as kao
    from kafka_assignment_optimizer_amd.waves import plan_waves
    kao.init(0)
    cur, plan = _doc([[1], [2], [3], [5]]), _doc([[2], [1], [4], [3]])
    caps = {1: 100, 2: 100, 3: 100, 4: 50, 5: "1K"}
    res = plan_waves(cur, plan, sizes=_plain([60, 60, 40, 70]), capacity=caps)
    assert res.headroom and res.wave.tolist() == [-2, -2, 0, 1] and (res.n_waves, res.lower_bound, res.optimal) == (2, 1, False)
    assert res.stuck == [("t", 0, [2]), ("t", 1, [1])] and res.stuck_bytes == 120
    assert res.stuck_document == {"version": 1, "partitions": [{"topic": "t", "partition": 0, "replicas": [2]}, {"topic": "t", "partition": 1, "replicas": [1]}]}
    assert (res.min_free, res.min_free_wave, res.min_free_broker) == (10, 0, 4)
    assert res.peak_utilisation_ppm == [800000, 700000] and [len(d["partitions"]) for d in res.waves] == [1, 1]
    assert res.stats[0] == 2 and res.stats[3] == 64
    res = plan_waves(cur, plan, sizes=_plain([60, 60, 40, 70]), capacity=caps, stored={4: 20})
    assert res.wave.tolist() == [-2, -2, -2, -2] and res.n_waves == 0 and res.waves == [] and res.min_free == -1
    # without any headroom keyword the call is the sized planner's, as before
    res = plan_waves(cur, plan, sizes=_plain([60, 60, 40, 70]), max_bytes_per_broker=100)
    assert not res.headroom and res.stuck == [] and res.wave.min() >= 0


def test_both_tools_exit_0_on_an_input_that_completes(tmp_path):
    cur = _doc([[1], [2]])
    plan = _doc([[2], [3]])
    rc, err, files = _both(tmp_path, cur, plan, _plain([60, 60]), ["--default-capacity", "125", "--max-utilisation", "80", "--max-per-broker", "1"])
    assert rc == 0 and sorted(files) == ["1.json", "2.json"]          # the chain: 2 -> 3 first, then 1 -> 2 (effective capacity 100)
    assert files["1.json"]["partitions"] == [{"topic": "t", "partition": 1, "replicas": [3]}]
    assert err.strip() == ("waves=2 lower_bound=2 optimal=yes partitions_per_wave=1,1 bytes_lower_bound=0 max_broker_bytes_per_wave=60,60 "
                           "fullest_receiver_pct_per_wave=48.00,48.00 min_free=40 min_free_wave=1 min_free_broker=3 stuck=0 stuck_bytes=0")


def test_capacity_falls_back_from_the_table_to_total_bytes_to_the_default(tmp_path):
    """Broker 2 is named in --capacities, broker 3 reports totalBytes, broker 4 has neither.  Each receives one 60-byte partition
    and holds 40 bytes of another; the table and totalBytes leave room (100), the default (99) does not."""
    cur = _doc([[1], [1], [1], [2], [3], [4]])
    plan = _doc([[2], [3], [4], [2], [3], [4]])

    def broker(b, entries, total):
        d = {"logDir": "/d", "error": None, "partitions": [{"partition": f"t-{p}", "size": s, "offsetLag": 0, "isFuture": False} for p, s in entries]}
        if total is not None:
            d["totalBytes"], d["usableBytes"] = total, 0
        return {"broker": b, "logDirs": [d]}
    logdirs = {"version": 1, "brokers": [broker(1, [(0, 60), (1, 60), (2, 60)], 1000), broker(2, [(3, 40)], 50), broker(3, [(4, 40)], 100),
                                         broker(4, [(5, 40)], None)]}
    rc, err, files = _both(tmp_path, cur, plan, logdirs, ["--capacities", "2:100", "--default-capacity", "99"])
    assert rc == 3 and sorted(files) == ["-stuck.json", "1.json"]
    assert [e["partition"] for e in files["1.json"]["partitions"]] == [0, 1]
    assert files["-stuck.json"]["partitions"] == [{"topic": "t", "partition": 2, "replicas": [4]}]
    assert "fullest_receiver_pct_per_wave=100.00 min_free=0 min_free_wave=1 min_free_broker=2 stuck=1 stuck_bytes=60" in err
    # with a default of 100 everything fits
    (tmp_path / "again").mkdir()
    rc, err, files = _both(tmp_path / "again", cur, plan, logdirs, ["--capacities", "2:100", "--default-capacity", "100"])
    assert rc == 0 and "stuck=0" in err and sorted(files) == ["1.json"] and [e["partition"] for e in files["1.json"]["partitions"]] == [0, 1, 2]

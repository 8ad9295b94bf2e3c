"""The log-dir front ends (cli/kao-logdirs and kafka_assignment_optimizer_amd.logdirs) against what they gave before they shared one
mapping, one report path and one plan writer: tests/golden/logdirs_front/<case>/ holds the input documents of a small cluster and,
in case.json, the arrays that parse_input / parse_place_input made of them (or the text of the refusal) and, per flag list, the exit
status, the report and the plan file that both programs wrote.  No device here: the mappings, the runs that are refused before the
device is touched, and the reason one mapping serves both calls (parse_input is parse_place_input without plan or evacuation, on
200 random documents).  The runs that reach the device are in test_gpu_logdirs_front.py."""
import dataclasses
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FRONT = os.path.join(GOLDEN, "logdirs_front")
CASES = sorted(os.listdir(FRONT))
PROGS = {"cli": [os.path.join(ROOT, "cli", "kao-logdirs")], "py": [sys.executable, "-m", "kafka_assignment_optimizer_amd.logdirs"]}


def load_case(case):
    with open(os.path.join(FRONT, case, "case.json")) as f:
        return json.load(f)


def _document(case, name):
    with open(os.path.join(FRONT, case, name)) as f:
        return f.read() if name.endswith(".txt") else json.load(f)


def plain(x):
    """A mapping's fields as JSON holds them: an array as its dtype and values, a tuple as a list."""
    if dataclasses.is_dataclass(x):
        return {f.name: plain(getattr(x, f.name)) for f in dataclasses.fields(x)}
    if isinstance(x, np.ndarray):
        return {"dtype": str(x.dtype), "values": x.tolist()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def mappings_of(case, args):
    """{"place": ..., "balance": ...}: the fields of parse_place_input, and without plan and evacuation those of parse_input as well;
    {"error": text} for a refusal."""
    from kafka_assignment_optimizer_amd.logdirs import parse_input, parse_place_input
    cur, dirs = _document(case, args["current"]), _document(case, args["log_dirs"])
    plan = None if args["plan"] is None else _document(case, args["plan"])
    calls = {"place": lambda: parse_place_input(cur, dirs, plan, [tuple(e) for e in args["evacuate"]], args["broker_list"], args["default_size"])}
    if plan is None and not args["evacuate"]:
        calls["balance"] = lambda: parse_input(cur, dirs, args["broker_list"])
    out = {}
    for name, call in calls.items():
        try:
            out[name] = plain(call())
        except ValueError as e:
            out[name] = {"error": str(e)}
    return out


def run(case, flags, prog, out):
    """One program in a fresh child process: (exit status, stderr, the bytes of --out or None)."""
    args = [os.path.join(FRONT, case, a[1:]) if a.startswith("@") else a for a in flags]
    r = subprocess.run(PROGS[prog] + args + ["--report", "--out", str(out)], capture_output=True, cwd=ROOT, env=dict(os.environ, COLUMNS="80"))
    return r.returncode, r.stderr.decode(), out.read_text() if out.exists() else None


def check_runs(case, runs, tmp_path):
    """Both programs on every run, eight children at a time: the recorded status, stderr and plan file."""
    jobs = [(i, prog) for i in range(len(runs)) for prog in PROGS]
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(lambda j: run(case, runs[j[0]]["flags"], j[1], tmp_path / f"{j[0]}{j[1]}.json"), jobs))
    for (i, prog), (status, err, out) in zip(jobs, got):
        want = runs[i]
        text = want["stderr"][prog] if isinstance(want["stderr"], dict) else want["stderr"]
        assert (status, err, out) == (want["status"], text, want["out"]), (case, prog, want["flags"])


@pytest.mark.parametrize("case", CASES)
def test_the_mappings_are_the_recorded_ones(case):
    """Every field of LogDirsInput and PlaceInput, dtypes included, and the text of every refusal."""
    seen = 0
    for m in load_case(case)["mappings"]:
        got = mappings_of(case, m["args"])
        assert set(got) == set(m) - {"args"}
        for name in got:
            assert got[name] == m[name], (case, m["args"], name)
            seen += 1
    assert seen


@pytest.mark.parametrize("case", CASES)
def test_refused_runs_never_reach_the_device(case, tmp_path):
    """The runs with a status other than 0 are input and usage errors: both programs give the recorded status and stderr and write no
    plan, with or without a device."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cli")], stdout=subprocess.DEVNULL)
    runs = [r for r in load_case(case)["runs"] if r["status"] != 0]
    assert all(r["status"] in (1, 2) and r["out"] is None for r in runs)
    check_runs(case, runs, tmp_path)


def test_the_cases_cover_what_they_are_for():
    cases = {c: load_case(c) for c in CASES}
    places = [m["place"] for c in cases.values() for m in c["mappings"] if "error" not in m["place"]]
    tables = [json.loads(_document(c, n).splitlines()[-1])["brokers"] for c in CASES for n in sorted(os.listdir(os.path.join(FRONT, c))) if n.endswith(".txt")]
    assert 6 <= len(CASES) <= 8 and all(4 <= len(t) <= 6 and all(len(b["logDirs"]) <= 4 for b in t) for t in tables)
    assert any(sum(p["skipped"]) for p in places) and any([] in p["dir_names"] for p in places)                  # a failed dir; a broker with no usable dir
    assert any(-1 in p["dir"]["values"] and any(p["planned"]) for p in places) and any(sum(p["stranded"]) for p in places)   # arrivals; stranded entries
    assert any(sum(p["evacuated"]) for p in places)
    errors = " ".join(m["place"]["error"] for c in cases.values() for m in c["mappings"] if "error" in m["place"])
    for text in ("listed twice", "is not in the current assignment", "lists a broker twice", "is not a usable log dir of a listed broker", "is left without a usable log dir",
                 "empty broker list", "duplicate id in broker list", "twice", "no size for partition"):
        assert text in errors, text
    statuses = [r["status"] for c in cases.values() for r in c["runs"]]
    assert statuses.count(0) >= 30 and statuses.count(1) >= 12 and statuses.count(2) >= 2
    assert any("no capacity for log dirs" in json.dumps(r["stderr"]) for c in cases.values() for r in c["runs"] if r["status"] == 2)


# ---- why one mapping is enough -------------------------------------------------------------------------------------------------------
def random_documents(seed):
    """(current document, log-dirs document, broker list or None): 2-6 brokers with 0-4 dirs each, failed dirs, future entries, entries
    of partitions and brokers that the current document does not hold, rows with brokers that have no dirs, lists with strangers,
    and now and then what is refused: a partition twice on a broker or in the document, an empty list, an id twice."""
    rng = np.random.default_rng(seed)
    ids = sorted(int(b) for b in rng.choice(10, size=int(rng.integers(2, 7)), replace=False))
    names = [(t, p) for t in ("t", "u-x") for p in range(4)]
    rows = [{"topic": t, "partition": p, "replicas": [int(b) for b in rng.choice(ids + [10, 11], size=int(rng.integers(1, 4)), replace=False)]}
            for t, p in names[:6] + [("v", 0)] if rng.random() < 0.8]
    brokers = []
    for b in ids:
        dirs = [{"logDir": f"/d{i}", "error": "IOException" if rng.random() < 0.15 else None, "partitions": []} for i in rng.permutation(6)[:int(rng.integers(0, 5))]]
        for t, p in names:
            row = [r for r in rows if (r["topic"], r["partition"]) == (t, p)]
            for _ in range(2 if rng.random() < 0.03 else 1):   # seldom a second copy
                if dirs and rng.random() < (0.8 if row and b in row[0]["replicas"] else 0.1):
                    dirs[int(rng.integers(0, len(dirs)))]["partitions"].append(
                        {"partition": f"{t}-{p}", "size": int(rng.integers(0, 1 << 40)), "offsetLag": 0, "isFuture": bool(rng.random() < 0.15)})
        brokers.append({"broker": b, "logDirs": dirs})
    if rows and rng.random() < 0.05:
        rows.append(dict(rows[0]))
    lst = None
    if rng.random() < 0.6:
        lst = [int(b) for b in rng.choice(13, size=int(rng.integers(0 if rng.random() < 0.1 else 1, 6)), replace=False)]
        if lst and rng.random() < 0.05:
            lst.append(lst[0])
    return {"version": 1, "partitions": rows}, {"version": 1, "brokers": brokers}, lst


def test_parse_input_is_parse_place_input_without_plan_or_evacuation():
    """On 200 random documents both give the same arrays, dtypes included, or refuse with the same text; every replica is a resident
    on the owner of its dir, nothing is evacuated, stranded or planned.  So the balance call needs no mapping of its own."""
    from kafka_assignment_optimizer_amd.logdirs import parse_input, parse_place_input
    refused = replicas = 0
    for seed in range(200):
        cur, dirs, lst = random_documents(seed)
        got = []
        for call in (lambda: parse_input(cur, dirs, lst), lambda: parse_place_input(cur, dirs, None, (), lst)):
            try:
                got.append(call())
            except ValueError as e:
                got.append(str(e))
        li, pi = got
        if isinstance(li, str) or isinstance(pi, str):
            assert li == pi, seed
            refused += 1
            continue
        a, b = plain(li), plain(pi)
        assert set(a) == {"broker_ids", "dir_names", "skipped", "slots", "keys", "rows", "dir_start", "base", "dir", "size"}
        assert all(a[k] == b[k] for k in a), seed
        assert (np.searchsorted(pi.dir_start, pi.dir, side="right") - 1 == pi.broker).all() and pi.broker.dtype == np.int32
        assert pi.evacuated == [0] * len(pi.broker_ids) == pi.stranded and not any(pi.planned) and len(pi.planned) == len(pi.keys)
        replicas += len(pi.dir)
    print(f"refused {refused} of 200, replicas {replicas}")
    assert 10 <= refused <= 100 and replicas >= 200   # both kinds of document in numbers

"""Arguments the five planner entry points must refuse, by case id, and the call that feeds one case to libkao.so.

Every planner validates before it touches a device, so these calls need no GPU.  tests/golden/make_plan_errors.py records the
return code and the kao_last_error() text of every case into tests/golden/plan_errors.json; tests/test_plan_errors.py replays them.
A case is (entry point, overrides of that entry point's valid base arguments); a value of None is a null pointer."""
import ctypes as C

import numpy as np

NONE = 0xFFFF
MAX_FO_BROKERS = 8000   # KAO_FAILOVER_MAX_BROKERS

ROWS = [[0, 1], [1, 2], [2, 3]]
BASE = {
    "cluster": dict(B=4, P=3, W=2, rows=ROWS, topic_of=[0, 0, 1], T=2, tlo=[0, 0], thi=[2, 2], clo=0, chi=-1, n_changed=0, peak_before=0,
                    peak_after=0, status=0),
    "weighted": dict(B=4, P=3, W=2, rows=ROWS, weight=[1, 2, 3], n_changed=0, peak_before=0, peak_after=0, lower_bound=0, status=0),
    "failover": dict(B=4, R=2, rack_of=[0, 1, 0, 1], P=3, W=2, rows=ROWS, scope=0, scen=0, n_reordered=0),
    "wfailover": dict(B=4, R=2, rack_of=[0, 1, 0, 1], P=3, W=2, rows=ROWS, weight=[1, 2, 3], scope=0, scen=0, n_reordered=0, status=0),
    "leaders": dict(topic=0, B=4, R=2, rack_of=[0, 1, 0, 1], P=3, rf=2, rows=ROWS, lead_lo=-1, lead_hi=-1, w=4, n_changed=0, status=0),
}
OUT_POINTERS = {
    "cluster": ("rows", "topic_of", "tlo", "thi", "n_changed", "peak_before", "peak_after", "status"),
    "weighted": ("rows", "weight", "n_changed", "peak_before", "peak_after", "lower_bound", "status"),
    "failover": ("rack_of", "rows", "scen", "n_reordered"),
    "wfailover": ("rack_of", "rows", "scen", "n_reordered", "weight", "status"),
    "leaders": ("topic", "rows", "n_changed", "status"),
}

# row faults, each at a partition index above 0 (width 3 where an empty slot must be followed by something)
ROW_FAULTS = {
    "slot0_empty": dict(rows=[[0, 1], [NONE, 2], [2, 3]]),
    "broker_after_empty": dict(W=3, rows=[[0, 1, 2], [1, 2, 3], [2, NONE, 3]]),
    "index_too_large": dict(rows=[[0, 1], [1, 4], [2, 3]]),
    "broker_repeated": dict(rows=[[0, 1], [1, 2], [3, 3]]),
}
SLOT_CAP = dict(P=2000001, W=2, rows=[[0, 1]])   # one real row: the call must return before it reads a row
HEAVY = 1 << 61


def _cases():
    c = {}
    for e in ("cluster", "weighted", "failover", "wfailover"):
        for ptr in OUT_POINTERS[e]:
            c[f"{e}/null_{ptr}"] = (e, {ptr: None})
        c[f"{e}/width_0"] = (e, dict(W=0))
        c[f"{e}/width_9"] = (e, dict(W=9))
        c[f"{e}/brokers_0"] = (e, dict(B=0))
        c[f"{e}/brokers_65535"] = (e, dict(B=65535))
        c[f"{e}/partitions_negative"] = (e, dict(P=-1))
        c[f"{e}/slot_cap"] = (e, dict(SLOT_CAP))
        for name, o in ROW_FAULTS.items():
            c[f"{e}/row_{name}"] = (e, dict(o))
        c[f"{e}/two_width_0_brokers_0"] = (e, dict(W=0, B=0))
        c[f"{e}/two_null_rows_width_9"] = (e, dict(rows=None, W=9))
        c[f"{e}/two_slot_cap_row_fault"] = (e, dict(SLOT_CAP, rows=[[NONE, 1]]))
        c[f"{e}/two_row_faults"] = (e, dict(rows=[[0, 1], [1, 1], [NONE, 3]]))
    # kao_balance_leaders_cluster: topics, bands, the cluster band, topic_of
    e = "cluster"
    c[f"{e}/topics_0"] = (e, dict(T=0))
    c[f"{e}/cluster_lo_negative"] = (e, dict(clo=-1))
    c[f"{e}/cluster_hi_below_minus_1"] = (e, dict(chi=-2))
    c[f"{e}/cluster_hi_below_lo"] = (e, dict(clo=2, chi=1))
    c[f"{e}/band_lo_negative"] = (e, dict(tlo=[0, -1]))
    c[f"{e}/band_lo_above_hi"] = (e, dict(tlo=[0, 3], thi=[2, 2]))
    c[f"{e}/topic_of_negative"] = (e, dict(topic_of=[0, -1, 1]))
    c[f"{e}/topic_of_too_large"] = (e, dict(topic_of=[0, 0, 2]))
    c[f"{e}/two_partitions_negative_topics_0"] = (e, dict(P=-1, T=0))
    c[f"{e}/two_slot_cap_band"] = (e, dict(SLOT_CAP, tlo=[3, 0]))
    c[f"{e}/two_cluster_hi_slot_cap"] = (e, dict(SLOT_CAP, chi=-2))
    c[f"{e}/two_band_row"] = (e, dict(tlo=[0, -1], rows=ROW_FAULTS["broker_repeated"]["rows"]))
    c[f"{e}/two_row_then_topic_of"] = (e, dict(rows=ROW_FAULTS["index_too_large"]["rows"], topic_of=[0, 0, 2]))
    c[f"{e}/two_topic_of_and_row_same_partition"] = (e, dict(rows=ROW_FAULTS["index_too_large"]["rows"], topic_of=[0, 5, 1]))
    # the weighted planners: the weight sum
    for e in ("weighted", "wfailover"):
        c[f"{e}/weights_reach_2_62"] = (e, dict(weight=[HEAVY, HEAVY, 0]))
        c[f"{e}/weights_overflow_64_bits"] = (e, dict(weight=[1, (1 << 64) - 1, 5]))
        c[f"{e}/two_slot_cap_weights"] = (e, dict(SLOT_CAP, weight=[1 << 62]))
        c[f"{e}/two_row_fault_then_weights"] = (e, dict(rows=ROW_FAULTS["slot0_empty"]["rows"], weight=[1, HEAVY, HEAVY]))
        c[f"{e}/two_weights_then_row_fault"] = (e, dict(rows=ROW_FAULTS["broker_repeated"]["rows"], weight=[HEAVY, HEAVY, 0]))
    # the failover planners: scope, racks, the broker limit, rack_of
    for e in ("failover", "wfailover"):
        c[f"{e}/scope_negative"] = (e, dict(scope=-1))
        c[f"{e}/scope_2"] = (e, dict(scope=2))
        c[f"{e}/racks_0"] = (e, dict(R=0))
        c[f"{e}/racks_256"] = (e, dict(R=256))
        c[f"{e}/brokers_above_limit"] = (e, dict(B=MAX_FO_BROKERS + 1, rack_of=[0] * (MAX_FO_BROKERS + 1)))
        c[f"{e}/rack_of_too_large"] = (e, dict(rack_of=[0, 1, 2, 1]))
        c[f"{e}/two_scope_width"] = (e, dict(scope=2, W=0))
        c[f"{e}/two_brokers_racks"] = (e, dict(B=0, R=0))
        c[f"{e}/two_racks_partitions"] = (e, dict(R=0, P=-1))
        c[f"{e}/two_slot_cap_brokers_above_limit"] = (e, dict(SLOT_CAP, B=MAX_FO_BROKERS + 1, rack_of=[0] * (MAX_FO_BROKERS + 1)))
        c[f"{e}/two_brokers_above_limit_rack_of"] = (e, dict(B=MAX_FO_BROKERS + 1, rack_of=[9] * (MAX_FO_BROKERS + 1)))
        c[f"{e}/two_rack_of_row"] = (e, dict(rack_of=[0, 1, 0, 7], rows=ROW_FAULTS["slot0_empty"]["rows"]))
    c["wfailover/two_null_weight_scope"] = ("wfailover", dict(weight=None, scope=2))
    c["wfailover/two_rack_of_weights"] = ("wfailover", dict(rack_of=[0, 1, 0, 7], weight=[HEAVY, HEAVY, 0]))
    # kao_balance_leaders: a topic; complete rows only
    e = "leaders"
    for ptr in OUT_POINTERS[e]:
        c[f"{e}/null_{ptr}"] = (e, {ptr: None})
    c[f"{e}/width_0"] = (e, dict(rf=0))
    c[f"{e}/width_9"] = (e, dict(rf=9))
    c[f"{e}/brokers_0"] = (e, dict(B=0))
    c[f"{e}/brokers_65535"] = (e, dict(B=65535))
    c[f"{e}/partitions_negative"] = (e, dict(P=-1))
    c[f"{e}/partitions_0"] = (e, dict(P=0))
    c[f"{e}/racks_0"] = (e, dict(R=0))
    c[f"{e}/racks_256"] = (e, dict(R=256))
    c[f"{e}/rack_of_too_large"] = (e, dict(rack_of=[0, 1, 2, 1]))
    c[f"{e}/rf_above_brokers"] = (e, dict(B=1, rack_of=[0]))
    # (validate() reads topic.current before it reaches the cap, and stops at the 24-bit objective first unless the weights are 0:
    # current is whole, the assignment passed is the one real row)
    c[f"{e}/slot_cap"] = (e, dict(P=2000001, rf=2, rows=[[0, 1]], w=0))
    c[f"{e}/objective_24_bits"] = (e, dict(P=2000001, rf=2, rows=[[0, 1]], w=5))
    c[f"{e}/band_lo_above_hi"] = (e, dict(lead_lo=2, lead_hi=1))
    c[f"{e}/row_slot_empty"] = (e, dict(rows=[[0, 1], [1, 2], [2, NONE]]))
    c[f"{e}/row_index_too_large"] = (e, dict(rows=[[0, 1], [1, 4], [2, 3]]))
    c[f"{e}/row_broker_repeated"] = (e, dict(rows=[[0, 1], [1, 2], [3, 3]]))
    c[f"{e}/two_null_rows_width_0"] = (e, dict(rows=None, rf=0))
    c[f"{e}/two_band_row"] = (e, dict(lead_lo=2, lead_hi=1, rows=[[0, 1], [1, 1], [2, 3]]))
    c[f"{e}/two_row_faults"] = (e, dict(rows=[[0, 1], [1, 1], [NONE, 3]]))
    c[f"{e}/two_index_and_repeat_in_one_row"] = (e, dict(rows=[[0, 1], [7, 7], [2, 3]]))
    return c


CASES = _cases()


def _ptr(arr, ctype):
    return None if arr is None else arr.ctypes.data_as(C.POINTER(ctype))


def call(lib, case_id):
    """(return code, kao_last_error() text, rows buffer unchanged) of one case."""
    from kafka_assignment_optimizer_amd import _ffi
    entry, over = CASES[case_id]
    a = dict(BASE[entry], **over)
    null = {k for k in OUT_POINTERS[entry] if a[k] is None}
    rows = None if "rows" in null else np.array(a["rows"], dtype=np.uint16).reshape(-1)
    before = None if rows is None else rows.copy()
    i32 = lambda name, n=1: None if name in null else np.zeros(n, dtype=np.int32)      # noqa: E731
    u64 = lambda name, n=1: None if name in null else np.zeros(n, dtype=np.uint64)     # noqa: E731
    arr = lambda name, dt: None if name in null else np.array(a[name], dtype=dt).reshape(-1)   # noqa: E731
    stats32, stats64 = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int64)
    n_scen = max(a.get("B", 1), a.get("R", 1), 1)
    if entry == "cluster":
        outs = [i32("n_changed"), i32("peak_before"), i32("peak_after"), i32("status")]
        rc = lib.kao_balance_leaders_cluster(a["B"], a["P"], a["W"], _ptr(rows, C.c_uint16), _ptr(arr("topic_of", np.int32), C.c_int32), a["T"],
                                             _ptr(arr("tlo", np.int32), C.c_int32), _ptr(arr("thi", np.int32), C.c_int32), a["clo"], a["chi"], 0,
                                             *[_ptr(o, C.c_int32) for o in outs], _ptr(stats32, C.c_int32))
    elif entry == "weighted":
        rc = lib.kao_balance_leaders_weighted(a["B"], a["P"], a["W"], _ptr(rows, C.c_uint16), _ptr(arr("weight", np.uint64), C.c_uint64), 0, 0, 0,
                                              _ptr(i32("n_changed"), C.c_int32), _ptr(u64("peak_before"), C.c_uint64),
                                              _ptr(u64("peak_after"), C.c_uint64), _ptr(u64("lower_bound"), C.c_uint64),
                                              _ptr(i32("status"), C.c_int32), _ptr(stats64, C.c_int64))
    elif entry == "failover":
        rc = lib.kao_failover_order(a["B"], a["R"], _ptr(arr("rack_of", np.uint8), C.c_uint8), a["P"], a["W"], _ptr(rows, C.c_uint16), a["scope"], 0,
                                    _ptr(i32("scen", 5 * n_scen), C.c_int32), _ptr(i32("n_reordered"), C.c_int32), _ptr(stats32, C.c_int32))
    elif entry == "wfailover":
        rc = lib.kao_failover_order_weighted(a["B"], a["R"], _ptr(arr("rack_of", np.uint8), C.c_uint8), a["P"], a["W"], _ptr(rows, C.c_uint16),
                                             _ptr(arr("weight", np.uint64), C.c_uint64), a["scope"], 0, 0, 0, _ptr(u64("scen", 6 * n_scen), C.c_uint64),
                                             _ptr(i32("n_reordered"), C.c_int32), _ptr(i32("status"), C.c_int32), _ptr(stats64, C.c_int64))
    else:
        rack_of = np.array(a["rack_of"], dtype=np.uint8)
        current = np.resize(np.array(ROWS, dtype=np.uint16), max(a["P"], 1) * max(a["rf"], 1))   # the base rows over and over
        t = _ffi.KaoTopic(n_brokers=a["B"], n_racks=a["R"], n_partitions=a["P"], rf=a["rf"], rf_cur=a["rf"], rack_of=_ptr(rack_of, C.c_uint8),
                          current=_ptr(current, C.c_uint16), rep_lo=-1, rep_hi=-1, lead_lo=a["lead_lo"], lead_hi=a["lead_hi"], rack_lo=-1,
                          rack_hi=-1, prack_lo=-1, prack_hi=-1)
        t.w[0][0], t.w[0][1], t.w[1][0], t.w[1][1] = a["w"], a["w"] // 2, a["w"] // 2, a["w"] // 4
        obj = C.c_int64(0)
        rc = lib.kao_balance_leaders(None if "topic" in null else C.byref(t), _ptr(rows, C.c_uint16), _ptr(i32("n_changed"), C.c_int32),
                                     C.byref(obj), _ptr(i32("status"), C.c_int32), _ptr(stats32, C.c_int32))
    text = lib.kao_last_error().decode()
    return int(rc), text, rows is None or bool((rows == before).all())

"""K-eval on every path it dispatches (run on the MI355X box with -m gpu), against the scalar restatement kao_port.port_eval:
objective and all eight violation counts, exact equality.

  * the RF-3 stream instantiation k_eval<4,false,3> on trips whose 64 partitions are all filled -- the branch every candidate of
    K-search and KAO-CX takes, with its C7 shortcut (one / two / three racks per partition, prack_lo 0 and above 0);
  * filled and holed trips inside one candidate, and alternating between the consecutive candidates of one wavefront;
  * many candidates per wavefront (the counters are zeroed between them), RF 3, RF 6 and broker weights;
  * one evaluation plan over several batch sizes with device buffers: the block map rebuilt, the switch between the cooperative
    and the one-wavefront kernel, the packed best key (lowest id on ties, no feasible candidate);
  * kao_evaluate_batch in chunks of 2^20 candidates.
"""
import functools

import numpy as np
import pytest

from conftest import random_candidates, to_product_topic

pytestmark = pytest.mark.gpu

INVALID = -1      # KAO_ERR_INVALID
KEY_NONE = -1     # ~0ull as int64: no candidate seen


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


def port_all(kp, ot, cands):
    """port_eval of every candidate -> (objective [n] int64, violations [n, 8] int64); one C topic for the whole batch."""
    import ctypes as C
    ct = kp.CTopic(ot)
    fn = kp.lib().kao_port_eval
    c = np.ascontiguousarray(cands, dtype=np.uint16).reshape(len(cands), -1)
    assert c.shape[1] == ot.n_partitions * ot.rf
    obj = np.zeros(len(c), dtype=np.int64)
    viol = np.zeros((len(c), 8), dtype=np.int32)
    o = C.c_int64()
    for i in range(len(c)):
        rc = fn(C.byref(ct.s), c[i].ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(o), viol[i].ctypes.data_as(C.POINTER(C.c_int32)))
        assert rc == 0
        obj[i] = o.value
    return obj, viol.astype(np.int64)


def assert_equal_to_port(kp, ot, cands, obj, viol, what):
    po, pv = port_all(kp, ot, cands)
    bad = np.flatnonzero((np.asarray(obj, dtype=np.int64) != po) | (np.asarray(viol, dtype=np.int64) != pv).any(axis=1))
    assert bad.size == 0, (what, len(bad), [(int(i), int(obj[i]), np.asarray(viol[i]).tolist(), int(po[i]), pv[i].tolist()) for i in bad[:4]])
    return po, pv


def expected_key(po, pv):
    """The packed best key of a batch from the port's values: violation | inverted objective | id, the minimum over the batch."""
    return min((min(int(v[0]), 0xFFFFF) << 44) | ((0xFFFFFF - min(int(o), 0xFFFFFF)) << 20) | i for i, (o, v) in enumerate(zip(po, pv)))


# ------------------------------------------------------------------------------- a. all-filled trips, RF-3 stream instantiation
# (B0, R, P, removed, added, bounds_override): RF = current RF = 3, so the current assignment is staged in LDS
FULL_SHAPES = [
    (12, 1, 70, [], [], None),
    (12, 2, 65, [3], [(12, 0)], None),
    (12, 3, 64, [], [(12, 1)], None),
    (20, 5, 130, [4], [(20, 2)], None),
    (20, 5, 130, [4], [(20, 2)], {"prack_lo": 1, "prack_hi": 1}),
    (20, 5, 130, [4], [(20, 2)], {"prack_lo": 0, "prack_hi": 3}),
    (150, 75, 63, [], [], None),         # more than 64 racks: one copy of the rack counters
    (9, 3, 1, [], [], None),
]


@functools.lru_cache(maxsize=None)
def full_case(i):
    """-> (oracle topic, 39 complete candidates [39, P, 3]) of FULL_SHAPES[i]."""
    import kao_oracle as ko
    B0, R, P, removed, added, bo = FULL_SHAPES[i]
    ot = ko.make_cluster("full", B0, R, 1, P, 3, removed, added, bounds_override=bo).topics[0]
    cands = random_candidates(ot, 40, R * 1000 + P, p_mut=0.3, p_none=0.0)[1:]   # candidate 0 keeps the holes of `current`
    cands.setflags(write=False)
    return ot, cands


def rack_classes(ot, cands):
    """Partitions of the candidates on one / two / three racks, and with a repeated broker."""
    rk = np.asarray(ot.rack_of, dtype=np.int64)[cands.astype(np.int64)]
    e01, e02, e12 = rk[..., 0] == rk[..., 1], rk[..., 0] == rk[..., 2], rk[..., 1] == rk[..., 2]
    one = e01 & e12
    two = (e01 | e02 | e12) & ~one
    c = cands.astype(np.int64)
    rep = (c[..., 0] == c[..., 1]) | (c[..., 0] == c[..., 2]) | (c[..., 1] == c[..., 2])
    return int(one.sum()), int(two.sum()), int((~one & ~two).sum()), int(rep.sum())


def test_full_trip_inputs_cover_every_rack_class():
    """What test_full_trips_rf3_stream feeds the device: partitions on one, two and three racks (the three constants of the C7
    shortcut) and repeated brokers (C5) all occur.  Counted here: 3,286 / 8,101 / 14,080 and 2,333."""
    tot = np.zeros(4, dtype=np.int64)
    for i in range(len(FULL_SHAPES)):
        tot += rack_classes(*full_case(i))
    assert tot[0] >= 50 and tot[1] >= 50 and tot[2] >= 50 and tot[3] >= 100, tot.tolist()


@pytest.mark.parametrize("i", range(len(FULL_SHAPES)))
def test_full_trips_rf3_stream(kao, ko, kp, i):
    ot, cands = full_case(i)
    assert ot.rf == 3 and ot.rf_cur == 3
    assert int(cands.max()) < ot.n_brokers          # every slot filled: every trip takes the all-filled branch
    obj, viol = kao.evaluate_batch(to_product_topic(ot), cands)
    assert_equal_to_port(kp, ot, cands, obj, viol, FULL_SHAPES[i])
    for j in range(0, len(cands), 7):
        o, v = ko.verify(ot, cands[j])
        assert (int(obj[j]), viol[j].tolist()) == (o, v.tolist()), (FULL_SHAPES[i], j)


# ------------------------------------------------------------------------------- b. mixed trips
def test_mixed_trips_alternate_inside_a_wavefront(kao, ko, kp, fill):
    """130 partitions are two full trips and a 2-lane tail.  Exactly one slot of a complete candidate is emptied (0xFFFF) or put
    out of range (B + 7): in trip 0 only, in trip 1 only, in the tail only, or in a leader slot (C2).  Candidates ci, ci + 4, ...
    go to one wavefront; blocks of four complete candidates alternate with blocks of four holed ones, so every wavefront takes
    the all-filled branch and the general one in turn (eight candidates per wavefront at this batch size)."""
    ot = full_case(3)[0]
    B, P = ot.n_brokers, ot.n_partitions
    n = 8192 + 40
    assert n >= 8 * fill                            # then kao_eval_plan_run puts 32 candidates in a workgroup: eight per wavefront
    cands = random_candidates(ot, n + 1, 77, p_mut=0.3, p_none=0.0)[1:].copy()
    assert int(cands.max()) < B
    holed = (np.arange(n) // 4) % 2 == 1
    for i in np.flatnonzero(holed):
        kind = (i // 8) % 8
        bad = 0xFFFF if kind < 4 else B + 7
        p, k = [(i % 64, i % 3), (64 + i % 64, (i + 1) % 3), (128 + i % 2, (i + 2) % 3), ((i * 7) % P, 0)][kind % 4]
        cands[i, p, k] = bad
    assert ((cands >= B).sum(axis=(1, 2)) == holed).all()
    obj, viol = kao.evaluate_batch(to_product_topic(ot), cands)
    po, pv = assert_equal_to_port(kp, ot, cands, obj, viol, "mixed trips")
    assert (pv[:, 1] == holed).all() and (pv[:, 2] == (cands[:, :, 0] >= B).sum(axis=1)).all() and pv[:, 2].sum() >= n // 8
    for j in range(0, n, 211):
        o, v = ko.verify(ot, cands[j])
        assert (int(obj[j]), viol[j].tolist()) == (o, v.tolist()), j


# ------------------------------------------------------------------------------- c. many candidates per wavefront
def many_topic(ko, which):
    if which == "rf6":
        return ko.make_cluster("rf6", 30, 5, 1, 36, 6, [3, 7], [(30, 3), (31, 2)]).topics[0]
    ot = ko.make_cluster("rf3", 20, 5, 1, 130, 3, [4], [(20, 2)]).topics[0]
    if which == "rf3_weights":
        rng = np.random.default_rng(5)
        ot.broker_w = rng.integers(0, 6, ot.n_brokers).astype(np.int32)
        ot.broker_wl = rng.integers(0, 4, ot.n_brokers).astype(np.int32)
    return ot


@pytest.mark.parametrize("which", ["rf3", "rf6", "rf3_weights"])
def test_many_candidates_per_wavefront(kao, ko, kp, fill, which):
    """8,205 distinct candidates in one call: 32 per workgroup, eight in a row per wavefront, a partial last workgroup.  Half of
    them complete, half with a few empty or out-of-range slots; every result is compared."""
    ot = many_topic(ko, which)
    n = 8192 + 13
    assert n >= 8 * fill                            # 32 candidates per workgroup (kao_eval_plan_run), eight per wavefront
    full = random_candidates(ot, n + 1, 31, p_mut=0.3, p_none=0.0)[1:]
    some = random_candidates(ot, n + 1, 32, p_mut=0.3, p_none=0.004)[1:]
    pick = np.random.default_rng(33).random(n) < 0.5
    cands = np.where(pick[:, None, None], some, full)
    n_holed = int(((cands >= ot.n_brokers).sum(axis=(1, 2)) > 0).sum())
    assert n // 5 < n_holed < n // 2 and len(np.unique(cands.reshape(n, -1), axis=0)) == n
    obj, viol = kao.evaluate_batch(to_product_topic(ot), cands)
    assert_equal_to_port(kp, ot, cands, obj, viol, which)


# ------------------------------------------------------------------------------- d. one plan, device buffers, best key
# The plan's buffers are torch tensors.  torch brings its own copy of the HIP runtime, which finds no device once libkao.so has
# initialised the system's copy in the same process, while libkao.so loaded after torch shares torch's copy
# (observed: after kao.init, torch.cuda.get_device_properties(0) raises "RuntimeError: No HIP GPUs are available" in this process;
# torch.cuda.device_count(), which test_gpu_parity.py calls in-process, does not initialise torch's runtime).  The checks of this
# section therefore run in one child process that imports torch first (`python tests/test_gpu_eval_paths.py`, as
# test_gpu_parity.py::test_allreduce_best_resident_matches_host_packing does); the three tests below read its verdicts.
class PlanRunner:
    """One kao.EvalPlan with torch buffers; run() returns what the device wrote."""

    def __init__(self, kao, pt, per, cap):
        import torch
        self.torch, self.plan, self.per, self.cap = torch, kao.EvalPlan(pt), per, cap
        self.obj = torch.empty(cap + 8, dtype=torch.int32, device="cuda")
        self.viol = torch.empty((cap + 8, 8), dtype=torch.int32, device="cuda")
        self.key = torch.empty(1, dtype=torch.int64, device="cuda")

    def run(self, cands):
        torch = self.torch
        n = len(cands)
        assert n <= self.cap
        d_c = torch.from_numpy(np.ascontiguousarray(cands, dtype=np.uint16).reshape(n, self.per).view(np.int16)).cuda()
        self.obj.fill_(-7); self.viol.fill_(-7); self.key.fill_(KEY_NONE)
        torch.cuda.synchronize()                      # the plan's stream does not wait for torch's
        self.plan.run(d_c.data_ptr(), n, self.obj.data_ptr(), self.viol.data_ptr(), self.key.data_ptr())
        self.plan.sync()
        obj, viol = self.obj.cpu().numpy(), self.viol.cpu().numpy()
        assert (obj[n:] == -7).all() and (viol[n:] == -7).all()    # nothing written past the batch (a stale block map would)
        return obj[:n], viol[:n], int(self.key.cpu()[0]) & (2 ** 64 - 1)


def feasible_fill(ko, ot):
    for t in (1, 2, 3, 5, 7):
        a = ko.balanced_fill(ot.n_brokers, ot.n_racks, ot.n_partitions, ot.rf, t, [int(r) for r in ot.rack_of])
        if ko.verify(ot, a)[1][0] == 0:
            return a
    raise AssertionError("no feasible balanced fill")


def device_fill():
    """Candidates that give every SIMD of the device one wavefront (what kao_eval_plan_run sizes its workgroups by)."""
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def plan_batch_sizes(kao, ko, kp):
    """P = 1100 is above the cooperative threshold (1024): batches of more than `fill` candidates take the one-wavefront kernel,
    smaller ones the cooperative kernel, on the same plan, whose block map is rebuilt whenever n changes."""
    ot = ko.make_cluster("plan", 60, 3, 1, 1100, 3, [7], [(60, 1)]).topics[0]
    P, per = ot.n_partitions, ot.n_partitions * ot.rf
    good = feasible_fill(ko, ot)
    fill = device_fill()
    big = fill + 76
    runner = PlanRunner(kao, to_product_topic(ot), per, big)
    try:
        # run 1: the one-wavefront kernel, ceil(big / fill) = 2 candidates per wavefront (fill > 76); no feasible candidate
        assert fill > 76
        c1 = random_candidates(ot, big + 1, 41, p_mut=0.05, p_none=0.0005)[1:]
        obj, viol, key = runner.run(c1)
        po, pv = assert_equal_to_port(kp, ot, c1, obj, viol, "run 1")
        assert pv[:, 0].min() > 0
        assert key == expected_key(po, pv) and key >> 44 == pv[:, 0].min()
        # run 2: five candidates, the cooperative kernel; the feasible one wins
        c2 = random_candidates(ot, 6, 42, p_mut=0.05, p_none=0.0005)[1:].copy()
        c2[3] = good
        obj, viol, key = runner.run(c2)
        po, pv = assert_equal_to_port(kp, ot, c2, obj, viol, "run 2")
        assert key == expected_key(po, pv) and key >> 44 == 0 and key & 0xFFFFF == 3
        # run 3: the first size again with other candidates; the best one sits at two ids in different workgroups: the lower wins
        c3 = random_candidates(ot, big + 1, 43, p_mut=0.05, p_none=0.0005)[1:].copy()
        c3[fill + 9] = good
        c3[37] = good
        obj, viol, key = runner.run(c3)
        po, pv = assert_equal_to_port(kp, ot, c3, obj, viol, "run 3")
        assert (po[37], pv[37].tolist()) == (po[fill + 9], pv[fill + 9].tolist()) and pv[37, 0] == 0
        assert key == expected_key(po, pv) and key & 0xFFFFF == 37
        # run 4: a single candidate
        c4 = c1[11:12]
        obj, viol, key = runner.run(c4)
        po, pv = assert_equal_to_port(kp, ot, c4, obj, viol, "run 4")
        assert key == expected_key(po, pv) and key & 0xFFFFF == 0
        # batch sizes outside 1 .. 2^20 are refused before anything is launched
        import torch
        d_c = torch.zeros(per, dtype=torch.int16, device="cuda")
        for n in (0, 2 ** 20 + 1):
            with pytest.raises(kao.KaoError) as e:
                runner.plan.run(d_c.data_ptr(), n, runner.obj.data_ptr(), runner.viol.data_ptr(), runner.key.data_ptr())
            assert e.value.code == INVALID
    finally:
        runner.plan.close()


def plan_cooperative_70_racks(kao, ko, kp, weights):
    """70 racks (one copy of the rack counters) and exactly 1024 partitions, three candidates: the cooperative kernel."""
    ot = ko.make_cluster("coop", 140, 70, 1, 1024, 3, [], []).topics[0]
    if weights:
        rng = np.random.default_rng(6)
        ot.broker_w = rng.integers(0, 6, ot.n_brokers).astype(np.int32)
        ot.broker_wl = rng.integers(0, 4, ot.n_brokers).astype(np.int32)
    cands = random_candidates(ot, 4, 51, p_mut=0.2, p_none=0.001)[1:].copy()
    cands[2][cands[2] >= ot.n_brokers] = 0          # one complete candidate
    runner = PlanRunner(kao, to_product_topic(ot), ot.n_partitions * ot.rf, 3)
    try:
        obj, viol, key = runner.run(cands)
        po, pv = assert_equal_to_port(kp, ot, cands, obj, viol, "cooperative, 70 racks")
        assert key == expected_key(po, pv)
    finally:
        runner.plan.close()
    o, v = ko.verify(ot, cands[2])
    assert (int(obj[2]), viol[2].tolist()) == (o, v.tolist())


PLAN_CHECKS = {
    "batch_sizes": lambda kao, ko, kp: plan_batch_sizes(kao, ko, kp),
    "cooperative_70_racks": lambda kao, ko, kp: plan_cooperative_70_racks(kao, ko, kp, False),
    "cooperative_70_racks_weights": lambda kao, ko, kp: plan_cooperative_70_racks(kao, ko, kp, True),
}


@pytest.fixture(scope="module")
def plan_child():
    """stdout + stderr of the child process that runs PLAN_CHECKS."""
    import subprocess, sys
    out = subprocess.run([sys.executable, __file__], capture_output=True, text=True, timeout=300)
    return out.stdout[-6000:] + out.stderr[-3000:]


@pytest.fixture(scope="module")
def fill(plan_child):
    """4 x compute units, as the child read it from torch: what kao_eval_plan_run sizes its workgroups by."""
    import re
    m = re.search(r"^plan-fill (\d+)$", plan_child, re.M)
    assert m, plan_child
    return int(m.group(1))


@pytest.mark.parametrize("check", list(PLAN_CHECKS))
def test_eval_plan_with_device_buffers(plan_child, check):
    assert f"plan-ok {check}\n" in plan_child, plan_child


# ------------------------------------------------------------------------------- e. kao_evaluate_batch above 2^20 candidates
def test_evaluate_batch_chunks_above_2_to_20(kao, ko, kp):
    """2^20 + 77 candidates go to the device in two chunks; 997 distinct ones tiled (2^20 is no multiple of 997, so the second
    chunk starts inside a period): candidate i has the port's value of candidate i mod 997."""
    ot = ko.make_cluster("tiny", 8, 2, 1, 4, 1, [], []).topics[0]
    values = np.array(list(range(8)) + [0xFFFF, 8 + 7], dtype=np.uint16)
    codes = np.arange(997) * 7 + 3                  # < 10^4: four distinct base-10 digit strings
    base = values[(codes[:, None] // 10 ** np.arange(4)[None, :]) % 10].reshape(997, 4, 1)
    assert len(np.unique(base.reshape(997, -1), axis=0)) == 997
    n = 2 ** 20 + 77
    idx = np.arange(n) % 997
    obj, viol = kao.evaluate_batch(to_product_topic(ot), base[idx])
    po, pv = port_all(kp, ot, base)
    assert (obj.astype(np.int64) == po[idx]).all()
    assert (viol.astype(np.int64) == pv[idx]).all()


if __name__ == "__main__":
    import traceback
    import torch
    torch.cuda.set_device(0)                     # torch's HIP runtime first (see section d)
    import kafka_assignment_optimizer_amd as kao_mod
    import kao_oracle
    import kao_port
    kao_mod.init(0)
    assert "gfx950" in kao_mod.device_name(), kao_mod.device_name()
    kao_port.build()
    print(f"plan-fill {device_fill()}", flush=True)
    for name, check in PLAN_CHECKS.items():
        try:
            check(kao_mod, kao_oracle, kao_port)
            print(f"plan-ok {name}", flush=True)
        except Exception:
            traceback.print_exc()
            print(f"plan-FAILED {name}", flush=True)

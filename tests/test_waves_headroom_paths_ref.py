"""CPU checks of what tests/test_gpu_waves_headroom_paths.py relies on: every instance of tests/headroom_paths_cases.py goes
through the sequential reference and its independent checker, and has the property it exists for -- the clamped least free
bytes tie, the broker beyond the workgroup is the one that fills, the ties fall where the kernel's loops and reductions decide
them, capacity binds on the wide rows and the mid-size plan, and the conveyors take the waves their round count is derived from."""
import functools

import numpy as np
import pytest

import headroom_paths_cases as hc
import waves_headroom_ref as hr
import waves_paths_cases as wc
import waves_ref as wr

I64_MAX = (1 << 63) - 1


@functools.lru_cache(maxsize=None)
def _cases():
    return {c[0]: c for c in hc.all_cases()}


@functools.lru_cache(maxsize=None)
def _run(name):
    """(wave, n_waves, lower_bound, stats) of the model, checked."""
    _, cur, tgt, size, stored, capacity, C, k, seed = _cases()[name]
    wave, nw, lb, stats = hr.model(cur, tgt, size, stored, capacity, C, k, seed)
    assert hr.check_headroom(cur, tgt, size, stored, capacity, C, k, wave, nw, lb) == stats[0]
    assert stats[3] == 64
    return wave.tolist(), nw, lb, stats


def test_names_are_unique_and_every_family_is_there():
    names = [c[0] for c in hc.all_cases()]
    assert len(names) == len(set(names)) == 3 + 2 + 4 + 42 + 4 + 3
    assert set(hc.SHAPE_NAMES) == {n for n in names if "@" in n and not n.split("@")[0] in hc.MID}
    assert len(hc.sized_shape_cases()) == 14 and not any(c[0].endswith("/count") for c in hc.sized_shape_cases())


def test_clamped_free_bytes_tie_at_the_first_wave_and_the_lowest_broker():
    wave, nw, _, stats = _run("clamp/all")
    assert (wave, nw, stats[0]) == ([0, 0, 0], 1, 0) and stats[5:] == [I64_MAX, 0, 1]
    # unclamped, broker 2 has the fewest free bytes: comparing before the clamp reports it
    _, _, _, size, stored, capacity, *_ = _cases()["clamp/all"]
    free = {b: capacity[b] - stored[b] - a for b, a in ((1, 10), (2, 15))}
    assert I64_MAX < free[2] < free[1] and min(capacity) > hr.UNLIMITED
    wave, nw, _, stats = _run("clamp/control")
    assert (wave, nw) == ([0, 0, 0], 1) and stats[5:] == [(1 << 63) - 115, 0, 2]
    wave, nw, _, stats = _run("clamp/waves")
    assert (wave, nw, stats[2]) == ([0, 1], 2, 0) and stats[5:] == [I64_MAX, 0, 1]
    _, _, _, size, stored, capacity, *_ = _cases()["clamp/waves"]
    assert I64_MAX < capacity[2] - stored[2] - 10 < capacity[1] - stored[1] - 10     # the later wave has fewer, unclamped


@pytest.mark.parametrize("name, B, last", [("wide/1000", 1000, 999), ("wide/257", 257, 256)])
def test_the_broker_beyond_the_workgroup_fills_over_four_waves(name, B, last):
    case = _cases()[name]
    assert len(case[4]) == len(case[5]) == B and case[1].shape == (5, 1) and int(case[2].max()) == last
    wave, nw, lb, stats = _run(name)
    assert (wave, nw, lb) == ([0, 1, 2, 3, 0], 4, 4)
    assert stats[5:] == [(1 << 40) - 28, 3, last]
    assert len(wr.classify(case[1], case[2])[1]) <= 256     # one workgroup per order: the row clear strides


@pytest.mark.parametrize("name, wave, least", [("tie/thread", [0, 0], [40, 0, 44]), ("tie/threads", [0, 0], [40, 0, 45]),
                                               ("tie/strict", [0, 0, 0], [39, 0, 999]), ("tie/waves", [0, 1], [40, 0, 44])])
def test_least_free_ties(name, wave, least):
    got, nw, _, stats = _run(name)
    assert got == wave and nw == max(wave) + 1 and stats[0] == 0
    assert stats[5:] == least
    assert len(_cases()[name][4]) == 1000
    tgt = sorted(_cases()[name][2][:, 0].tolist())
    if name == "tie/thread":
        assert tgt[1] - tgt[0] == 256
    if name == "tie/threads":
        assert tgt[0] % 256 != tgt[1] % 256


def _sized_waves(name):
    """n_waves of kao_plan_waves_sized on the rows of a shape or mid case: capacity out of the picture."""
    base = name.split("@")[0]
    case = wc.mid_case(base) if base in hc.MID else next(c for c in wc.shape_cases() if c[0] == base)
    return wc.run_model(case)[1]


def test_capacity_binds_on_the_row_shapes():
    _, nw, _, stats = _run("nine/C0@120")
    assert stats[0] == 0 and stats[2] == 5 and nw == 10 and _sized_waves("nine/C0@120") == 9
    case = _cases()["nine/C0@120"]
    assert case[1].shape[1] == 8 and max(len(s) for s in wr.classify(case[1], case[2])[1]) == 9
    assert _run("nine/C0@110")[3][0] == 11 and _run("nine/C2@110")[3][0] == 11
    assert (_run("nosource/C0@100")[3][0], _run("nosource/C0@100")[3][2]) == (2, 3)
    assert _run("moving256/C0@100")[3][2] == 48
    stuck, slower, winners = 0, 0, set()
    for name in hc.SHAPE_NAMES:
        _, nw, _, stats = _run(name)
        winners.add(stats[2])
        stuck += stats[0] > 0
        slower += stats[0] == 0 and nw > _sized_waves(name)
    assert stuck >= 1 and slower >= 1 and len(winners) >= 5


def test_row_shape_cases_keep_their_rows():
    """No source with followers, RF changes both ways, 255 / 256 / 257 moving partitions and the three seeds, as in
    tests/test_waves_cap_ref.py, reach the headroom planner."""
    names = {n.split("@")[0] for n in hc.SHAPE_NAMES}
    assert {"nine/C0", "nine/C2", "padded/C0", "nosource/C0", "nosource/C2", "rfchange/C0", "rfchange/C2"} <= names
    assert {f"moving{n}/C0" for n in (255, 256, 257)} <= names
    assert {c[8] for n, c in _cases().items() if n.startswith("seed")} == {0, 1 << 63, (1 << 64) - 1}
    cur = _cases()["nosource/C0@100"][1]
    assert any(cur[p, 0] == wc.NONE and (cur[p, 1:3] != wc.NONE).all() for p in range(len(cur)))
    for n in (255, 256, 257):
        c = _cases()[f"moving{n}/C0@100"]
        assert sum(1 for s in wr.classify(c[1], c[2])[1] if s) == n


@pytest.mark.parametrize("name, stuck, n_waves, lb, winner, least", [
    ("loguniform/C2", 25, 47, 48, 0, (0, 41)), ("equal/C0", 0, 21, 17, 32, (0, None)),
    ("oversized/C2", 0, 49, None, 1, None), ("zeros/02", 19, None, None, None, None)])
def test_mid_plans(name, stuck, n_waves, lb, winner, least):
    full = f"{name}@{hc.MID[name]}"
    case = _cases()[full]
    assert sum(1 for s in wr.classify(case[1], case[2])[1] if s) == 1000 and len(case[4]) == 40
    _, nw, got_lb, stats = _run(full)
    assert stats[0] == stuck
    assert n_waves is None or nw == n_waves
    assert lb is None or got_lb == lb
    assert winner is None or stats[2] == winner
    if least:
        assert stats[5] == least[0] and (least[1] is None or stats[6] == least[1])


def test_conveyors_take_one_partition_per_wave_in_every_order():
    for case, done_round, launches in hc.conveyor_cases():
        name, cur, tgt, size, stored, capacity, C, k, seed = case
        fork = name.endswith("+fork")
        n = int(name.split("/")[1].split("+")[0])
        wave, nw, _, stats = _run(name)
        want = [n - i if fork else n - 1 - i for i in range(n)] + ([0, 0] if fork else [])
        assert wave == want and nw == (n + 1 if fork else n) and stats[0] == 0
        # two rounds per wave, three for the wave whose two partitions share a source, and the idle wave's one
        assert done_round == 2 * nw + (1 if fork else 0) and launches == 32 * (done_round // 32 + 1)
        cls, parts, traf = hr.traffic(cur, tgt, size)
        ar = hr.add_rem(cur, tgt)
        for o in range(64):
            wv, onw, _ = hr.run_order(cls, parts, traf, ar, size, stored, capacity, C, k, hr.sized_order(parts, traf, o, seed))
            assert [wv[p] for p in range(len(want))] == want and onw == nw, (name, o)
    assert [(d, l) for _, d, l in hc.conveyor_cases()] == [(30, 32), (31, 32), (32, 64)]

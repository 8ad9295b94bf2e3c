"""CPU tests of KAO-CX's host side: how a squaring is split over the midpoints (kao_cycle_square_plan: the function Cx::square()
itself calls; needs no device), the test hook KAO_CX_SQUARE_SPLIT that steers it, and the node limit, which is refused before
any device call."""
import numpy as np
import pytest

from test_gpu_cycle import _drifted

HOOK = "KAO_CX_SQUARE_SPLIT"


def _production(n):
    """The rule as DESIGN.md states it: below 200 tiles of 64 x 64 outputs, about 512 workgroups in 2..8 slices of a multiple of 16
    midpoints; from 200 tiles on one unsplit launch."""
    np_ = (n + 63) // 64 * 64
    tiles = (np_ // 64) ** 2
    ks = min(8, max(2, -(-512 // tiles))) if tiles < 200 else 1
    kchunk = -(-(-(-np_ // ks)) // 16) * 16
    return np_, -(-np_ // kchunk), kchunk


def test_square_plan_of_the_production_rule(monkeypatch):
    import kafka_assignment_optimizer_amd as kao
    for value in (None, "0", ""):
        monkeypatch.delenv(HOOK, raising=False) if value is None else monkeypatch.setenv(HOOK, value)
        assert kao.cycle_square_plan(186) == (192, 6, 32)
        assert kao.cycle_square_plan(317) == (320, 7, 48)          # 6 x 48 + 32: the last slice is shorter
        assert kao.cycle_square_plan(51) == (64, 4, 16) and kao.cycle_square_plan(107) == (128, 8, 16)
        for n in (897, 949, 2048):
            assert kao.cycle_square_plan(n) == ((n + 63) // 64 * 64, 1, (n + 63) // 64 * 64)
        for n in range(1, 2049):
            np_, ks, kchunk = kao.cycle_square_plan(n)
            assert (np_, ks, kchunk) == _production(n)
            assert kchunk % 16 == 0 and ks * kchunk >= np_ > (ks - 1) * kchunk      # the slices cover every midpoint, none is empty
            assert (ks == 1) == (np_ >= 960)


def test_square_plan_under_the_test_hook(monkeypatch):
    import kafka_assignment_optimizer_amd as kao
    monkeypatch.setenv(HOOK, "1")
    for n in (1, 51, 100, 186, 317, 949, 2048):
        assert kao.cycle_square_plan(n)[1] == 1
    monkeypatch.setenv(HOOK, "3")
    assert kao.cycle_square_plan(128) == (128, 3, 48)              # 48, 48 and 32 midpoints
    assert kao.cycle_square_plan(51) == (64, 2, 32) and kao.cycle_square_plan(192) == (192, 3, 64)
    for forced in (2, 3, 5, 8, 13, 64, 5000):
        monkeypatch.setenv(HOOK, str(forced))
        for n in (64, 128, 320, 960, 2048):
            np_, ks, kchunk = kao.cycle_square_plan(n)
            assert kchunk % 16 == 0 and 2 <= ks <= forced and ks * kchunk >= np_ > (ks - 1) * kchunk
    monkeypatch.delenv(HOOK)
    for n in (0, -1, 2049):
        with pytest.raises(kao.KaoError):
            kao.cycle_square_plan(n)


def test_2048_brokers_and_racks_are_refused_before_any_device_call(ko):
    import kafka_assignment_optimizer_amd as kao
    import kao_cycle as kc
    pt, t = _drifted(ko, 2041, 7, 2400, 3)                         # n = 2049
    assert not kc.supported(t)
    for call in (lambda: kao.improve_cycles(pt, np.zeros((2400, 3), dtype=np.uint16), 1),
                 lambda: kao.cycle_matrices(pt, np.zeros((2400, 3), dtype=np.uint16), 0, 0)):
        with pytest.raises(kao.KaoError) as e:
            call()
        assert e.value.code == -2                                  # KAO_ERR_UNSUPPORTED
    assert kc.supported(_drifted(ko, 2040, 7, 2400, 3)[1])


def test_oracle_round_without_closures(ko, kp):
    import kao_cycle as kc
    _, t = _drifted(ko, 30, 3, 60)
    a = kp.port_search(t, 3, 0, 2, 64)["best"]
    full, edges = kc.Round(t, a), kc.Round(t, a, closures=False)
    assert np.array_equal(full.EF, edges.EF) and np.array_equal(full.ES, edges.ES) and not hasattr(edges, "DF")
    assert np.array_equal(full.DF[0], edges._dist0(edges.EF))

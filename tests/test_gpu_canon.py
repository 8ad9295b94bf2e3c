"""kao.canonicalize (k_canon on the device) against canon_ref (tests/canon_ref.py, itself held against kao_oracle.canonicalize by
tests/test_canon_ref.py), run on the MI355X box with -m gpu.  The inputs are expansions, decommissions and RF changes in which
most replicas are new -- built without a solver (canon_ref.canon_input) -- so many moves happen: the small ones of
test_canon_ref.py (RF 1..6, k_canon<4> and k_canon<8>) and larger ones that only the fast reference can afford.

(passes, moves) of the larger inputs under canon_ref:
  big140   (140, 7, 130, rf 3), slack        (2, 80)
  uneven   (150, 4, 200, rf 3), racks of 34 / 37 / 37 / 37 brokers: 148 internal broker slots      (2, 20), slack (2, 21)
  rackmap  (90, 5, 160, rf 3), rack_of a random permutation of b mod R                              (2, 27), slack (2, 28)
  rf6      (100, 5, 210, rf 6), k_canon<8>, four 64-partition blocks                                (2, 35), slack (2, 48)
  big300   (300, 6, 420, rf 3)                                                                      (2, 49)
  big300s  (300, 6, 430, rf 3), slack                                                               (2, 80)
"""
import functools

import numpy as np
import pytest

from canon_ref import SMALL_CASES, SMALL_SHAPES, canon_input, canon_ref
from conftest import to_product_topic

pytestmark = pytest.mark.gpu

UNEVEN = (150, 4, 200, 3, [0, 4, 8, 12, 16, 1], [(150, 0)], None)
RACKMAP = (90, 5, 160, 3, [2, 9], [(90, 1), (91, 4)], None)
RF6 = (100, 5, 210, 6, [3, 7], [(100, 3), (101, 2)], None)
# name -> (shape, slack bands, random rack map)
LARGE = {
    "big140": ((140, 7, 130, 3, [9, 10, 11], [(140, 2), (141, 3), (142, 4)], None), True, False),
    "uneven": (UNEVEN, False, False),
    "uneven_slack": (UNEVEN, True, False),
    "rackmap": (RACKMAP, False, True),
    "rackmap_slack": (RACKMAP, True, True),
    "rf6": (RF6, False, False),
    "rf6_slack": (RF6, True, False),
    "big300": ((300, 6, 420, 3, [5, 17], [(300, 0), (301, 1)], None), False, False),
    "big300s": ((300, 6, 430, 3, [5, 17], [(300, 0), (301, 1)], None), True, False),
}


@pytest.fixture(scope="module")
def kao():
    import kafka_assignment_optimizer_amd as k
    k.init(0)
    assert "gfx950" in k.device_name(), k.device_name()
    return k


@functools.lru_cache(maxsize=None)
def large_case(name):
    shape, slack, rackmap = LARGE[name]
    rack_of = None
    if rackmap:   # the target brokers' racks: as many per rack as b mod R gives, in a random order
        B = shape[0] - len(shape[4]) + len(shape[5])
        rack_of = np.random.default_rng(11).permutation(np.arange(B) % shape[1])
    return canon_input(shape, slack, rack_of)


def check_against_ref(kao, ko, ot, a1, min_moves):
    pt = to_product_topic(ot)
    want, passes, moves = canon_ref(ot, a1)
    assert passes >= 2 and moves >= min_moves, (passes, moves)
    got = kao.canonicalize(pt, a1)
    assert got.dtype == want.dtype and got.tolist() == want.tolist()
    obj0, v0 = ko.verify(ot, a1)
    obj, v = ko.verify(ot, got)
    assert v0[0] == 0 and v[0] == 0 and obj == obj0
    assert kao.canonicalize(pt, got).tolist() == got.tolist()     # a fixpoint
    return moves


@pytest.mark.parametrize("i,slack", SMALL_CASES)
def test_canonicalize_small_inputs(kao, ko, i, slack):
    ot, a1 = canon_input(SMALL_SHAPES[i], slack)
    check_against_ref(kao, ko, ot, a1, 1)


@pytest.mark.parametrize("name", list(LARGE))
def test_canonicalize_large_inputs(kao, ko, name):
    ot, a1 = large_case(name)
    if name.startswith("uneven"):
        sizes = np.bincount(np.asarray(ot.rack_of), minlength=ot.n_racks)
        assert sizes.min() < sizes.max() and ot.n_racks * sizes.max() > 128      # uneven racks, padded internal slots, three scan strides
    if name.startswith("rackmap"):
        assert (np.asarray(ot.rack_of) != np.arange(ot.n_brokers) % ot.n_racks).sum() > ot.n_brokers // 2
    check_against_ref(kao, ko, ot, a1, 20)


def test_canonicalize_returns_what_it_cannot_polish(kao, ko):
    """Broker weights (a move would change the objective), an empty slot, a band violation: the input comes back as it is --
    not even the follower order is touched."""
    ot, a1 = canon_input(SMALL_SHAPES[0], True)
    pt = to_product_topic(ot)
    assert kao.canonicalize(pt, a1).tolist() != a1.tolist()         # (the plain input does change)
    wt = canon_input(SMALL_SHAPES[0], True)[0]
    wt.broker_w = np.ones(wt.n_brokers, dtype=np.int32)
    assert kao.canonicalize(to_product_topic(wt), a1).tolist() == a1.tolist()
    for bad_value in (0xFFFF, ot.n_brokers):
        hole = a1.copy()
        hole[17, 2] = bad_value
        assert kao.canonicalize(pt, hole).tolist() == hole.tolist()
    # one band violation: a follower moved inside its rack, from a broker at rep_hi to one that is then one replica above it
    ot, a1 = canon_input(SMALL_SHAPES[0], False)
    pt = to_product_topic(ot)
    rack, hi = np.asarray(ot.rack_of), ot.bounds()["rep_hi"]
    cnt = np.bincount(a1.ravel().astype(np.int64), minlength=ot.n_brokers)
    over = None
    for p in range(ot.n_partitions):
        b = int(a1[p, 2])
        to = [int(x) for x in np.flatnonzero((rack == rack[b]) & (cnt == hi)) if int(x) not in a1[p]]
        if cnt[b] == hi and to:
            over = a1.copy()
            over[p, 2] = to[0]
            break
    assert over is not None
    v = ko.verify(ot, over)[1]
    assert v.tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    assert kao.canonicalize(pt, over).tolist() == over.tolist()
    assert canon_ref(ot, over)[0].tolist() == over.tolist()

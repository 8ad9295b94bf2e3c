"""canon_ref (tests/canon_ref.py, the fast restatement that tests/test_gpu_canon.py holds k_canon against) equals
kao_oracle.canonicalize bit for bit on inputs small enough for the oracle: expansions, decommissions and RF changes with RF 1..6,
where 84 % to 100 % of the replicas are new, as derived and with slack bands.  No GPU.

(passes, moves) of the inputs, as derived / with slack:
  (24, 3, 40, rf 3)        (2, 9)  / (2, 9)
  (30, 5, 36, rf 6)        (2, 8)  / (2, 10)
  (28, 4, 30, rf 4 -> 5)   (2, 7)  / (2, 10)
  (28, 4, 44, rf 5 -> 3)   (2, 8)  / (2, 16)
  (20, 1, 70, rf 2)        (2, 8)  / (2, 10)
  (16, 2, 33, rf 1)        (2, 2)  / (2, 2)
"""
import numpy as np
import pytest

from canon_ref import SMALL_CASES, SMALL_SHAPES, canon_input, canon_ref, new_fraction


@pytest.mark.parametrize("i,slack", SMALL_CASES)
def test_canon_ref_equals_the_oracle(ko, i, slack):
    ot, a1 = canon_input(SMALL_SHAPES[i], slack)
    assert ko.verify(ot, a1)[1][0] == 0 and new_fraction(ot, a1) >= 0.8
    got, passes, moves = canon_ref(ot, a1)
    want = ko.canonicalize(ot, a1)
    assert got.dtype == want.dtype and got.tolist() == want.tolist()
    assert passes >= 2 and moves >= 1, (passes, moves)


def test_canon_ref_inputs_move_enough():
    total = 0
    for i, slack in SMALL_CASES:
        ot, a1 = canon_input(SMALL_SHAPES[i], slack)
        got, passes, moves = canon_ref(ot, a1)
        assert passes >= 2 and moves >= 1, (i, slack, passes, moves)
        total += moves
    assert total >= 80, total


def test_canon_ref_leaves_infeasible_inputs_alone(ko):
    ot, a1 = canon_input(SMALL_SHAPES[0])
    bad = a1.copy()
    bad[3, 1] = 0xFFFF
    got, passes, moves = canon_ref(ot, bad)
    assert got.tolist() == bad.tolist() == ko.canonicalize(ot, bad).tolist() and (passes, moves) == (0, 0)


def test_canon_ref_keeps_the_objective_under_broker_weights(ko):
    """With broker weights a move to another broker can change the objective; the oracle refuses those moves, and so does
    canon_ref."""
    ot, a1 = canon_input(SMALL_SHAPES[5], True)
    rng = np.random.default_rng(3)
    ot.broker_w = rng.integers(0, 2, ot.n_brokers).astype(np.int32)
    ot.broker_wl = rng.integers(0, 2, ot.n_brokers).astype(np.int32)
    got, passes, moves = canon_ref(ot, a1)
    assert got.tolist() == ko.canonicalize(ot, a1).tolist()
    assert ko.verify(ot, got)[0] == ko.verify(ot, a1)[0]

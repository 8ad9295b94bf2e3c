"""CPU checks of what tests/test_gpu_waves_paths.py relies on: the host restatements of the wave cap (the second dimension of the
kernel's load arrays, which never leaves the device) and of the order budget, and the properties of the pinned instances -- the
cap bounds every first fit of the family and is reached by some, and the winners of the order-budget plans come late."""
import numpy as np

import waves_paths_cases as wc
import waves_ref as wr
import waves_sized_ref as sr


def test_family_covers_the_variants():
    fam = wc.cap_family()
    assert len(fam) == 240
    kinds = {}
    for c in fam:
        kinds.setdefault(c[0].split("-")[0], []).append(c)
    assert {k: len(v) for k, v in kinds.items()} == {"count": 40, "equal": 40, "tiny": 40, "tinyk": 40, "sized": 40, "c1": 40}
    assert all(c[3] is None for c in kinds["count"])
    assert all(len(set(c[3].tolist())) == 1 for c in kinds["equal"])
    assert all(c[4] == 1 for c in kinds["c1"])
    assert all(int(c[3].max()) <= 3 and 1 <= c[4] <= 5 for c in kinds["tiny"] + kinds["tinyk"])
    assert all(c[5] == 0 for c in kinds["tinyk"]) and sum(c[5] == 0 for c in fam) >= 60
    assert all(wc.n_moving(c) > 0 for c in fam)


def test_the_cap_bounds_every_first_fit_and_is_reached():
    """Every order's sequential first fit of every plan stays inside wave_cap waves (its highest wave is below the cap), and
    801 of the 240 x 64 first fits, on 13 plans, use exactly wave_cap waves: there a cap one too small loses a partition."""
    tight, tight_fits = [], 0
    for i, case in enumerate(wc.cap_family()):
        cap = wc.case_cap(case)
        fits = wc.case_fits(case)
        assert len(fits) == 64
        used = [max(f) + 1 for f in fits]
        assert max(used) <= cap, (case[0], max(used), cap)
        if cap in used:
            tight.append(i)
            tight_fits += used.count(cap)
    assert tight_fits >= 10
    assert (tuple(tight), tight_fits) == (wc.TIGHT, wc.TIGHT_FITS)
    # both planners and both kinds of cap are among them
    cases = [wc.cap_family()[i] for i in wc.TIGHT]
    assert any(c[3] is None for c in cases) and any(c[3] is not None and c[5] == 0 for c in cases)
    assert any(c[3] is not None and c[5] >= 1 for c in cases)


def test_wave_cap_by_hand():
    # a star of 5 at k = 2: the source has degree 5, every destination degree 1 -> 1 + floor(4 / 2)
    _, cur, tgt, *_ = wc.star(5)
    assert wr.wave_cap(cur, tgt, 2) == 3 and wr.wave_cap(cur, tgt, 1) == 5
    assert wr.wave_cap(cur, cur, 1) == 0
    # broker 0 sends 500 (above C = 100), 0, 40 and 70 bytes: T_0 = 610, degree 4; the destinations have degree 1 and add 0.
    # p0: t > C -> by = 110, min(3, 110) = 3.  p1: t = 0, 100 < 610 -> 610 // 101 = 6 -> 3.  p2: 60 < 570 -> 570 // 61 = 9 -> 3.
    cur = np.array([[0, 1], [0, 2], [0, 3], [0, 4]], dtype=np.uint16)
    tgt = np.array([[0, 5], [0, 6], [0, 7], [0, 8]], dtype=np.uint16)
    size = np.array([500, 0, 40, 70], dtype=np.uint64)
    assert sr.wave_cap_sized(cur, tgt, size, 100, 0) == 4
    assert sr.wave_cap_sized(cur, tgt, size, 100, 1) == 7      # + floor(3 / 1) by count
    assert sr.wave_cap_sized(cur, tgt, size, 100, 2) == 5
    assert sr.wave_cap_sized(cur, tgt, size, 0, 2) == 2        # no byte cap: the count term alone
    # two partitions of 10 and 20 bytes under C = 100: no load at broker 0 can block either (C - t >= rest)
    assert sr.wave_cap_sized(cur[:2], tgt[:2], np.array([10, 20], dtype=np.uint64), 100, 0) == 1
    # 60 and 50: 50 blocks 60 (40 < 50 -> 50 // 41 = 1) -> 2
    assert sr.wave_cap_sized(cur[:2], tgt[:2], np.array([60, 50], dtype=np.uint64), 100, 0) == 2


def test_order_count_at_its_boundaries():
    """per_order = B * wcap * (4 | 8 | 12) + 4 * n_mv + 24 * B against the budget of 2^30 bytes."""
    # 4 bytes (count-only): 1024 * (4 * 4089 + 24) = 16,773,120, + 4 * 1024 = 2^24 exactly -> 64 orders; 4 bytes more -> 63
    assert wr.order_count(1024, 4089, 1024, False, 1) == 64
    assert wr.order_count(1024, 4089, 1025, False, 1) == 63
    assert wr.order_count(1024, 4089, 1025, False, 3) == 63     # k does not enter the count-only layout
    # 8 bytes (sized, k = 0): 32768 * (8 * 2045 + 24) = 2^29 exactly -> 2 orders; 4 bytes more -> 1
    assert wr.order_count(32768, 2045, 0, True, 0) == 2
    assert wr.order_count(32768, 2045, 1, True, 0) == 1
    # 12 bytes (sized, k >= 1): 1000 * (12 * 1396 + 24) = 16,776,000, + 4 * 304 = 2^24 exactly -> 64; 4 bytes more -> 63
    assert wr.order_count(1000, 1396, 304, True, 1) == 64
    assert wr.order_count(1000, 1396, 305, True, 1) == 63
    assert wr.order_count(1000, 1396, 304, True, 0) == 64 and wr.order_count(1000, 1396, 304, False, 1) == 64
    # the same shape in the three layouts: 2^30 // (20000 * (w * 300 + 24) + 1200) = 43 | 22 | 14 for w = 4 | 8 | 12
    assert [wr.order_count(20000, 300, 300, s, k) for s, k in ((False, 1), (True, 0), (True, 2))] == [43, 22, 14]
    # never fewer than one order, never more than 64
    assert wr.order_count(65534, 5000, 70000, True, 1) == 1
    assert wr.order_count(1, 1, 1, False, 1) == 64


def test_models_report_the_winner_and_keep_their_old_result():
    cur, tgt, k = wr.random_instance(3)
    assert len(wr.kernel_model(cur, tgt, k, 4)) == 3
    wave, nw, lb, win = wr.kernel_model(cur, tgt, k, 4, with_winner=True)
    used = [max(f) + 1 for f in wr.order_fits(cur, tgt, k, 4)]
    assert (nw, win) == (min(used), used.index(min(used)))
    assert (wave.tolist(), nw, lb) == (wr.kernel_model(cur, tgt, k, 4)[0].tolist(),) + wr.kernel_model(cur, tgt, k, 4)[1:]
    scur, stgt, size, C, sk = sr.random_sized_instance(3)
    assert len(sr.kernel_model_sized(scur, stgt, size, C, sk, 4)) == 3
    assert sr.kernel_model_sized(scur, stgt, size, C, sk, 4, with_winner=True)[:3][1:] == sr.kernel_model_sized(scur, stgt, size, C, sk, 4)[1:]
    assert wr.kernel_model(cur, cur, k, 4, with_winner=True)[3] == -1     # nothing moves: no winner


def test_order_budget_plans_win_late():
    """The pinned plans of the order-budget tests: the winner among 64 orders is the pinned order j >= 8, strictly better than
    every earlier order, and both sides of the boundary are reachable with n_brokers <= 65534."""
    for layout, b_in in ((4, 19326), (8, 14812), (12, 8054)):
        case, j = wc.budget_case(layout)
        sized, k = case[3] is not None, case[5]
        assert (4 if not sized or k else 0) + (8 if sized else 0) == layout
        used = [max(f) + 1 for f in wc.case_fits(case)]
        assert j >= 8 and used.index(min(used)) == j and min(used[:j]) > used[j]
        assert wc.run_model(case, 64, True)[3] == j
        assert wc.run_model(case, j + 1)[1] == used[j] and wc.run_model(case, j)[1] == min(used[:j]) > used[j]
        wcap, n_mv = wc.case_cap(case), wc.n_moving(case)
        assert wc.brokers_for(case, j + 1) == b_in <= 65533
        assert wr.order_count(b_in, wcap, n_mv, sized, k) == j + 1 and wr.order_count(b_in + 1, wcap, n_mv, sized, k) == j
        assert wr.order_count(b_in - 1, wcap, n_mv, sized, k) >= j + 1 and wr.order_count(wc.brokers_of(case), wcap, n_mv, sized, k) == 64
    one = wc.one_order_case()
    assert wc.case_cap(one) == 2062 and wr.order_count(65534, 2062, 230, False, 1) == 1
    # 65534 * (4 * 2042 + 24) + 920 = 536,855,448 <= 2^29 = 536,870,912 < 65534 * (4 * 2043 + 24)
    assert wr.order_count(65534, 2042, 230, False, 1) == 2 and wr.order_count(65534, 2043, 230, False, 1) == 1


def test_stars_need_a_wave_and_a_round_per_partition():
    for n in (31, 32, 33, 64, 65):
        for case in (wc.star(n), wc.star(n, wc.GIB, 0, 1), wc.star(n, wc.GIB, wc.GIB, 0)):
            wave, nw, lb = wc.run_model(case)
            assert nw == lb == n == wc.case_cap(case) and wave.tolist() == list(range(n))


def test_row_shape_cases_hold_what_they_name():
    cases = {c[0]: c for c in wc.shape_cases()}
    assert len(cases) == len(wc.SHAPE_NAMES) == 24
    parts = lambda name: [s for s in wr.classify(cases[name][1], cases[name][2])[1] if s]   # noqa: E731
    assert cases["nine/C0"][1].shape[1] == 8 and max(len(s) for s in parts("nine/C0")) == 9
    cur, tgt = cases["padded/C2"][1:3]
    assert cur.shape[1] == 8 and (cur[:, 2:] == wc.NONE).all() and (tgt[:, 2:] == wc.NONE).all() and (cur[:, :2] != wc.NONE).all()
    cur, tgt = cases["nosource/C0"][1:3]
    bare = [p for p in range(len(cur)) if cur[p, 0] == wc.NONE]
    assert bare and all((cur[p, 1:3] != wc.NONE).all() for p in bare)
    _, pp, traf = sr.traffic(cur, tgt, cases["nosource/C0"][3])
    assert {len(pp[p]) for p in bare} == {1, 2, 3}      # no source: every participant is an added broker and carries size[p]
    assert all(set(traf[p]) == {int(cases["nosource/C0"][3][p])} for p in bare)
    cur, tgt = cases["rfchange/count"][1:3]
    rf = lambda rows: (rows != wc.NONE).sum(axis=1)     # noqa: E731
    cls = wr.classify(cur, tgt)[0]
    assert any(a < b and c == 1 for a, b, c in zip(rf(cur), rf(tgt), cls))      # RF up: a broker added
    assert any(a > b and c == 0 for a, b, c in zip(rf(cur), rf(tgt), cls))      # RF down, nothing added: wave 0
    assert any(a > b and c == 1 for a, b, c in zip(rf(cur), rf(tgt), cls))      # RF down and a broker replaced
    for n in (255, 256, 257):
        assert len(parts(f"moving{n}/C0")) == n and cases[f"moving{n}/C0"][1].shape[0] % 64 != 0
    assert {c[6] for c in cases.values() if c[0].startswith("seed")} == {0, 1 << 63, (1 << 64) - 1}

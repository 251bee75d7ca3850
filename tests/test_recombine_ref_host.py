"""The NumPy restatement of ``mpp_recombine`` (tests/recombine_ref.py) on hand-made inputs with known answers: the link
boundary, ties, an empty replica, non-finite sums, the composite order, the does-not-fit status.  No GPU."""
import math

import numpy as np

from recombine_ref import linked, recombine_tile, same_bits, select_winner, slot_sum

CAP, MAX_INTER = 8, 32.0
A, B = (10, 10), (100, 100)          # two places that do not interact


def tile(replicas, cap=CAP):
    """replicas: per replica a list of (x, y, e)"""
    xy = [np.array([[p[0], p[1]] for p in r], dtype=np.int32).reshape(-1, 2) for r in replicas]
    e = [np.array([p[2] for p in r], dtype=np.float64) for r in replicas]
    return recombine_tile(xy, e, cap, MAX_INTER)


def test_the_link_boundary():
    assert linked(0, 32, 32.0) and linked(24, 21, 32.0) and linked(0, 0, 32.0)            # 1024, 1017, 0
    assert not linked(32, 1, 32.0) and not linked(31, 8, 32.0) and not linked(20, 25, 32.0)   # all 1025
    assert linked(-32, 0, 32.0) and not linked(-32, -1, 32.0)


def test_two_groups_take_the_best_of_each():
    # replica 0: good at A, bad at B; replica 1 the reverse.  Replica 0 wins as a whole (-1.0 + 0.5 < 0.75 - 1.0 is false:
    # -0.5 vs -0.25), the composite takes B from replica 1
    t = tile([[(*A, -1.0), (*B, 0.5)], [(A[0] + 3, A[1], 0.75), (B[0], B[1] + 3, -1.0)]])
    assert t["winner"] == 0 and t["status"] == 1 and t["n_clusters"] == 2 and t["n_taken"] == 1
    assert t["kept"] == [(0, 0), (1, 1)] and t["n_before"] == 2 and t["n_after"] == 2
    assert t["E_winner"] == -0.5 and t["E_sum"] == -2.0 and t["E_after"] is None
    assert t["src"][:2].tolist() == [[0, 0], [1, 1]] and np.all(t["src"][2:] == -1)
    assert t["cluster"][0].tolist() == [0, 1] and t["cluster"][1].tolist() == [0, 1]       # ids: smallest r * cap + slot
    assert t["S"][0] == [-1.0, 0.75] and t["S"][1] == [0.5, -1.0]


def test_a_link_decides_the_outcome():
    # replica 0: p (e -1.0) and q (e +0.5), offset d apart; replica 1: only p' on p (e -0.9).  Linked: one cluster, S = [-0.5, -0.9],
    # replica 1 is taken and q goes.  Not linked: q's cluster has S = [0.5, 0.0] (taken: q goes), p's has [-1.0, -0.9] (stays)
    for d, is_linked in (((0, 32), True), ((24, 21), True), ((32, 1), False), ((31, 8), False), ((20, 25), False)):
        t = tile([[(50, 50, -1.0), (50 + d[0], 50 + d[1], 0.5)], [(50, 50, -0.9)]])
        assert t["winner"] == 1                                   # -0.9 < -0.5
        t = tile([[(50, 50, -1.0), (50 + d[0], 50 + d[1], 0.25)], [(50, 50, -0.7)]])
        assert t["winner"] == 0                                   # -0.75 < -0.7
        if is_linked:
            assert t["n_clusters"] == 1 and t["status"] == 0 and t["kept"] == [(0, 0), (0, 1)], d
        else:
            assert t["n_clusters"] == 2 and t["status"] == 1 and t["n_taken"] == 1 and t["kept"] == [(0, 0)], d
            assert t["E_sum"] == -1.0


def test_ties_stay_with_the_winner():
    # equal chain energies: replica 0 wins; equal cluster sums: nothing is taken, also not by a later replica
    t = tile([[(*A, -0.5), (*B, 0.25)], [(*A, -0.5), (*B, 0.25)], [(*A, -0.5), (*B, 0.25)]])
    assert t["winner"] == 0 and t["status"] == 0 and t["n_taken"] == 0 and t["n_clusters"] == 2
    assert t["src"][:2].tolist() == [[0, 0], [0, 1]] and t["E_after"] == t["E_winner"] == t["E_sum"] == -0.25
    # the winner is replica 1; replica 0 ties with it in A and does not take it, replica 2 ties with replica 0's better B
    t = tile([[(*A, -0.5), (*B, 0.0)], [(*A, -0.5), (*B, -0.25)], [(*A, 0.5), (*B, -0.25)]])
    assert t["winner"] == 1 and t["status"] == 0 and all(r == 1 for r in t["choice"].values())


def test_an_empty_replica_competes_with_zero():
    # replica 1 is empty: chain energy 0.0.  Replica 0 wins with -0.5; its cluster at B costs +0.5 > 0.0: taken from the empty one
    t = tile([[(*A, -1.0), (*B, 0.5)], []])
    assert t["winner"] == 0 and t["status"] == 1 and t["n_taken"] == 1 and t["kept"] == [(0, 0)] and t["n_after"] == 1
    assert t["E_sum"] == -1.0 and t["S"][1] == [0.5, 0.0]
    # the empty replica as the winner: a cluster with a negative sum is taken from the other
    t = tile([[], [(*A, 0.75), (*B, -0.5)]])
    assert t["winner"] == 0 and t["n_before"] == 0 and t["status"] == 1 and t["kept"] == [(1, 1)] and t["E_sum"] == -0.5
    assert t["cluster"][1].tolist() == [CAP, CAP + 1]
    # all empty
    t = tile([[], [], []])
    assert t["status"] == 0 and t["n_clusters"] == 0 and t["n_after"] == 0 and t["E_sum"] == 0.0 and np.all(t["src"] == -1)


def test_non_finite_sums():
    nan, inf = float("nan"), float("inf")
    assert select_winner([nan, 1.0]) == 1 and select_winner([nan, inf, nan]) == 0 and select_winner([1.0, nan, -inf]) == 2
    assert select_winner([inf, 2.0, 1.0]) == 2 and select_winner([-inf, 1.0]) == 1
    # replica 0 wins (finite), its A cluster is fine; replica 1 has a NaN at A and the better B
    t = tile([[(*A, -1.0), (*B, 0.5)], [(*A, nan), (*B, -0.5)]])
    assert t["winner"] == 0 and math.isnan(slot_sum([nan, -0.5])) and t["kept"] == [(0, 0), (1, 1)] and t["E_sum"] == -1.5
    # the winner's own cluster is NaN where another replica is finite: taken, however large the finite sum
    t = tile([[(*A, nan), (*B, -3.0)], [(*A, 100.0), (*B, 0.0)], [(*A, nan), (*B, inf)]])
    assert t["winner"] == 1                                       # the only finite chain energy
    t = tile([[(*A, nan), (*B, nan)], [(*A, nan), (*B, 7.0)], [(*A, inf), (*B, 9.0)]])
    assert t["winner"] == 0 and t["choice"] == {0: 0, 1: 1} and t["kept"] == [(0, 0), (1, 1)] and math.isnan(t["E_sum"])
    assert same_bits(t["E_sum"], nan) and not same_bits(0.0, -0.0) and same_bits([1.5, nan], [1.5, nan])
    # +inf + -inf inside a sum is NaN.  The walk is the rule, not "the minimum": -inf is strictly lower than 5.0 and takes the
    # lead, and a later finite value takes it back from a best that is not finite
    t = tile([[(*A, inf), (A[0] + 1, A[1], -inf)], [(*A, 5.0)], [(*A, -inf)]])
    assert t["winner"] == 2 and t["choice"] == {0: 1} and t["E_sum"] == 5.0 and t["status"] == 1
    t = tile([[(*A, 5.0)], [(*A, -inf)], [(*A, inf), (A[0] + 1, A[1], -inf)]])
    assert t["winner"] == 1 and t["choice"] == {0: 0} and t["E_sum"] == 5.0
    t = tile([[(*A, -inf)], [(*A, inf), (A[0] + 1, A[1], -inf)]])
    assert t["winner"] == 0 and t["choice"] == {0: 0} and t["E_sum"] == -inf and t["status"] == 0


def test_the_composite_order_is_winner_first_then_replicas_ascending():
    C = (10, 100)
    # winner 1 keeps B; A comes from replica 2, C from replica 0: order 1, 0, 2 -- slots ascending within a replica
    t = tile([[(*C, -1.0), (*A, 0.5), (C[0] + 2, C[1], -1.0)],
              [(*A, 0.0), (*B, -5.0), (*C, 0.0)],
              [(A[0] + 1, A[1], -0.25), (*A, -0.25)]])
    assert t["winner"] == 1 and t["status"] == 1 and t["n_taken"] == 2 and t["n_clusters"] == 3
    assert t["kept"] == [(1, 1), (0, 0), (0, 2), (2, 0), (2, 1)]
    assert t["src"][:5].tolist() == [[1, 1], [0, 0], [0, 2], [2, 0], [2, 1]] and t["n_before"] == 3 and t["n_after"] == 5
    # cluster ids ascending: C (g = 0), A (g = 1), B (g = 9); the sums added in that order
    assert sorted(t["choice"]) == [0, 1, CAP + 1] and t["E_sum"] == ((0.0 + -2.0) + -0.5) + -5.0


def test_the_sums_are_formed_in_slot_order():
    v = [1e16, 1.0, -1e16, 1.0]
    assert slot_sum(v) == 1.0 and slot_sum(v[::-1]) == 0.0
    t = tile([[(10, 10, 1e16), (11, 10, 1.0), (12, 10, -1e16), (13, 10, 1.0)], [(10, 10, 0.5)]])
    assert t["S"][0] == [1.0, 0.5] and t["winner"] == 1 and t["status"] == 0


def test_does_not_fit():
    # cap 3: the winner holds 2 points at A; B, with two points, comes from replica 1: 4 > 3
    t = tile([[(*A, -1.0), (A[0] + 1, A[1], -1.0)], [(*A, 0.0), (*B, -0.5), (B[0] + 1, B[1], -0.5)]], cap=3)
    assert t["winner"] == 0 and t["n_taken"] == 1 and len(t["kept"]) == 4 and t["status"] == 2
    assert t["n_after"] == 2 and t["src"].tolist() == [[0, 0], [0, 1], [-1, -1]] and t["E_after"] == t["E_winner"] == -2.0
    assert t["E_sum"] == -3.0
    # ... and with room for it: status 1
    t = tile([[(*A, -1.0), (A[0] + 1, A[1], -1.0)], [(*A, 0.0), (*B, -0.5), (B[0] + 1, B[1], -0.5)]], cap=4)
    assert t["status"] == 1 and t["n_after"] == 4


def test_a_chain_of_links_is_one_cluster_with_the_smallest_index_as_id():
    # a path whose points alternate between the replicas, 30 px apart; the smallest global index sits in the middle
    xs = [10 + 30 * k for k in range(7)]
    order0, order1 = [3, 1, 5], [0, 2, 4, 6]                     # replica 0's slot 0 is the path's middle
    t = tile([[(xs[k], 10, -0.1) for k in order0], [(xs[k], 10, -0.1) for k in order1]])
    assert t["n_clusters"] == 1 and t["cluster"][0].tolist() == [0, 0, 0] and t["cluster"][1].tolist() == [0, 0, 0, 0]

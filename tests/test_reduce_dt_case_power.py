"""CPU, oracle only: the order and root cases of tests/test_gpu_reduce_dt.py CAN fail, and the instantiation matrix
of tests/test_gpu_reduce_dt_matrix.py covers what it says.

A GPU case protects an operand order only if the oracle's own expectation changes when that order does. For
every case of reduce_dt_cases.ORDER_ROWS the expectation is recomputed under each mutation the case is there to
catch, and must then differ in bits (reduce_dt_cases.differs' rule: two NaNs of a float SUM / PROD are equal)
on at least one packed element of at least one rank's significant receive buffer:
  root   Reduce: the root replaced by another root. Float MAX / MIN and the pair types show the operand order
         itself, so each of their cases must tell EVERY other root. Float SUM is commutative bit for bit (NaNs
         aside) and shows association only: FT from root 0 and from root 1 are the same sum, so a SUM case must
         tell the other root of its row (0 against P - 1), whose folds differ in association.
  swap   the send vectors of ranks i < j exchanged — every pair must be told apart by at least one case of the
         world's set (a single case need not); at P = 2 a new-collectives Reduce_scatter case on an op that shows
         the operand order must tell the pair apart on rank 1's block, the one place where the ring
         {in[1], in[0]} (FLOAT) and the MST order {in[0], in[1]} (the pair types) differ.
  flag   MPJX_FLAG_OLD_COLLECTIVES flipped, where the two algorithms define different orders. They do not always:
         at P = 2 MST, FT and Reduce agree on {in[root], in[1 - root]} (only Reduce_scatter's ring on a base type
         differs, on rank 1, and only for an op that is not commutative), and at P = 3 the MST tree rooted at 0
         or 1 IS the FT fold (x[root], then the others ascending), so a P = 3 Reduce tells them apart at root 2
         only and a P = 3 Reduce_scatter (MST(0) against the fold from x[0]) cannot. Where the orders differ,
         every float SUM / PROD case must show it (the two differ in association, which is what SUM shows); the
         MAX / MIN / pair cases see a regrouping only through a NaN or a zero in the right place, so they must
         show it as a world's set, and singly where the operand order itself differs (the P = 2 ring).
This is a condition on the inputs, not a measurement; the seeds of ORDER_ROWS are chosen so that it holds.

The matrix pins wiring, which integer results show too, so it needs no such check, with one exception: a case
whose expected result equals one operand's packed input over the whole vector would pass with the combine
skipped. None may; and the matrix's parametrisation must launch every (functor, kind, P, W) of
launch_functor_dt."""
import itertools

import numpy as np
import pytest

import oracle as O
import reduce_dt_cases as RC
from util import flat


def changed(case, a, b):
    """Packed elements whose bits differ between two results of `case`"""
    t = RC.ORACLE_TYPE[case.base]
    fa, fb = flat(np.ascontiguousarray(a), t), flat(np.ascontiguousarray(b), t)
    if fa.size == 0:
        return 0
    ne = fa.view(np.uint8).reshape(fa.size, -1) != fb.view(np.uint8).reshape(fb.size, -1)
    ne = ne.any(axis=1)
    if t in (O.FLOAT, O.DOUBLE) and case.op in (O.SUM, O.PROD):
        ne &= ~(np.isnan(fa) & np.isnan(fb))
    return int(ne.sum())


def significant(case, P, res, root=None):
    """The packed results that a call of `case` delivers: (rank, vector)"""
    if case.kind == "reduce":
        root = case.root if root is None else root
        return [(case.root, res[root])]
    return [(r, res[r]) for r in range(P)]


def delta(case, P, true, mut, root=None, rank=None):
    """Elements that differ between the true results and a mutation's, over the significant buffers"""
    return sum(changed(case, a, b) for (r, a), (_, b) in zip(significant(case, P, true), significant(case, P, mut, root))
               if rank is None or r == rank)


def flag_shows(case, P):
    """The old- and new-collectives orders of `case` differ (the module docstring's reasoning)"""
    pair = RC.ORACLE_TYPE[case.base] in O.PAIR_BASE
    if case.kind == "reduce":
        return P >= 4 or (P == 3 and case.root == 2)
    if case.kind == "reduce_scatter":
        return P >= 4 or (P == 2 and not pair)
    return case.kind == "allreduce" and P >= 3


def commutes(case):
    """Float SUM and PROD give the same bits for a (op) b and b (op) a: they show association, not operand order"""
    return case.op in (O.SUM, O.PROD)


@pytest.mark.parametrize("row,P", RC.ORDER_ROWS, ids=[f"{row}-P{P}" for row, P in RC.ORDER_ROWS])
def test_order_cases_tell_the_orders_apart(row, P):
    cases = RC.order_group(row, P)
    told = {pair: 0 for pair in itertools.combinations(range(P), 2)}
    flag_told, flag_due = 0, False
    for case in cases:
        _, packed = RC.inputs(case, P)
        assert packed[0].size >= 16, case
        true = RC.combine(case, P, packed)
        if case.kind == "reduce":
            for other in ((0, P - 1) if commutes(case) else range(P)):
                if other != case.root:
                    assert delta(case, P, true, RC.combine(case, P, packed, root=other), root=other) > 0, \
                        (case, "cannot tell root", other)
        if flag_shows(case, P):
            d = delta(case, P, true, RC.combine(case, P, packed, old=not case.old))
            if P == 2:  # the ring against the fold: the operand order on rank 1
                assert commutes(case) or d > 0, (case, "cannot tell the flag")
            else:
                assert not commutes(case) or d > 0, (case, "cannot tell the flag")
                flag_due = True
                flag_told += d > 0
        for i, j in told:
            swapped = list(packed)
            swapped[i], swapped[j] = packed[j], packed[i]
            mut = RC.combine(case, P, swapped)
            told[(i, j)] += delta(case, P, true, mut) > 0
            if P == 2 and case.kind == "reduce_scatter" and not case.old and not commutes(case):
                assert delta(case, P, true, mut, rank=1) > 0, (case, "rank 1's block")
    assert all(told.values()), (row, P, "no case tells these ranks' sends apart", [p for p, n in told.items() if not n])
    assert flag_told or not flag_due, (row, P, "no case tells the old collectives from the new")


@pytest.mark.parametrize("P", range(2, 9))
def test_no_matrix_case_equals_an_operand(P):
    """Scan's rank 0 receives its own input by definition; every other significant result must differ from
    every operand somewhere."""
    for op in RC.OPS:
        new, old = RC.matrix_cases(P, op)
        for case in new + old:
            _, packed = RC.inputs(case, P)
            res = RC.combine(case, P, packed)
            for r, got in significant(case, P, res):
                if case.kind == "scan" and r == 0:
                    continue
                for p in range(P):
                    assert changed(case, got, packed[p]) > 0, (case, "rank", r, "receives operand", p)


def test_the_matrix_launches_every_instantiation():
    got = set()
    for P in range(2, 9):
        for op in RC.OPS:
            got |= set(RC.matrix_launches(P, op))
    functors = [(op, RC.TYPE_NAMES[t - 1]) for op, t in O.valid_pairs()] + \
               [(op, O.TYPE_NAMES[t]) for op, t in O.loc_pairs()]
    assert len(functors) == 56
    want = set()
    for op, base in functors:
        e = RC.elem_bytes(base)
        for W in {1, 16 // e}:
            want |= {(op, base, RC.K_FOLD, P, W) for P in range(2, 9)}
            want |= {(op, base, RC.K_MST, P, W) for P in range(3, 9)}
            want |= {(op, base, RC.K_SCAN, P, W) for P in range(2, 9)}
    assert got == want, (sorted(want - got)[:5], sorted(got - want)[:5])
    assert len(want) == 20 * (52 * 2 + 4)  # LONG2 and DOUBLE2 are their own granule: one width


def test_matrix_counts_are_one_tile_and_a_partial_one():
    for P in range(2, 9):
        for base in RC.TYPE_NAMES:
            for _, W, _, _ in RC.matrix_widths(base):
                tile = 256 * RC.dt_unroll(P, W)
                gran = RC.matrix_count(base, P, W) * 96 // (W * RC.elem_bytes(base))
                assert tile < gran <= tile + 96, (base, P, W, gran)
    assert [256 * RC.dt_unroll(P, 1) for P in range(2, 9)] == [1024, 512, 512, 256, 256, 256, 256]
    assert {RC.dt_unroll(P, W) for P in range(3, 9) for W in (8, 16)} == {1}

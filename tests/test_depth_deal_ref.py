"""Without a GPU: every case of test_gpu_depth_deal.py reaches the path it is named for — tie path, chunked bucket, bucket at
capacity, overflow — judged from the restatement alone (depth_deal_cases.Plan on dsort_ref's digits and bucket sizes), and the
restatement's buckets are runs of the stable order it expects."""
import numpy as np
import pytest

import depth_deal_cases as D
import dsort_ref as R

CASES = D.build_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_case_reaches_its_path(case):
    refs = D.reference(case)
    D.check_claims(case, refs)
    for (keys, counts), (plan, run) in zip(case.frames, refs):
        f = run.frame
        assert np.array_equal(f.order, np.flatnonzero(keys != R.CULLED)[np.argsort(keys[keys != R.CULLED], kind="stable")])
        if plan.valid:   # the table's buckets are runs of that order, in bucket order
            assert np.array_equal(np.cumsum(plan.sizes)[-1:], [f.nv])
            d = R.table_digits(keys, np.asarray(plan_table(case, refs, plan)))[f.order]
            assert np.all(np.diff(d) >= 0)


def plan_table(case, refs, plan):
    table = np.array(case.table)
    for p, run in refs:
        if p is plan:
            return table
        table = run.table
    raise AssertionError


def test_the_cases_cover_what_the_issue_names():
    ids = {c.id for c in CASES}
    claims = {cl for c in CASES for cl in c.claims}
    assert {"listed-%d-of-%d" % x for x in ((0, 4101), (1, 4101), (63, 4101), (64, 65537), (65, 65537), (16383, 65537), (16384, 65537), (200000, (1 << 20) + 1))} <= ids
    assert {"overflow", "no-overflow", "tied", "chunked", "resident", "at-capacity", "on-splitter", "one-bucket"} <= claims
    assert any(len(c.frames) == 3 for c in CASES) and sum(len(c.strides) == 5 for c in CASES) >= 1
    assert D.deal_capacity(1 << 20) == 8192 and D.deal_capacity(1000) == 2048

"""Linear-transform plans without a GPU (include/fhelin.h "Linear transforms"): a plan is host data - it is created on a device-less
context, reports its split and exactly the rotation keys it needs, and the planner's choice of n1 minimises the cost its comment states
(csrc/capi_lt.cpp split_cost).  Applying a plan needs a device."""
import numpy as np
import pytest

ERR_ARG, ERR_NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def host(fa):
    e = fa.Engine("toy13", device=-1)
    yield e
    e.close()


def _cost(idx, n1):
    """the planner's cost in quarters of a pair-ModDown, restated from its comment: 4 (n2 + ceil(R / 7)) + baby keys read, with n2 the
    groups and R the rotated ones among them"""
    groups = {d - d % n1 for d in idx}
    babies = {d % n1 for d in idx} - {0}
    n2, R = len(groups), len(groups - {0})
    return 4 * (n2 + -(-R // 7)) + len(babies)


def _best_n1(idx):
    return min(range(1, 33), key=lambda n1: (_cost(idx, n1), n1))       # ties: the smaller n1


def test_plan_on_a_device_less_context(fa, host):
    assert not host.has_device
    ns = 1 << host.params.log_slots
    rng = np.random.default_rng(0)
    idx = [0, 1, 2, 5, 9, -1, 12 + ns]                     # reduced mod slots: -1 -> ns - 1, 12 + ns -> 12
    lt = host.lt_create(rng.uniform(-1, 1, (len(idx), ns)), idx, n1=4)
    red = sorted(d % ns for d in idx)
    inf = lt.info()
    assert inf == dict(n1=4, n2=len({d - d % 4 for d in red}), n_terms=len(idx), slots=ns)
    # exactly the needed keys: the baby residues in use (1, 2, 3 = (ns - 1) % 4; 5 and 9 share 1) and the nonzero group offsets
    want = {d % 4 for d in red if d % 4} | {d - d % 4 for d in red if d - d % 4}
    rot = lt.rotations()
    assert len(rot) == len(set(rot)) and set(rot) == want
    with pytest.raises(fa.FhelinError) as ei:
        host.lt_apply(lt, [])
    assert ei.value.code == ERR_NO_DEVICE
    lt.free()


def test_plan_from_terms_reports_only_the_keys_of_present_terms(fa, host):
    ns = 1 << host.params.log_slots
    p = host.encode(np.linspace(-1, 1, ns))
    pts = [[None, p, None, None], [p, None, None, p]]      # baby column 2 carries no term: its key is not needed
    lt = host.lt_create_pts(pts, [0, 3, 5, -7], [0, 64])
    assert lt.info() == dict(n1=4, n2=2, n_terms=3, slots=ns)
    assert sorted(lt.rotations()) == [-7, 3, 64]
    for bad in (lambda: host.lt_create_pts(pts, [1, 3, 5, 7], [0, 64]),          # baby[0] must be the unrotated step
                lambda: host.lt_create_pts(pts, [0, 3, 3 + ns, 7], [0, 64]),     # duplicate baby step mod slots
                lambda: host.lt_create_pts(pts, [0, 3, 5, 7], [64, 64 - ns]),    # duplicate giant step mod slots
                lambda: host.lt_create_pts([[None] * 4] * 2, [0, 3, 5, 7], [0, 64]),
                lambda: host.lt_create_pts([[p] * 33], list(range(33)), [0])):
        with pytest.raises(fa.FhelinError) as ei:
            bad()
        assert ei.value.code == ERR_ARG


@pytest.mark.parametrize("name,idx", [
    ("8 dense", list(range(8))),
    ("16 dense", list(range(16))),
    ("128 dense", list(range(128))),
    ("128 at multiples of 128", [128 * i for i in range(128)]),
])
def test_planner_minimises_its_stated_cost(fa, name, idx):
    """log_slots = 14 so that 128 multiples of 128 are distinct diagonals; bench's ring, no device"""
    e = fa.Engine("bench", device=-1)
    try:
        ns = 1 << e.params.log_slots
        assert len({d % ns for d in idx}) == len(idx)
        lt = e.lt_create(np.ones((len(idx), ns)), idx)
        inf = lt.info()
        best = _best_n1(idx)
        assert inf["n1"] == best, (name, inf, best)
        assert inf["n2"] == len({d - d % best for d in idx}) and inf["n_terms"] == len(idx)
    finally:
        e.close()

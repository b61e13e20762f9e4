"""Deferred evaluation across lanes (csrc/deferred.h; fhelin_ctx_set_lane / fhelin_ctx_lane_wait): a deferred operation is evaluated
under the lane it was issued under, whoever reads it; fhelin_ctx_lane_wait evaluates what that lane still holds; a flush that fails
leaves the context on the caller's lane; fhelin_sync visits every lane and reports one failure.  fhelin_ct_force on rows of two
deferred groups evaluates exactly the listed rows, together.  Every result is compared byte for byte with the batched eager call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CF = np.array([0.3, 0.5, -0.2, 0.1, 0.05, -0.03, 0.02, 0.01])           # degree 7 (test_deferred_failures_gpu.py)


@pytest.fixture(scope="module")
def lanes(fa):
    eng = fa.Engine("toy13", seed=4)
    eng.keygen()
    eng.gen_relin_key()
    eng.gen_rotation_keys([1])
    ns = 1 << eng.params.log_slots
    v = np.random.default_rng(1).uniform(-0.9, 0.9, ns)
    x = eng.encrypt(v, level=0)
    x_low = eng.encrypt(v, level=eng.n_q - 2)        # 2 limbs: passes the call-time check, runs out of limbs on the host during evaluation
    want = eng.eval_chebyshev_batch([x], CF)[0].export()
    eng.sync()                                       # the inputs exist before any lane reads them
    yield dict(eng=eng, x=x, x_low=x_low, want=want, v=v)
    eng.set_lane(0)
    eng.close()


def _under(eng, lane, f):
    eng.set_lane(lane)
    try:
        return f()
    finally:
        eng.set_lane(0)


def test_a_result_deferred_under_another_lane_is_read_under_this_one(lanes):
    eng, x, want = lanes["eng"], lanes["x"], lanes["want"]
    h = _under(eng, 1, lambda: eng.eval_chebyshev(x, CF))
    assert np.array_equal(h.export(), want)
    eng.sync()


def test_lane_wait_evaluates_what_the_other_lane_deferred(lanes):
    eng, x, want = lanes["eng"], lanes["x"], lanes["want"]
    eng.sync()
    h = _under(eng, 1, lambda: eng.eval_chebyshev(x, CF))
    eng.stats(reset=True)
    assert eng.stats()["keyswitch"] == 0             # issuing is not evaluating
    eng.lane_wait(1)
    assert eng.stats()["keyswitch"] > 0              # evaluated by the wait, before any read
    assert np.array_equal(h.export(), want)
    eng.sync()


@pytest.mark.parametrize("surface", ["read", "lane_wait"])
def test_the_callers_lane_is_back_after_a_failing_flush(lanes, fa, surface):
    eng, x, x_low, want = lanes["eng"], lanes["x"], lanes["x_low"], lanes["want"]
    bad = _under(eng, 1, lambda: eng.eval_chebyshev(x_low, CF))
    if surface == "lane_wait":
        eng.lane_wait(1)                             # evaluates lane 1's operation; its failure stays with the handle
    with pytest.raises(fa.FhelinError) as e:
        bad.export()
    assert "deferred operation failed" in str(e.value)
    eng.stats(reset=True)
    good = eng.eval_chebyshev(x, CF)
    assert eng.stats()["keyswitch"] == 0             # still deferred: the context is back on the caller's lane (elsewhere it would run at the call)
    assert np.array_equal(good.export(), want)
    assert eng.stats()["keyswitch"] > 0
    eng.sync()                                       # nothing pending, no stale error


def test_sync_visits_every_lane_and_reports_one_failure(lanes, fa):
    eng, x, x_low, want = lanes["eng"], lanes["x"], lanes["x_low"], lanes["want"]
    g0 = eng.eval_chebyshev(x, CF)
    g1, bad = _under(eng, 1, lambda: (eng.eval_chebyshev(x, CF), eng.eval_chebyshev(x_low, CF)))
    with pytest.raises(fa.FhelinError):
        eng.sync()
    eng.sync()                                       # reported once
    assert np.array_equal(g0.export(), want) and np.array_equal(g1.export(), want)
    del bad
    eng.sync()


def test_force_evaluates_exactly_the_listed_rows_of_two_groups(lanes):
    eng, v = lanes["eng"], lanes["v"]
    ns = len(v)
    rng = np.random.default_rng(7)
    w, b = eng.encode(rng.uniform(-1, 1, ns) / 8), eng.encode(rng.uniform(-1, 1, ns))
    rows = [eng.encrypt(rng.uniform(-0.9, 0.9, ns), level=0) for _ in range(6)]
    ga_rows, gb_rows = rows[:3], rows[3:]
    listed = [ga_rows[0], ga_rows[2], gb_rows[1], gb_rows[2]]
    eng.set_lazy_rows(False)
    try:
        eng.sync()
        eng.stats(reset=True)
        eager = [o.export() for o in eng.matmul_pt(listed, w, b, 2, 1)]
        eager_ks = eng.stats()["keyswitch"]
        rest = [o.export() for o in eng.matmul_pt([ga_rows[1], gb_rows[0]], w, b, 2, 1)]
    finally:
        eng.set_lazy_rows(True)
    assert eager_ks > 0
    eng.sync()
    eng.stats(reset=True)
    ga, gb = eng.matmul_pt(ga_rows, w, b, 2, 1), eng.matmul_pt(gb_rows, w, b, 2, 1)
    assert eng.stats()["keyswitch"] == 0
    eng.force([ga[0], ga[2], gb[1], gb[2]])
    assert eng.stats()["keyswitch"] == eager_ks      # the four listed rows, nothing else
    for h, e in zip([ga[0], ga[2], gb[1], gb[2]], eager):
        assert np.array_equal(h.export(), e)
    assert eng.stats()["keyswitch"] == eager_ks      # reading them evaluates nothing more
    assert np.array_equal(ga[1].export(), rest[0]) and np.array_equal(gb[0].export(), rest[1])
    assert eng.stats()["keyswitch"] > eager_ks       # the rows left were evaluated when read
    eng.sync()

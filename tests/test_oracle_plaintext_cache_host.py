"""ResidueEvaluator.hoisted_dot keeps the stacked plaintexts of its last call under the identities of the encoder callables.  An
identity is only unique among live objects: once a list of encoders is collected, the next callable may take the same id(), and a
cache keyed on ids alone would then hand the new call the old plaintexts.  The entry therefore holds its encoders."""
import numpy as np
import pytest

LD = np.longdouble
TRIES = 4000


def _encoder(v):
    return lambda ell, sc: v[:ell]


def test_hoisted_dot_uses_the_plaintexts_of_its_own_call(fa, orc):
    from oracle.residue_eval import RCt, ResidueEvaluator
    # the collision needs an interpreter that hands a freed callable's slot to the next one
    repeat = False
    for _ in range(TRIES):
        f = _encoder(None)
        freed = id(f)
        del f
        g = _encoder(None)
        if id(g) == freed:
            repeat = True
            break
    if not repeat:
        pytest.skip(f"no id() of a dropped callable came back in {TRIES} tries: the collision cannot be constructed here")
    eng = fa.Engine("toy", device=-1, seed=1)
    try:
        key = np.stack([orc.uniform_residues(50 * j, eng.moduli, eng.N) for j in range(2 * eng.dnum_digits)])
        keys = {1: key.reshape(eng.dnum_digits, 2, eng.n_limbs, eng.N)}
        new = lambda: ResidueEvaluator(eng.q, eng.p, eng.psi_q, eng.psi_p, eng.alpha, eng.log_n, keys, eng.params.log_slots)
        ell = 3
        x = RCt(np.stack([orc.uniform_residues(7 + p, eng.q[:ell], eng.N) for p in range(2)]), 1, new().sf[eng.n_q - ell])
        vs = [orc.uniform_residues(100 + s, eng.moduli, eng.N) for s in range(2)]
        want = [new().hoisted_dot(x, [_encoder(v), _encoder(v)], [1]).d for v in vs]    # an evaluator of its own each: nothing cached
        assert not np.array_equal(want[0], want[1])
        rev = new()
        first = _encoder(vs[0])
        freed = id(first)
        assert np.array_equal(rev.hoisted_dot(x, [first, first], [1]).d, want[0])
        del first                                  # the only references left are the evaluator's own, if it keeps any
        # new callables over the OTHER plaintexts until one takes the id of the dropped one; an evaluator that keeps its encoders alive never
        # lets that happen (the check above showed that a freed slot does come back), and then the last one made is as good as any
        for _ in range(TRIES):
            other = _encoder(vs[1])
            if id(other) == freed:
                break
        print("the id of the dropped encoder came back:", id(other) == freed)
        assert np.array_equal(rev.hoisted_dot(x, [other, other], [1]).d, want[1]), "the plaintexts of an earlier call"
        again = _encoder(vs[0])
        assert np.array_equal(rev.hoisted_dot(x, [again, again], [1]).d, want[0])
    finally:
        eng.close()

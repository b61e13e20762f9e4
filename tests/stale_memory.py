"""Harness of tests/test_stale_memory_gpu.py and tests/test_stale_memory_client_gpu.py: three engines of equal arguments and seed (the
pool's fill knob off, w = 1, w = 2), a recorder of what a scenario returns and which operands it used, and the runner that compares."""
import numpy as np
import pytest

from test_default_path_gpu import _evk, _imp, _rev, _same

LD = np.longdouble
KNOB = "FHELIN_POOL_FILL"
WORDS = (0, 1, 2)
SEED = 77


def make_trios(fa):
    """the body of a module-scoped fixture: yields get(preset, tag=None, **overrides) -> [engine with the knob off, with w = 1, with w = 2]
    (the same arguments and the same non-zero seed; the variable is set around each creation and put back), closes them at module end"""
    made = {}

    def get(preset, tag=None, **kw):
        key = (preset, tag, tuple(sorted(kw.items())))          # tag: a trio of its own for scenarios that change the context's keys
        if key not in made:
            engs = []
            for w in WORDS:
                mp = pytest.MonkeyPatch()
                try:
                    if w:
                        mp.setenv(KNOB, str(w))
                    else:
                        mp.delenv(KNOB, raising=False)
                    engs.append(fa.Engine(preset, seed=SEED, **kw))
                finally:
                    mp.undo()
            made[key] = engs
        return made[key]

    yield get
    for engs in made.values():
        for e in engs:
            e.close()
    made.clear()


class Rec:
    """what one run of a scenario on one engine returns and which operands it used"""

    def __init__(self, eng, orc, rnd, k):
        self.eng, self.orc, self.rnd, self.k = eng, orc, rnd, k     # k: the engine's place in the trio
        self.anchor = k == 0                                          # engine 1 is the one compared with the oracle
        self.arrays, self.names, self.watched = [], [], []

    def seed(self, s):
        """input seeds of the round: the second round runs on other inputs"""
        return s + 50021 * self.rnd

    def rev(self, keys):
        return _rev(self.orc, self.eng, keys)

    def watch(self, what, read):
        """something the scenario reads and must leave as it is: read() now, and again in finish()"""
        self.watched.append((what, read, read()))

    def operand(self, ct, what="operand"):
        self.watch(what, lambda: (ct.export().tobytes(), ct.info(), ct.scale_parts()))
        return ct

    def wrapped(self, w, what="wrapped operand"):
        """a wrapped handle has no export(): its compact form holds every residue of c0 and the seed of c1"""
        self.watch(what, lambda: (bytes(w.export_compact()), w.info(), w.wrapped_info()))
        return w

    def plain(self, pt, encodings, what="plaintext"):
        """a plaintext operand: its encodings at (limbs, scale), scale 0 = that limb count's own - the cached blocks the operation reads.
        An encoding is made when first asked for, so this asks before the operation does; a fixed plaintext
        (debug_pt_from_residues) holds exactly one."""
        for ell, sc in encodings:
            self.watch((what, ell), lambda ell=ell, sc=sc: self.eng.pt_export(pt, ell, sc))
        return pt

    def key(self, kind, index=0):
        """an evaluation key the scenario reads (kind 0: relinearisation, 1: rotation `index`)"""
        self.watch(("key", kind, index), lambda: self.eng.key_export(kind, index))

    def imp(self, rev, x, deg=1):
        """the same ciphertext as an engine handle (registered as an operand) and as the oracle's RCt"""
        c, r = _imp(self.eng, rev, x, deg=deg)
        self.operand(c)
        return c, r

    def raw(self, what, arr, want=None):
        arr = np.ascontiguousarray(arr)
        self.arrays.append(arr)
        self.names.append(what)
        if want is not None and self.anchor:
            w = want() if callable(want) else want
            assert arr.dtype == w.dtype and arr.shape == w.shape and arr.tobytes() == w.tobytes(), ("engine 1 vs oracle", what)

    def out(self, what, ct, want=None):
        """a result ciphertext: residues, shape and scale parts; want: the oracle's RCt or residues (or a callable that makes them),
        evaluated on engine 1 only"""
        inf = ct.info()
        self.raw(what, ct.export())
        self.raw(what + " info", np.array([inf["npoly"], inf["ell"], inf["level"], inf["deg"], inf["slots"]], dtype=np.int64))
        self.raw(what + " scale", np.array(ct.scale_parts(), dtype=np.float64))
        if want is not None and self.anchor:
            w = want() if callable(want) else want
            if isinstance(w, np.ndarray):
                assert np.array_equal(self.arrays[-3], w), ("engine 1 vs oracle", what)
            else:
                _same(ct, w, ("engine 1 vs oracle", what))
                hi, lo = ct.scale_parts()
                assert LD(hi) + LD(lo) == w.scale, ("engine 1 vs oracle: scale", what)

    def finish(self):
        for what, read, before in self.watched:
            now = read()
            same = np.array_equal(now, before) if isinstance(before, np.ndarray) else now == before
            assert same, ("operand changed", what)


def run(trio, orc, scenario, rounds=2):
    """the scenario on the three engines, twice: everything equal, counters moved where the knob is on and only there"""
    for rnd in range(rounds):
        recs = []
        for k, eng in enumerate(trio):
            before = eng.pool_fill_stats()
            s = Rec(eng, orc, rnd, k)
            scenario(s)
            eng.sync()
            s.finish()
            after = eng.pool_fill_stats()
            if WORDS[k] == 0:
                assert before == (0, 0) and after == (0, 0), ("the knob is off on engine 1", after)
            else:
                assert after[0] > before[0] and after[1] > before[1], ("no block was filled on engine", k + 1, before, after)
            recs.append(s)
        a = recs[0]
        assert a.arrays, "the scenario returned nothing"
        for k, b in enumerate(recs[1:], start=2):
            assert b.names == a.names
            for what, x, y in zip(a.names, a.arrays, b.arrays):
                same = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                assert same, (f"engine 1 and engine {k} (w = {WORDS[k - 1]}) differ", what, "round", rnd,
                              np.argwhere(x != y)[:4].tolist() if x.shape == y.shape else (x.shape, y.shape))


_KEYS = {}


def keys_for(s, indices, seed, watch=None):
    """uniform rotation 'keys' (parity of integer functions needs no real ones), made once and imported into every engine that asks;
    every one of them is watched as an operand, or those of `watch` where reading all of them back twice would take seconds"""
    eng = s.eng
    tag = (eng.log_n, eng.n_q, eng.n_p, seed)
    have = getattr(eng, "_stale_keys", None)
    if have is None:
        have = eng._stale_keys = {}
    keys = {}
    for r in indices:
        if (tag, r) not in _KEYS:
            _KEYS[(tag, r)] = _evk(s.orc, eng, seed + 17 * (r % 100003))
        keys[r] = _KEYS[(tag, r)]
        if have.get(r) != seed:
            eng.key_import(1, r, keys[r])
            have[r] = seed
        if watch is None or r in watch:
            s.key(1, r)
    return keys


def relin_for(s, seed=31):
    eng = s.eng
    tag = (eng.log_n, eng.n_q, eng.n_p, "relin", seed)
    if tag not in _KEYS:
        _KEYS[tag] = _evk(s.orc, eng, seed)
    if getattr(eng, "_stale_relin", None) != seed:
        eng.key_import(0, 0, _KEYS[tag])
        eng._stale_relin = seed
    s.key(0)
    return _KEYS[tag]

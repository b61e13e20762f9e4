"""Packed formats on the GPU (include/fhelin.h "Packed formats"): the pack and unpack kernels against the Python-int model of the bit
stream, bit for bit, at every width 20..60 in one mixed-width launch; packed ciphertext blobs round-trip every residue, the exact
80-bit scale, degree and slots, and give the handles the compact and the plain import give; sizes equal the formula; malformed
blobs are refused all or nothing."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 4
WIDTHS = list(range(20, 61))
TOY15 = dict(log_n=15, n_q=5, n_p=2, dnum=3, log_slots=14, hamming=64)   # the smallest ring with the 16384 slots of wrapped inputs


def pack_model(v, w):
    """the model: sum(v[j] << (j w)) written little-endian, as u64 words.  64 residues are exactly w words, so the stream is formed
    64 residues at a time and the pieces joined: the same bytes, without shifting a 30 KB integer 4096 times"""
    out = bytearray()
    for g in range(0, len(v), 64):
        stream = 0
        for j, x in enumerate(v[g:g + 64]):
            stream |= int(x) << (j * w)
        out += stream.to_bytes(8 * w, "little")
    return np.frombuffer(bytes(out), dtype="<u8")


def unpack_model(words, w, n):
    """(stream >> (j w)) & (2^w - 1), 64 residues (w words) at a time"""
    raw = np.ascontiguousarray(words, dtype="<u8").tobytes()
    out = []
    for g in range(n // 64):
        stream = int.from_bytes(raw[8 * w * g:8 * w * (g + 1)], "little")
        out += [(stream >> (j * w)) & ((1 << w) - 1) for j in range(64)]
    return np.array(out, dtype=np.uint64)


def pack_all(vs, ws):
    return np.concatenate([pack_model(v, w) for v, w in zip(vs, ws)])


def _rand(rng, w, n):
    return rng.integers(0, 1 << w, n, dtype=np.uint64)


@pytest.fixture(scope="module")
def eng(engine_factory):
    return engine_factory("toy")


@pytest.fixture(scope="module")
def patterns(eng):
    """name -> (vectors [41][N], one per width 20..60, and their packed model), computed once"""
    N = eng.N
    rng = np.random.default_rng(20)
    j = np.arange(N)
    pats = {
        "even all-ones": [np.where(j % 2 == 0, (1 << w) - 1, 0).astype(np.uint64) for w in WIDTHS],
        "odd all-ones": [np.where(j % 2 == 1, (1 << w) - 1, 0).astype(np.uint64) for w in WIDTHS],
        "single bit j mod w": [(np.uint64(1) << (j % w).astype(np.uint64)) for w in WIDTHS],
        "random": [_rand(rng, w, N) for w in WIDTHS],
    }
    return {k: (np.stack(v), [pack_model(x, w) for x, w in zip(v, WIDTHS)]) for k, v in pats.items()}


@pytest.mark.parametrize("name", ["even all-ones", "odd all-ones", "single bit j mod w", "random"])
def test_kernels_equal_the_int_model_at_every_width(eng, patterns, name):
    vs, packed = patterns[name]
    for order in (list(range(len(WIDTHS))), list(range(len(WIDTHS)))[::-1]):   # one mixed-width call of 41 vectors, then reversed
        ws = [WIDTHS[i] for i in order]
        want = np.concatenate([packed[i] for i in order])
        got = eng.debug_pack(vs[order], ws)
        assert got.size == sum(eng.N * w // 64 for w in ws)
        assert np.array_equal(got, want), name
        assert np.array_equal(eng.debug_unpack(want, ws), vs[order]), name


def test_toy_chain_moduli_boundary_vectors(eng):
    mods = [int(m) for m in eng.moduli]
    ws = [m.bit_length() for m in mods]
    assert all(20 <= w <= 60 for w in ws)
    hi = np.stack([np.full(eng.N, m - 1, dtype=np.uint64) for m in mods])
    got = eng.debug_pack(hi, ws)
    assert np.array_equal(got, pack_all(hi, ws))
    assert np.array_equal(eng.debug_unpack(got, ws), hi)
    zero = np.zeros_like(hi)
    got = eng.debug_pack(zero, ws)
    assert not got.any() and got.size == sum(eng.N * w // 64 for w in ws)
    assert not eng.debug_unpack(got, ws).any()


def test_unpack_of_random_words_and_both_round_trips(eng):
    rng = np.random.default_rng(21)
    ws = [60, 20, 33, 52, 53, 47]
    words = [rng.integers(0, 1 << 64, eng.N * w // 64, dtype=np.uint64) for w in ws]   # every bit of a stream is a residue bit
    y = np.concatenate(words)
    x = eng.debug_unpack(y, ws)
    for i, w in enumerate(ws):
        assert np.array_equal(x[i], unpack_model(words[i], w, eng.N)), w
    assert np.array_equal(eng.debug_pack(x, ws), y)                                   # pack(unpack(y)) == y
    v = np.stack([_rand(rng, w, eng.N) for w in ws])
    assert np.array_equal(eng.debug_unpack(eng.debug_pack(v, ws), ws), v)             # unpack(pack(x)) == x


def test_hook_refusals(fa, eng):
    v = np.zeros((1, eng.N), dtype=np.uint64)
    for w in (19, 61, 0, 64):
        with pytest.raises(fa.FhelinError) as ex:
            eng.debug_pack(v, [w])
        assert ex.value.code == ERR_ARG, w
        with pytest.raises(fa.FhelinError) as ex:
            eng.debug_unpack(np.zeros(eng.N * 20 // 64, dtype=np.uint64), [w])
        assert ex.value.code == ERR_ARG, w
    v[0, 5] = 1 << 20                                      # at 2^w
    with pytest.raises(fa.FhelinError) as ex:
        eng.debug_pack(v, [20])
    assert ex.value.code == ERR_ARG
    with pytest.raises(fa.FhelinError) as ex:              # a word count that is not the widths'
        eng.debug_unpack(np.zeros(eng.N * 20 // 64 + 1, dtype=np.uint64), [20])
    assert ex.value.code == ERR_ARG


def test_rate_hook_times_every_step(fa, eng):
    ms = eng.debug_pack_rate([55, 52, 53, 60], reps=2)     # the probe's hook: pack, copy, unpack, copy per round
    assert ms.shape == (2, 4) and (ms > 0).all()
    with pytest.raises(fa.FhelinError) as ex:
        eng.debug_pack_rate([61], reps=1)
    assert ex.value.code == ERR_ARG


# ---- ciphertext blobs


def _client(fa, preset="toy", seed=77, **over):
    e = fa.Engine(preset, seed=seed, **over)
    e.keygen()
    e.gen_relin_key()
    return e


def _widths(e, ell):
    return [int(m).bit_length() for m in e.moduli[:ell]]


def _formula(e, ell, stored, count=0):
    return 112 + 8 * ell + 8 * ((count + 1) // 2) + stored * sum(e.N * w // 8 for w in _widths(e, ell))


def _same(a, b):
    ia, ib = a.info(), b.info()
    assert (ia["npoly"], ia["ell"], ia["deg"], ia["slots"]) == (ib["npoly"], ib["ell"], ib["deg"], ib["slots"])
    assert a.scale_parts() == b.scale_parts()
    assert np.array_equal(a.export(), b.export())


@pytest.fixture(scope="module")
def client(fa):
    e = _client(fa)
    yield e
    e.close()


def test_full_round_trips_sizes_and_mixed_limb_counts(fa, client):
    e = client
    rng = np.random.default_rng(22)
    n = 1 << e.params.log_slots
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    fresh = e.encrypt(x)
    prod = e.mult(fresh, e.encrypt(y))                     # degree 2, before its rescale
    assert prod.info()["deg"] == 2
    low = e.encrypt(y, level=2)
    lower = e.encrypt(x, level=3)
    prod2 = e.mult(e.encrypt(y), fresh)                    # a second product of the same limb count: one (stored, ell) group of two
    cts = [fresh, prod, low, lower, prod2]
    assert len({c.info()["ell"] for c in cts}) == 3        # three limb counts through one import call
    blobs = [c.export_packed() for c in cts]
    for c, b in zip(cts, blobs):
        i = c.info()
        assert len(b) == _formula(e, i["ell"], i["npoly"]) == c.packed_bytes()
        assert len(b) < 8 * i["npoly"] * i["ell"] * e.N    # smaller than the bare words of the plain export
        assert fa.packed_info(b) == dict(log_n=e.log_n, ell=i["ell"], deg=i["deg"], slots=i["slots"], stored=i["npoly"], count=0)
        assert struct.unpack_from("<2d", b, 32) == c.scale_parts()
    back = e.import_packed(blobs)
    for c, r in zip(cts, back):
        _same(c, r)
        assert np.array_equal(e.decrypt(c), e.decrypt(r))
    assert np.allclose(e.decrypt(back[0]), x, atol=1e-6)
    # an imported value computes like the original
    assert np.array_equal(e.rescale(back[1]).export(), e.rescale(prod).export())
    assert e.import_packed([]) == []


def test_seeded_form_equals_the_compact_round_trip(fa, client):
    e = client
    e.set_seeded_encryption(True)
    try:
        rng = np.random.default_rng(23)
        n = 1 << e.params.log_slots
        cts = e.encrypt_batch(rng.uniform(-1, 1, (2, n))) + [e.encrypt(rng.uniform(-1, 1, n), level=2)]
        packed = [c.export_packed(seeded=True) for c in cts]
        compact = [c.export_compact() for c in cts]
        for c, p, k in zip(cts, packed, compact):
            ell = c.info()["ell"]
            assert len(p) == _formula(e, ell, 1) == c.packed_bytes(seeded=True) and len(p) < len(k)
            assert fa.packed_info(p)["stored"] == 1
            assert p[48:96] == k[48:96]                    # nonce, seed and the digest of the unpacked c0: the compact blob's
        for c, a, b in zip(cts, e.import_packed(packed), e.import_compact(compact)):
            _same(a, b)
            _same(a, c)
        # the full form of a seeded encryption carries both components and no seed
        full = cts[0].export_packed()
        assert fa.packed_info(full)["stored"] == 2 and not any(full[48:88])
        _same(e.import_packed([full])[0], cts[0])
        # an operation's result has no seeded form
        s = e.add(cts[0], cts[1])
        for fn in (lambda: s.export_packed(seeded=True), lambda: s.packed_bytes(seeded=True)):
            with pytest.raises(fa.FhelinError) as ex:
                fn()
            assert ex.value.code == ERR_STATE
    finally:
        e.set_seeded_encryption(False)
    with pytest.raises(fa.FhelinError) as ex:              # a public-key encryption neither
        e.encrypt(np.ones(4)).export_packed(seeded=True)
    assert ex.value.code == ERR_STATE


def _inputs(S, seed):
    rng = np.random.default_rng(seed)
    return dict(cls=rng.uniform(-1, 1, 128), pos=rng.uniform(-1, 1, (S, 128)), E_w=rng.uniform(-0.1, 0.1, (32, S + 1)),
                E_b=rng.uniform(-0.1, 0.1, 32), F_w=rng.uniform(-0.1, 0.1, (32, S + 1)), F_b=rng.uniform(-0.1, 0.1, 32),
                emb=rng.uniform(-1, 1, (S, 128)))


def test_wrapped_inputs_through_the_seeded_form(fa):
    e = fa.Engine("toy13", seed=31, **TOY15)
    try:
        e.keygen()
        e.gen_rotation_keys(fa.circuit_rotation_indices())
        S = 3
        ws = e.client_ingest_wrapped(**_inputs(S, 6), targets=[e.n_q] * 50 + [2] * (64 + S + 1 - 50))
        packed = [w.export_packed(seeded=True) for w in ws]
        compact = [w.export_compact() for w in ws]
        for w, p, k in zip(ws, packed, compact):
            i = w.wrapped_info()
            assert len(p) == _formula(e, i["ell"] + 1, 1, i["count"]) == w.packed_bytes(seeded=True) and len(p) < len(k)
            assert fa.packed_info(p)["count"] == i["count"] and fa.packed_info(p)["ell"] == i["ell"] + 1
            with pytest.raises(fa.FhelinError) as ex:      # a wrapped input has no full form
                w.export_packed()
            assert ex.value.code == ERR_ARG
        a, b = e.import_packed(packed), e.import_compact(compact)
        assert [w.wrapped_info() for w in a] == [w.wrapped_info() for w in b] == [w.wrapped_info() for w in ws]
        for x, y in zip(e.unwrap_inputs(a), e.unwrap_inputs(b)):
            _same(x, y)
    finally:
        e.close()


def _flip_payload_bit(blob, bit):
    H = struct.unpack_from("<I", blob, 12)[0]
    b = bytearray(blob)
    b[H + bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def test_all_or_nothing(fa, client):
    e = client
    rng = np.random.default_rng(24)
    n = 1 << e.params.log_slots
    cts = [e.encrypt(rng.uniform(-1, 1, n), level=l) for l in (0, 1, 0)]
    blobs = [c.export_packed() for c in cts]
    ell = cts[1].info()["ell"]
    ws = _widths(e, ell)
    # one payload bit of the second blob: inside residue 7 of the second limb vector of c1
    bit = 8 * (sum(e.N * w // 8 for w in ws) + e.N * ws[0] // 8) + 7 * ws[1] + 3
    with pytest.raises(fa.FhelinError) as ex:
        e.import_packed([blobs[0], _flip_payload_bit(blobs[1], bit), blobs[2]])
    assert ex.value.code == ERR_ARG and "blob 1" in str(ex.value)
    # a residue field overwritten with 2^w - 1 (not below its modulus): residue 5 of the first vector
    H = struct.unpack_from("<I", blobs[1], 12)[0]
    stream = int.from_bytes(blobs[1][H:], "little") | (((1 << ws[0]) - 1) << (5 * ws[0]))
    over = blobs[1][:H] + stream.to_bytes(len(blobs[1]) - H, "little")
    with pytest.raises(fa.FhelinError) as ex:
        e.import_packed([blobs[0], over])
    assert ex.value.code == ERR_ARG and "range" in str(ex.value)
    # a blob of another chain, a truncated one
    wrong_mod = bytearray(blobs[0])
    wrong_mod[112] ^= 2
    for bad in (bytes(wrong_mod), blobs[0][:-8]):
        with pytest.raises(fa.FhelinError) as ex:
            e.import_packed([blobs[2], bad])
        assert ex.value.code == ERR_ARG
    # the context is still usable
    good = e.import_packed(blobs)
    for c, r in zip(cts, good):
        _same(c, r)


# ---- key sets

ERR_KEY = 5
ROT = {1: 3, 2: 7, 5: 4}      # rotation index -> cap on toy13 (n_q = 7: index 2 stays uncapped)
RELIN_CAP = 3


def _g(e, r):
    return pow(5, r % (e.N // 2), 2 * e.N)


def _key_client(fa):
    e = fa.Engine("toy13", seed=77)
    e.set_seeded_keys(True)
    e.set_key_caps([(2, _g(e, 1), ROT[1]), (1, 0, RELIN_CAP)] + [(2, _g(e, 5), ROT[5])])
    e.keygen()
    e.gen_relin_key()
    e.gen_rotation_keys(list(ROT))
    e.gen_conj_key()
    return e


def _set_table(data):
    """(head bytes before the moduli, entry size, data_offset, entries) of any of the three key-set formats"""
    magic = data[:8]
    version, n_keys = struct.unpack_from("<II", data, 8)
    prm = struct.unpack_from("<9i", data, 16)
    head = {b"FHELINEK": 96, b"FHELINEC": 128, b"FHELINEP": 136}[magic]
    size = 48 if magic == b"FHELINEP" or version == 2 else 40
    base = head + 8 * (prm[1] + prm[4])
    ents = []
    for k in range(n_keys):
        kind, digits, g, off, words, dg = struct.unpack_from("<IIQQQQ", data, base + size * k)
        max_ell = struct.unpack_from("<I", data, base + size * k + 40)[0] if size == 48 else prm[1]
        ents.append(dict(kind=kind, digits=digits, galois=g, offset=off, words=words, digest=dg, max_ell=max_ell))
    return head, base + size * n_keys, struct.unpack_from("<Q", data, 80)[0], ents


def _rand_ct(e, ell, seed):
    rng = np.random.default_rng(seed)
    return e.ct_import(np.stack([np.stack([rng.integers(0, int(q), e.N, dtype=np.uint64) for q in e.q[:ell]]) for _ in range(2)]))


@pytest.fixture(scope="module")
def key_client(fa):
    e = _key_client(fa)
    yield e
    e.close()


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_packed_key_set_round_trip(fa, key_client, tmp_path, compact):
    b = key_client
    plain, packed, again = (str(tmp_path / n) for n in ("b.evk", "b.evp", "b2.evk"))
    b.save_eval_keys(plain, compact=compact)
    before = open(plain, "rb").read()
    b.save_evalkeys_packed(packed, compact=compact)
    b.save_eval_keys(again, compact=compact)
    assert open(again, "rb").read() == before              # the unpacked savers write what they wrote before a packed save
    data = open(packed, "rb").read()
    N, n_q, n_p = b.N, b.n_q, b.n_p
    w = [int(m).bit_length() for m in b.moduli]
    head, table_end, data_offset, ents = _set_table(data)
    assert data[:8] == b"FHELINEP" and struct.unpack_from("<I", data, 8)[0] == 1
    halves = 1 if compact else 2
    assert struct.unpack_from("<II", data, 128) == (halves, 0)
    assert data[96:128] == (b.key_set_seed() if compact else bytes(32))
    assert data_offset == -(-table_end // 4096) * 4096
    caps = {(1, 0): RELIN_CAP, (2, _g(b, 1)): ROT[1], (2, _g(b, 5)): ROT[5]}
    at = data_offset
    assert len(ents) == 1 + 1 + 1 + len(ROT)
    for en in ents:
        cap = n_q if en["kind"] == 0 else caps.get((en["kind"], en["galois"]), n_q)
        bits = sum(w[:cap]) + (sum(w[n_q:]) if en["kind"] else 0)
        digits = 0 if en["kind"] == 0 else -(-cap // b.alpha)
        assert (en["max_ell"], en["digits"], en["offset"]) == (cap, digits, at)
        assert en["words"] == (halves if en["kind"] == 0 else digits * halves) * bits * (N // 64)
        at += 8 * en["words"]
    assert len(data) == at < len(before)                   # the formula, exactly; smaller than the unpacked set
    # every table digest is the unpacked set's
    assert [en["digest"] for en in ents] == [en["digest"] for en in _set_table(before)[3]]
    # the payload is the model's: the b half of the first digit of rotation key 1, row 0
    en = next(x for x in ents if (x["kind"], x["galois"]) == (2, _g(b, 1)))
    row = np.frombuffer(data, dtype="<u8", count=N * w[0] // 64, offset=en["offset"])
    assert np.array_equal(row, pack_model(b.key_export(1, 1)[0, 0, 0], w[0]))
    c = fa.Engine.from_eval_keys(packed, seed=5)
    try:
        for r, cap in ROT.items():
            assert c.key_info(1, r) == dict(digits=-(-cap // b.alpha), max_ell=cap, seeded=compact)
            assert np.array_equal(c.key_export(1, r), b.key_export(1, r)), r
        for kind in (0, 2):
            assert np.array_equal(c.key_export(kind), b.key_export(kind)), kind
        # a rotation and a mult at the cap give the client's residues; above the cap the switch is still refused
        def some(e_):
            return [e_.rotate(_rand_ct(e_, ROT[1], 1), 1).export(), e_.mult(_rand_ct(e_, RELIN_CAP, 2), _rand_ct(e_, RELIN_CAP, 3)).export(),
                    e_.rotate(_rand_ct(e_, n_q, 4), 2).export()]
        for x, y in zip(some(b), some(c)):
            assert np.array_equal(x, y)
        for fn in (lambda: c.rotate(_rand_ct(c, ROT[1] + 1, 1), 1), lambda: c.mult(_rand_ct(c, RELIN_CAP + 1, 2), _rand_ct(c, RELIN_CAP + 1, 3))):
            with pytest.raises(fa.FhelinError) as ei:
                fn()
            assert ei.value.code == ERR_KEY
        # what it loaded it writes back: packed and unpacked, byte for byte
        back = str(tmp_path / "c.evp")
        c.save_evalkeys_packed(back, compact=compact)
        assert open(back, "rb").read() == data
        c.save_eval_keys(back, compact=compact)
        assert open(back, "rb").read() == before
    finally:
        c.close()
    # a flipped payload bit, a residue field at 2^w - 1: refused, and the context stays empty
    flip = bytearray(data)
    flip[en["offset"] + 11] ^= 4
    over = bytearray(data)
    stream = int.from_bytes(over[en["offset"]:en["offset"] + 8 * w[0]], "little") | (((1 << w[0]) - 1) << (9 * w[0]))
    over[en["offset"]:en["offset"] + 8 * w[0]] = stream.to_bytes(8 * w[0], "little")
    c2 = fa.Engine("toy13")
    try:
        for name, blob in (("flip", flip), ("range", over)):
            p = str(tmp_path / "bad.evp")
            open(p, "wb").write(bytes(blob))
            with pytest.raises(fa.FhelinError) as ei:
                c2.load_eval_keys(p)
            assert ei.value.code == ERR_ARG, name
            with pytest.raises(fa.FhelinError) as ei:
                c2.key_info(1, 1)
            assert ei.value.code == ERR_KEY, name
        c2.load_eval_keys(packed)
        assert np.array_equal(c2.key_export(1, 1), b.key_export(1, 1))
    finally:
        c2.close()


def test_packed_compact_needs_seeded_keys(fa, client, tmp_path):
    with pytest.raises(fa.FhelinError) as ei:
        client.save_evalkeys_packed(str(tmp_path / "x.evp"), compact=True)
    assert ei.value.code == ERR_STATE
    client.save_evalkeys_packed(str(tmp_path / "x.evp"))   # the full form of ordinary keys
    c = fa.Engine.from_eval_keys(str(tmp_path / "x.evp"))
    try:
        assert np.array_equal(c.key_export(0), client.key_export(0))
    finally:
        c.close()


def test_end_to_end_without_the_secret(fa, tmp_path):
    """client: ingest_wrapped -> export_packed; server (evaluation context from the packed compact set): import_packed -> unwrap_inputs
    -> sanitize -> export_packed; client: import_packed -> decrypt.  Against the same run through the unpacked formats."""
    cl = fa.Engine("toy13", seed=42, **TOY15)
    try:
        cl.set_seeded_keys(True)
        cl.keygen()
        cl.gen_rotation_keys(fa.circuit_rotation_indices())
        packed_set, plain_set = str(tmp_path / "s.evp"), str(tmp_path / "s.evc")
        cl.save_evalkeys_packed(packed_set, compact=True)
        cl.save_eval_keys(plain_set, compact=True)
        ws = cl.client_ingest_wrapped(**_inputs(2, 9))
        up = [w.export_packed(seeded=True) for w in ws]
        up_plain = [w.export_compact() for w in ws]
        assert sum(map(len, up)) < sum(map(len, up_plain))
        sv, sv_plain = fa.Engine.from_eval_keys(packed_set, seed=43), fa.Engine.from_eval_keys(plain_set, seed=43)
        try:
            outs = sv.unwrap_inputs(sv.import_packed(up))
            outs_plain = sv_plain.unwrap_inputs(sv_plain.import_compact(up_plain))
            assert len(outs) == len(outs_plain) > 0
            for x, y in zip(outs, outs_plain):
                _same(x, y)
            reply = sv.sanitize(outs[:2], flood_bits=24, out_ell=2)
            blobs = [r.export_packed() for r in reply]
            for r, blob in zip(reply, blobs):
                assert len(blob) == _formula(cl, 2, 2) < 112 + 16 + 8 * 2 * 2 * cl.N
            want = [cl.decrypt(c) for c in cl.unwrap_inputs(ws)[:2]]
        finally:
            sv.close()
            sv_plain.close()
        # the reply differs from the client's own unwrap by the flood, uniform below 2^24 per coefficient: a slot sees the sum of
        # 2 * slots such terms over the scale, standard deviation sqrt(slots) * 2^24 / sqrt(3) / scale (about 2^-22 at 2^52); the
        # encryption of zero and the rescales are far below that.  Eight standard deviations bound the largest of 16384 slots.
        for blob, wv in zip(blobs, want):
            back = cl.import_packed([blob])[0]
            bound = 8 * np.sqrt(back.slots) * 2.0 ** 24 / np.sqrt(3) / sum(back.scale_parts())
            assert bound < 2.0 ** -17
            assert np.abs(cl.decrypt(back) - wv).max() < bound
    finally:
        cl.close()

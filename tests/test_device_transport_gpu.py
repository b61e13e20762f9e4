"""Device transport on the GPU (include/fhelin.h "Device transport"): many ciphertexts through the frames of one device buffer.
Everything is compared bit for bit.  The frame layout is checked against a model written here: a raw frame is the bytes of export(),
a packed frame is every limb vector as the Python-int bit stream sum(v[j] << (j w)) at w = bitlen(q_l), little-endian.  The host
synchronisations of a call are read from the context's counter (Engine.sync_count), which only Context::sync() moves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = 1
RAW, PACKED = 0, 1
FORMATS = pytest.mark.parametrize("fmt", [RAW, PACKED], ids=["raw", "packed"])


def pack_model(v, w):
    """the packed limb vector of the residues v at width w, as bytes; 64 residues are exactly w words, so the stream is formed 64
    residues at a time and the pieces joined (the same bytes as one big integer)"""
    out = bytearray()
    for g in range(0, len(v), 64):
        stream = 0
        for j, x in enumerate(v[g:g + 64]):
            stream |= int(x) << (j * w)
        out += stream.to_bytes(8 * w, "little")
    return bytes(out)


def frame_model(e, limbs, fmt):
    """the frame of residues [npoly][ell][N]"""
    limbs = np.ascontiguousarray(limbs, dtype="<u8")
    if fmt == RAW:
        return limbs.tobytes()
    return b"".join(pack_model(vec, int(e.q[l]).bit_length()) for comp in limbs for l, vec in enumerate(comp))


def frame_formula(e, npoly, ell, fmt):
    if fmt == RAW:
        return npoly * ell * e.N * 8
    return npoly * sum(e.N * int(q).bit_length() // 8 for q in e.q[:ell])


def _round16(n):
    return -(-n // 16) * 16


def _rand_limbs(e, npoly, ell, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.integers(0, int(q), e.N, dtype=np.uint64) for q in e.q[:ell]]) for _ in range(npoly)])


def _crafted(e, ell, kind):
    """residues on the boundaries of the packed width: all q_l - 1, all 0, alternating q_l - 1 / 0"""
    j = np.arange(e.N)
    top = [np.full(e.N, int(q) - 1, dtype=np.uint64) for q in e.q[:ell]]
    one = {"top": top, "zero": [np.zeros(e.N, dtype=np.uint64)] * ell,
           "alternating": [np.where(j % 2 == 0, t, np.uint64(0)).astype(np.uint64) for t in top]}[kind]
    return np.stack([np.stack(one)] * 2)


def _facts(c):
    return c.export(), c.info(), c.scale_parts()


def _same(got, want):
    """got: a handle; want: (export, info, scale_parts) of its source"""
    limbs, info, scale = want
    assert got.info() == info
    assert got.scale_parts() == scale
    assert np.array_equal(got.export(), limbs)


def _device_bytes(frames):
    import torch
    t = torch.from_numpy(np.frombuffer(b"".join(frames), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()                                      # a call without a stream expects finished frames
    return t


def _fresh_buffer(n, stride, wait=True):
    """n frames of 0xA5; wait: the fill has finished (a call without a stream is not ordered behind torch's work)"""
    import torch
    t = torch.full((n, stride), 0xA5, dtype=torch.uint8, device="cuda")
    if wait:
        torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def client(fa):
    e = fa.Engine("toy", seed=77)
    e.keygen()
    e.gen_relin_key()
    yield e
    e.close()


@pytest.fixture(scope="module")
def zoo(client):
    """handles of mixed shapes and what each of them holds, computed once: limb counts 1, 3 and 6, degree 1 and 2, a
    three-component handle, and residues crafted to sit on the packed width's boundaries"""
    e = client
    rng = np.random.default_rng(40)
    n = 1 << e.params.log_slots
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    fresh = e.encrypt(x)
    cts = [
        fresh,                                                    # 6 limbs, degree 1
        e.mult(fresh, e.encrypt(y)),                              # 6 limbs, degree 2 (before its rescale)
        e.encrypt(y, level=3),                                    # 3 limbs
        e.ct_import(_rand_limbs(e, 2, 1, 41), slots=n),           # 1 limb
        e.ct_import(_rand_limbs(e, 2, 3, 42), deg=2),             # 3 limbs, degree 2, slots left unset
        e.ct_import(_rand_limbs(e, 3, 3, 43), deg=2, slots=n),    # three components
        e.ct_import(_crafted(e, 6, "top"), slots=n),
        e.ct_import(_crafted(e, 6, "zero"), slots=n),
        e.ct_import(_crafted(e, 6, "alternating"), slots=n),
    ]
    facts = [_facts(c) for c in cts]
    assert sorted({f[1]["ell"] for f in facts}) == [1, 3, 6] and {f[1]["deg"] for f in facts} == {1, 2}
    assert {f[1]["npoly"] for f in facts} == {2, 3}
    frames = {fmt: [frame_model(e, f[0], fmt) for f in facts] for fmt in (RAW, PACKED)}
    return cts, facts, frames


@FORMATS
def test_round_trip_of_mixed_shapes(client, zoo, fmt):
    import torch
    e = client
    cts, facts, _ = zoo
    sizes, most = e.frame_bytes(cts, fmt)
    stride = _round16(most)
    buf = torch.empty((len(cts), stride), dtype=torch.uint8, device="cuda")
    meta = e.export_device_many(cts, buf.data_ptr(), stride, buf.numel(), fmt)
    back = e.import_device_many(buf.data_ptr(), stride, meta)
    assert len(back) == len(cts)
    for r, f in zip(back, facts):
        _same(r, f)
    for c, f in zip(cts, facts):                                  # the sources are what they were
        _same(c, f)


@FORMATS
def test_frame_layout_equals_the_model(client, zoo, fmt):
    e = client
    cts, facts, frames = zoo
    sizes, most = e.frame_bytes(cts, fmt)
    assert sizes == [frame_formula(e, f[1]["npoly"], f[1]["ell"], fmt) for f in facts] and most == max(sizes)
    if fmt == PACKED:
        assert all(s < frame_formula(e, f[1]["npoly"], f[1]["ell"], RAW) for s, f in zip(sizes, facts))
    stride = _round16(most) + 48                                  # every frame is followed by bytes that are not its own
    buf = _fresh_buffer(len(cts), stride)
    meta = e.export_device_many(cts, buf.data_ptr(), stride, buf.numel(), fmt)
    host = buf.cpu().numpy()
    for i, (f, size) in enumerate(zip(facts, sizes)):
        assert host[i, :size].tobytes() == frames[fmt][i], i
        assert (host[i, size:] == 0xA5).all(), i                  # nothing past a payload is written
        hi, lo = f[2]
        assert meta[i].tolist() == [f[1]["npoly"], f[1]["ell"], f[1]["deg"], f[1]["slots"], hi, lo, size, fmt], i


def test_export_refusals_that_need_handles(fa, client, zoo):
    e = client
    cts, _, _ = zoo
    sizes, most = e.frame_bytes(cts[:2], PACKED)
    buf = _fresh_buffer(2, most)
    for what, args in {"stride below a payload": (most - 16, 2 * most), "capacity below n strides": (most, 2 * most - 16),
                       "stride not a multiple of 16": (most + 8, 4 * most)}.items():
        with pytest.raises(fa.FhelinError) as ei:
            e.export_device_many(cts[:2], buf.data_ptr(), args[0], args[1], PACKED)
        assert ei.value.code == ERR_ARG, what
    with pytest.raises(fa.FhelinError) as ei:
        e.export_device_many(cts[:2], buf.data_ptr(), most, 2 * most, 2)
    assert ei.value.code == ERR_ARG
    assert (buf.cpu().numpy() == 0xA5).all()                      # a refused call wrote nothing


@pytest.fixture(scope="module")
def rot_eng(fa):
    e = fa.Engine("toy13", seed=7)
    e.keygen()
    e.gen_relin_key()
    e.gen_rotation_keys(fa.circuit_rotation_indices())
    yield e
    e.close()


@FORMATS
def test_deferred_rows_are_forced_and_exported_together(rot_eng, fmt):
    e = rot_eng
    rng = np.random.default_rng(44)
    n = 1 << e.params.log_slots
    cts = e.encrypt_batch(rng.uniform(-1, 1, (4, n)))
    w = e.encode(rng.uniform(-1, 1, n))
    rows = e.matmulRE(cts, w, None)                               # deferred: nothing is read here
    sizes, most = e.frame_bytes(rows[1:], fmt)
    buf = _fresh_buffer(3, most)
    e.export_device_many(rows[1:], buf.data_ptr(), most, buf.numel(), fmt)
    host = buf.cpu().numpy()
    again = e.matmulRE(cts, w, None)                              # the same rows, forced and exported one by one
    for k in range(3):
        assert host[k, :sizes[k]].tobytes() == frame_model(e, again[1 + k].export(), fmt), k


def test_two_engines_of_one_seed_continue_from_the_frames(fa):
    import torch
    a, b = fa.Engine("toy13", seed=11), fa.Engine("toy13", seed=11)
    try:
        for e in (a, b):
            e.keygen()
            e.gen_rotation_keys([1, 2, 3])
        rng = np.random.default_rng(45)
        n = 1 << a.params.log_slots
        hi = a.mult_plain_batch(a.rotate_batch(a.encrypt_batch(rng.uniform(-1, 1, (3, n))), 1), a.encode(rng.uniform(-1, 1, n)))
        lo = a.mult_plain_batch(a.rotate_batch(a.encrypt_batch(rng.uniform(-1, 1, (2, n)), level=2), 1),
                                a.encode(rng.uniform(-1, 1, n), level=2))
        rows = [hi[0], lo[0], hi[1], lo[1], hi[2]]                # two shapes, interleaved
        shape = [0, 1, 0, 1, 0]
        ells = (hi[0].info()["ell"], lo[0].info()["ell"])
        assert ells[0] == ells[1] + 2 and all(c.info()["deg"] == 2 for c in rows)   # products before their rescale
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            stride = _round16(a.frame_bytes(rows, PACKED)[1])
            buf = torch.empty((len(rows), stride), dtype=torch.uint8, device="cuda")
            meta = a.export_device_many(rows, buf.data_ptr(), stride, buf.numel(), PACKED, stream=side.cuda_stream)
            got = b.import_device_many(buf.data_ptr(), stride, meta, stream=side.cuda_stream)
        for s in (0, 1):                                          # one block per shape, its rows back to back in frame order
            addr = [c.debug_addr() for c, k in zip(got, shape) if k == s]
            words = 2 * ells[s] * b.N
            assert len({blk for _, blk in addr}) == 1 and addr[0][1] != 0
            assert [d for d, _ in addr] == [addr[0][1] + 8 * words * k for k in range(len(addr))]
        for r, g in zip(rows, got):
            _same(g, _facts(r))
        for s in (0, 1):
            mine = [c for c, k in zip(rows, shape) if k == s]
            theirs = [c for c, k in zip(got, shape) if k == s]
            for x, y in zip(a.rescale_batch(a.rotate_sum(mine, [1, 2, 3])), b.rescale_batch(b.rotate_sum(theirs, [1, 2, 3]))):
                _same(y, _facts(x))
        side.synchronize()
    finally:
        a.close()
        b.close()


def test_stream_contract(client, zoo):
    import torch
    e = client
    cts, facts, frames = zoo
    sizes, most = e.frame_bytes(cts, PACKED)
    stride = _round16(most)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        buf = _fresh_buffer(len(cts), stride, wait=False)         # the fill is queued on that stream: the export is ordered behind it
        before = e.sync_count()
        meta = e.export_device_many(cts, buf.data_ptr(), stride, buf.numel(), PACKED, stream=side.cuda_stream)
        copy = buf.clone()                                        # torch's copy on that stream, right after the export
        back = e.import_device_many(buf.data_ptr(), stride, meta, stream=side.cuda_stream)
        assert e.sync_count() == before                           # no host synchronisation in either call
        checked = e.import_device_many(buf.data_ptr(), stride, meta, check=True, stream=side.cuda_stream)
        assert e.sync_count() == before + 1                       # the range check's download: exactly one
    side.synchronize()
    host = copy.cpu().numpy()
    for i, size in enumerate(sizes):
        assert host[i, :size].tobytes() == frames[PACKED][i], i
    for r, c, f in zip(back, checked, facts):
        _same(r, f)
        _same(c, f)
    # without a stream: one synchronisation per call, whatever the number of ciphertexts; the range check rides on it
    buf = _fresh_buffer(len(cts), stride)
    before = e.sync_count()
    meta = e.export_device_many(cts, buf.data_ptr(), stride, buf.numel(), PACKED)
    assert e.sync_count() == before + 1
    back = e.import_device_many(buf.data_ptr(), stride, meta)
    assert e.sync_count() == before + 2
    checked = e.import_device_many(buf.data_ptr(), stride, meta, check=True)
    assert e.sync_count() == before + 3
    for r, c, f in zip(back, checked, facts):
        _same(r, f)
        _same(c, f)
    # torch's default stream has the handle 0, which means "no stream": under its HIP name it is a stream like the side stream
    stride = _round16(e.frame_bytes(cts, RAW)[1])
    buf = _fresh_buffer(len(cts), stride, wait=False)
    before = e.sync_count()
    meta = e.export_device_many(cts, buf.data_ptr(), stride, buf.numel(), RAW, stream=e.STREAM_LEGACY)
    copy = buf.clone()
    back = e.import_device_many(buf.data_ptr(), stride, meta, stream=e.STREAM_LEGACY)
    assert e.sync_count() == before
    host = copy.cpu().numpy()
    for i, (r, f) in enumerate(zip(back, facts)):
        assert host[i, :len(frames[RAW][i])].tobytes() == frames[RAW][i], i
        _same(r, f)


class _WorldOfOne:
    """a stand-in for torch.distributed with one rank: device tensors (nccl), collectives that copy"""

    class ReduceOp:
        MAX = "max"

    def get_backend(self):
        return "nccl"

    def get_rank(self):
        return 0

    def get_world_size(self):
        return 1

    def all_reduce(self, t, op=None):
        pass

    def all_gather(self, out, t):
        out[0].copy_(t)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "raw"])
def test_all_gather_indexed_takes_the_single_buffer_path(client, zoo, packed, monkeypatch):
    from fhe_linformer_amd import shard
    e = client
    cts, facts, _ = zoo
    pick = [0, 2, 1, 4, 8]                                        # five rows of two shapes (6 and 3 limbs)
    assert sorted({facts[i][1]["ell"] for i in pick}) == [3, 6]
    transport = shard.EngineTransport(e, device=True, packed=packed)
    assert shard.EngineTransport(e, device=True).packed is True and transport.format == (PACKED if packed else RAW)

    def refuse(*a, **kw):
        raise AssertionError("the per-ciphertext path ran")
    monkeypatch.setattr(transport, "pack", refuse)
    monkeypatch.setattr(transport, "unpack", refuse)
    local = {10 + k: cts[i] for k, i in enumerate(pick)}
    before = e.sync_count()
    got = shard._all_gather_indexed(_WorldOfOne(), transport, local, [sorted(local)])
    assert e.sync_count() == before                               # no host synchronisation per row: none at all
    assert sorted(got) == sorted(local)
    for k, i in enumerate(pick):
        _same(got[10 + k], facts[i])


def test_single_ciphertext_entry_points(client, zoo):
    """fhelin_ct_export_device / fhelin_ct_import_device as they always were"""
    import torch
    e = client
    cts, facts, _ = zoo
    for i in (0, 1):                                              # degree 1 and degree 2
        limbs, info, (hi, lo) = facts[i]
        assert info["deg"] == i + 1
        words = info["npoly"] * info["ell"] * e.N
        t = torch.empty(words * 8, dtype=torch.uint8, device="cuda")
        before = e.sync_count()
        cts[i].export_device(t.data_ptr(), words)
        assert e.sync_count() == before + 1
        assert t.cpu().numpy().tobytes() == frame_model(e, limbs, RAW)
        back = e.ct_import_device(t.data_ptr(), info["npoly"], info["ell"], info["deg"], hi, lo, info["slots"])
        _same(back, facts[i])


def test_level_plan_terminals_equal_the_single_exports(rot_eng):
    import torch
    e = rot_eng
    rng = np.random.default_rng(46)
    n = 1 << e.params.log_slots
    x, y = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    buf = torch.empty((2, 3 * e.n_q * e.N * 8), dtype=torch.uint8, device="cuda")

    def prog(many):
        a, b = e.encrypt(x), e.encrypt(y)                         # sources 0 and 1
        c = e.mult(a, b)
        outs = [c, e.mult(c, c)]
        if many:
            e.export_device_many(outs, buf.data_ptr(), buf.shape[1], buf.numel(), PACKED)
        else:
            for k, o in enumerate(outs):
                o.export_device(buf[k].data_ptr(), buf.shape[1] // 8)

    try:
        plans = []
        for many in (True, False):
            e.level_plan_begin("record")
            prog(many)
            plans.append(e.level_plan_end())
        assert plans[0] == plans[1] and len(plans[0]) == 2
        assert all(0 < p < e.n_q for p in plans[0]), plans        # the exports are terminals: the sources are lowered, and not to nothing
    finally:
        e.level_plan_begin("off")


@FORMATS
def test_range_check(fa, client, zoo, fmt):
    e = client
    cts, facts, frames = zoo
    limbs, info, _ = facts[2]                                     # 3 limbs
    assert info["ell"] == 3
    size = frame_formula(e, 2, 3, fmt)
    meta = np.array([[2, 3, info["deg"], info["slots"], *facts[2][2], size, fmt]] * 2, dtype=np.float64)
    bad = limbs.copy()
    bad[1, 2, 77] = e.q[2]                                        # one residue equal to its modulus: the field holds q_l (below 2^w)
    assert int(e.q[2]) < 1 << int(e.q[2]).bit_length()
    good_frame, bad_frame = frames[fmt][2], frame_model(e, bad, fmt)
    assert len(good_frame) == len(bad_frame) == size and size % 16 == 0
    buf = _device_bytes([good_frame, bad_frame])
    with pytest.raises(fa.FhelinError) as ei:
        e.import_device_many(buf.data_ptr(), size, meta, check=True)
    assert ei.value.code == ERR_ARG and "frame 1" in str(ei.value) and "range" in str(ei.value)
    # without the check the frames are taken as they are (documented: for frames this library wrote)
    back = e.import_device_many(buf.data_ptr(), size, meta)
    assert np.array_equal(back[0].export(), limbs) and np.array_equal(back[1].export(), bad)
    # the good frame alone passes the check, and the context is as usable as before
    _same(e.import_device_many(buf.data_ptr(), size, meta[:1], check=True)[0], facts[2])

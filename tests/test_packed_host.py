"""Packed ciphertext blobs on the host (include/fhelin.h "Packed formats"): the header reader fhelin_packed_info on blobs built
here from the documented layout - full, seeded, wrapped with an odd count - and its refusals.  The model of the bit stream is a
Python int: sum(v[j] << (j * w)) written little-endian, and (stream >> (j * w)) & (2 ** w - 1) back.  No device needed."""
import struct

import numpy as np
import pytest

ERR_ARG = 1


def pack_model(v, w):
    """N residues below 2^w -> the N w / 8 bytes of the packed vector"""
    stream = 0
    for j, x in enumerate(v):
        assert 0 <= int(x) < (1 << w)
        stream |= int(x) << (j * w)
    return stream.to_bytes(len(v) * w // 8, "little")


def unpack_model(b, w, n):
    stream = int.from_bytes(b, "little")
    return [(stream >> (j * w)) & ((1 << w) - 1) for j in range(n)]


def build_blob(log_n, moduli, stored, payload=None, deg=1, slots=None, scale=(2.0 ** 52, 0.0), nonce=None, seed=None, digest=0,
               positions=(), total=None, magic=b"FHELINCP", version=1, header=None, reserved=0, count=None):
    """a packed ciphertext blob from the documented layout; payload: residues [stored][ell][N] (default: j + limb)"""
    N, ell = 1 << log_n, len(moduli)
    slots = slots if slots is not None else N // 2
    cnt = len(positions) if count is None else count
    if nonce is None:
        nonce = 3 if stored == 1 else 0
    if seed is None:
        seed = bytes(range(32)) if stored == 1 else bytes(32)
    H = 112 + 8 * ell + 8 * ((len(positions) + 1) // 2)
    h = bytearray(H)
    h[0:8] = magic
    struct.pack_into("<II4i2dQ", h, 8, version, H if header is None else header, log_n, ell, deg, slots, scale[0], scale[1], nonce)
    h[56:88] = seed
    struct.pack_into("<Q4I", h, 88, digest, stored, cnt, (max(positions) + 1 if positions else 0) if total is None else total, reserved)
    struct.pack_into("<%dQ" % ell, h, 112, *moduli)
    struct.pack_into("<%dI" % len(positions), h, 112 + 8 * ell, *positions)
    body = b""
    for c in range(max(stored, 0)):
        for l, m in enumerate(moduli):
            w = int(m).bit_length()
            v = payload[c][l] if payload is not None else [(j + l) & ((1 << w) - 1) for j in range(N)]
            body += pack_model(v, w)
    return bytes(h) + body


def _code(fa, blob):
    with pytest.raises(fa.FhelinError) as ei:
        fa.packed_info(blob)
    return ei.value.code


MODULI = [(1 << 55) - 55, (1 << 52) - 47, (1 << 52) + 21, (1 << 60) - 93, (1 << 20) + 7]   # 55, 52, 53, 60 and 21 bits


def test_stream_model_round_trips_and_straddles():
    rng = np.random.default_rng(3)
    for w in (20, 33, 52, 59, 60):
        v = [int(x) for x in rng.integers(0, 1 << w, 64, dtype=np.uint64)]
        b = pack_model(v, w)
        assert len(b) == 8 * w and unpack_model(b, w, 64) == v
    # residue 1 of a 60-bit vector starts at bit 60: its low 4 bits end word 0, the other 56 begin word 1
    b = pack_model([0, (1 << 60) - 1] + [0] * 62, 60)
    assert struct.unpack_from("<2Q", b) == (0xF << 60, (1 << 56) - 1)


def test_packed_info_accepts_the_documented_layouts(fa):
    log_n, N = 12, 4096
    full = build_blob(log_n, MODULI[:3], stored=2, deg=1, slots=1024)
    assert len(full) == 112 + 8 * 3 + 2 * N * (55 + 52 + 53) // 8
    assert fa.packed_info(full) == dict(log_n=12, ell=3, deg=1, slots=1024, stored=2, count=0)
    three = build_blob(log_n, MODULI[:2], stored=3, deg=2)
    assert fa.packed_info(three) == dict(log_n=12, ell=2, deg=2, slots=2048, stored=3, count=0)
    seeded = build_blob(log_n, MODULI, stored=1)
    assert len(seeded) == 112 + 8 * 5 + N * (55 + 52 + 53 + 60 + 21) // 8
    assert fa.packed_info(seeded) == dict(log_n=12, ell=5, deg=1, slots=2048, stored=1, count=0)
    wrapped = build_blob(log_n, MODULI[:4], stored=1, positions=(0, 4, 9), total=12)   # odd count: 4 bytes of padding
    assert len(wrapped) == 112 + 8 * 4 + 16 + N * (55 + 52 + 53 + 60) // 8
    assert fa.packed_info(wrapped) == dict(log_n=12, ell=4, deg=1, slots=2048, stored=1, count=3)
    # the payload sits where the layout says: the first vector of the full blob, read back with the model
    v = unpack_model(full[112 + 24:112 + 24 + N * 55 // 8], 55, N)
    assert v[:5] == [0, 1, 2, 3, 4] and v[-1] == N - 1


def test_packed_info_refusals(fa):
    log_n = 12
    m3 = MODULI[:3]
    good = build_blob(log_n, m3, stored=2)
    assert fa.packed_info(good)["ell"] == 3
    bad = {
        "magic": build_blob(log_n, m3, stored=2, magic=b"FHELINCC"),
        "version": build_blob(log_n, m3, stored=2, version=2),
        "H inconsistent": build_blob(log_n, m3, stored=2, header=112 + 8 * 3 + 8),
        "H short": build_blob(log_n, m3, stored=2, header=104 + 8 * 3),
        "one word short": good[:-8],
        "one word long": good + bytes(8),
        "one byte short": good[:-1],
        "truncated header": good[:100],
        "stored 0": build_blob(log_n, m3, stored=0),
        "stored 4": build_blob(log_n, m3, stored=4),
        "count with stored 2": build_blob(log_n, m3, stored=2, positions=(0, 1), total=2, nonce=0, seed=bytes(32)),
        "count 129": build_blob(log_n, m3, stored=1, positions=tuple(range(129)), total=200),
        "total below count": build_blob(log_n, m3, stored=1, positions=(0, 1, 2), total=2),
        "total without count": build_blob(log_n, m3, stored=1, total=5),
        "positions unordered": build_blob(log_n, m3, stored=1, positions=(4, 2), total=8),
        "padding": build_blob(log_n, m3, stored=1, positions=(0, 1, 2, 3), total=8, count=3),
        "reserved word": build_blob(log_n, m3, stored=2, reserved=1),
        "modulus of 61 bits": build_blob(log_n, [m3[0], (1 << 60) + 33, m3[2]], stored=2),
        "modulus of 19 bits": build_blob(log_n, [m3[0], (1 << 19) - 1, m3[2]], stored=2),
        "ell 0": build_blob(log_n, [], stored=2),
        "log_n": build_blob(11, m3, stored=2),
        "deg": build_blob(log_n, m3, stored=2, deg=0),
        "deg 3 seeded": build_blob(log_n, m3, stored=1, deg=3),
        "slots": build_blob(log_n, m3, stored=2, slots=1000),
        "scale": build_blob(log_n, m3, stored=2, scale=(-1.0, 0.0)),
        "scale lo": build_blob(log_n, m3, stored=2, scale=(2.0 ** 52, 2.0)),
        "digest field": build_blob(log_n, m3, stored=2, digest=(1 << 61) - 1),
        "seed in a full blob": build_blob(log_n, m3, stored=2, seed=bytes([1]) + bytes(31)),
        "nonce in a full blob": build_blob(log_n, m3, stored=2, nonce=1),
    }
    for what, blob in bad.items():
        assert _code(fa, blob) == ERR_ARG, what


# ---- packed key sets ("FHELINEP") built from the documented layout

PRM_FIELDS = ("log_n", "n_q", "first_bits", "scale_bits", "n_p", "special_bits", "dnum", "log_slots", "hamming")


def build_set_packed(cfg, moduli, keys, halves, magic=b"FHELINEP", version=1, seed=None, reserved=0, halves_field=None, words_delta=0,
                     table_cut=0):
    """keys: list of (kind, digits, galois, max_ell); zero payloads of the packed size; words_delta is added to the last entry's words
    (the payload is sized to the changed field, so only the field disagrees with the widths)"""
    N, n_q, n_p = 1 << cfg["log_n"], cfg["n_q"], cfg["n_p"]
    nm = len(moduli)
    w = [int(m).bit_length() for m in moduli]
    table_end = 136 + 8 * nm + 48 * len(keys)
    data_offset = -(-table_end // 4096) * 4096
    head = magic + struct.pack("<II", version, len(keys)) + struct.pack("<9i", *[cfg[f] for f in PRM_FIELDS])
    head += struct.pack("<7i", *([0] * 7)) + struct.pack("<QQ", data_offset, 0)
    if seed is None:
        seed = bytes(range(1, 33)) if halves == 1 else bytes(32)
    head += seed + struct.pack("<II", halves if halves_field is None else halves_field, reserved)
    head += np.asarray(moduli, dtype="<u8").tobytes()
    at = data_offset
    for i, (kind, digits, g, max_ell) in enumerate(keys):
        bits = sum(w[:max_ell]) + (sum(w[n_q:n_q + n_p]) if kind != 0 else 0)
        words = (halves if kind == 0 else digits * halves) * bits * (N // 64)
        if i == len(keys) - 1:
            words += words_delta
        head += struct.pack("<IIQQQQII", kind, digits, g, at, words, 0, max_ell, 0)   # the digest of zeros is 0
        at += 8 * words
    if table_cut:
        return head[:-table_cut]
    return head + bytes(at - len(head))


def _toy(fa):
    cfg = dict(fa.PRESETS["toy"])
    e = fa.Engine("toy", device=-1)
    try:
        return cfg, [int(m) for m in e.moduli], e.alpha
    finally:
        e.close()


def _set_keys(cfg, alpha, cap):
    """the public key, an uncapped relinearisation key, one rotation key capped at `cap`"""
    n_q, N = cfg["n_q"], 1 << cfg["log_n"]
    return [(0, 0, 0, n_q), (1, -(-n_q // alpha), 0, n_q), (2, -(-cap // alpha), pow(5, 1, 2 * N), cap)]


def _set_code(fa, path):
    with pytest.raises(fa.FhelinError) as ei:
        fa.Engine.eval_keys_params(str(path))
    return ei.value.code


@pytest.mark.parametrize("halves", [2, 1])
def test_packed_key_set_header_is_read(fa, tmp_path, halves):
    cfg, moduli, alpha = _toy(fa)
    keys = _set_keys(cfg, alpha, 3)
    blob = build_set_packed(cfg, moduli, keys, halves)
    N, w = 1 << cfg["log_n"], [int(m).bit_length() for m in moduli]
    n_q = cfg["n_q"]
    per_row = lambda ls: sum(w[l] for l in ls) * N // 8
    want = (halves * per_row(range(n_q)) + keys[1][1] * halves * per_row(range(len(w))) +
            keys[2][1] * halves * per_row(list(range(3)) + list(range(n_q, len(w)))))
    assert len(blob) == 4096 + want                      # the table fits the first 4096 bytes
    p = tmp_path / "set.evp"
    p.write_bytes(blob)
    got, boot, n = fa.Engine.eval_keys_params(str(p))
    assert got == cfg and boot is None and n == 3


def test_packed_key_set_refusals(fa, tmp_path):
    cfg, moduli, alpha = _toy(fa)
    keys = _set_keys(cfg, alpha, 3)
    p = tmp_path / "bad.evp"
    m61 = list(moduli)
    m61[1] = (1 << 60) + 33
    bad = {
        "version": build_set_packed(cfg, moduli, keys, 2, version=2),
        "halves 0": build_set_packed(cfg, moduli, keys, 2, halves_field=0),
        "halves 3": build_set_packed(cfg, moduli, keys, 2, halves_field=3),
        "halves field says compact, sizes say full": build_set_packed(cfg, moduli, keys, 2, halves_field=1, seed=bytes(range(1, 33))),
        "reserved": build_set_packed(cfg, moduli, keys, 2, reserved=1),
        "seed in a full set": build_set_packed(cfg, moduli, keys, 2, seed=bytes(range(1, 33))),
        "a modulus of 61 bits": build_set_packed(cfg, m61, keys, 2),
        "truncated table": build_set_packed(cfg, moduli, keys, 2, table_cut=20),
        "truncated header": build_set_packed(cfg, moduli, keys, 2)[:130],
        "words one more": build_set_packed(cfg, moduli, keys, 2, words_delta=1),
        "words one fewer": build_set_packed(cfg, moduli, keys, 1, words_delta=-1),
        "one word short": build_set_packed(cfg, moduli, keys, 2)[:-8],
        "one word long": build_set_packed(cfg, moduli, keys, 2) + bytes(8),
        "cap 0": build_set_packed(cfg, moduli, keys[:2] + [(2, 1, 5, 0)], 2),
        "digits of another cap": build_set_packed(cfg, moduli, keys[:2] + [(2, 1, 5, 3)], 2),
        "unpacked words": None,
    }
    # the unpacked word count (version 2's) under the packed magic
    N, n_q, n_p = 1 << cfg["log_n"], cfg["n_q"], cfg["n_p"]
    w = [int(m).bit_length() for m in moduli]
    packed_words = keys[2][1] * 2 * (sum(w[:3]) + sum(w[n_q:])) * (N // 64)
    bad["unpacked words"] = build_set_packed(cfg, moduli, keys, 2, words_delta=keys[2][1] * 2 * (3 + n_p) * N - packed_words)
    for what, blob in bad.items():
        p.write_bytes(blob)
        assert _set_code(fa, p) == ERR_ARG, what
    p.write_bytes(build_set_packed(cfg, moduli, keys, 2))
    assert fa.Engine.eval_keys_params(str(p))[0] == cfg

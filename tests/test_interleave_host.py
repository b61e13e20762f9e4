"""Interleaved samples on the host (include/fhelin.h "Interleaved samples"): the argument and state checks of
fhelin_ctx_set_interleave on a host-only context, the getter, the stride word of an evaluation-key set's header (offset 88) on
files built here from the documented format, and the Python interleave / de-interleave helpers.  No device needed."""
import struct

import numpy as np
import pytest

ERR_ARG, ERR_STATE = 1, 4
PRM_FIELDS = ("log_n", "n_q", "first_bits", "scale_bits", "n_p", "special_bits", "dnum", "log_slots", "hamming")


def _host(fa, preset="toy", **kw):
    return fa.Engine(preset, device=-1, **kw)


def _code(fa, fn):
    with pytest.raises(fa.FhelinError) as ei:
        fn()
    return ei.value.code


def test_error_codes_are_the_headers(fa):
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fhelin.h")).read()
    assert int(re.search(r"#define FHELIN_ERR_ARG\s+(\d+)", h).group(1)) == ERR_ARG
    assert int(re.search(r"#define FHELIN_ERR_STATE\s+(\d+)", h).group(1)) == ERR_STATE


def test_default_is_one_and_getter_reads_back(fa):
    e = _host(fa, log_slots=10)
    try:
        assert e.interleave == 1
        e.set_interleave(2)
        assert e.interleave == 2
        e.set_interleave(1)          # nothing exists on the context yet: the stride may still change
        assert e.interleave == 1
    finally:
        e.close()
    e = _host(fa, interleave=2, log_slots=10)
    try:
        assert e.interleave == 2
    finally:
        e.close()


@pytest.mark.parametrize("stride", [3, 0, -2, 6])
def test_stride_must_be_a_power_of_two(fa, stride):
    e = _host(fa, log_slots=9)
    try:
        assert _code(fa, lambda: e.set_interleave(stride)) == ERR_ARG
        assert e.interleave == 1
    finally:
        e.close()


def test_physical_packing_must_fit_the_ring(fa):
    e = _host(fa)                    # toy: log_slots 11 at N = 2^12 is full packing already
    try:
        assert _code(fa, lambda: e.set_interleave(2)) == ERR_ARG
        assert e.interleave == 1
    finally:
        e.close()
    e = _host(fa, log_slots=9)       # 512 logical slots: 4 x 512 = N/2 fits, 8 x 512 does not
    try:
        assert _code(fa, lambda: e.set_interleave(8)) == ERR_ARG
        e.set_interleave(4)
        assert e.interleave == 4
    finally:
        e.close()
    with pytest.raises(fa.FhelinError) as ei:
        _host(fa, interleave=2)
    assert ei.value.code == ERR_ARG


def test_refused_once_a_plaintext_exists(fa):
    e = _host(fa, log_slots=10)
    try:
        pt = e.encode(np.arange(8.0))     # a handle only: nothing is encoded before an operation asks for it
        assert _code(fa, lambda: e.set_interleave(2)) == ERR_STATE
        assert e.interleave == 1
        pt.free()
    finally:
        e.close()


def _build_header(cfg, moduli, word88, magic=b"FHELINEK", boot=(0,) * 7):
    """an evaluation-key set without keys, from the format in include/fhelin.h; word88: the u64 at offset 88"""
    nm = len(moduli)
    table_end = (96 if magic == b"FHELINEK" else 128) + 8 * nm
    data_offset = -(-table_end // 4096) * 4096
    head = magic + struct.pack("<II", 1, 0) + struct.pack("<9i", *[cfg[f] for f in PRM_FIELDS])
    head += struct.pack("<7i", *boot) + struct.pack("<QQ", data_offset, word88)
    assert len(head) == 96 and struct.unpack_from("<Q", head, 88)[0] == word88
    if magic != b"FHELINEK":
        head += bytes(32)            # the compact form's key-set seed
    head += np.asarray(moduli, dtype=np.uint64).tobytes()
    return head + b"\0" * (data_offset - len(head))


@pytest.fixture(scope="module")
def toy10(fa):
    cfg = dict(fa.PRESETS["toy"], log_slots=10)
    e = fa.Engine(cfg, device=-1)
    try:
        return cfg, [int(m) for m in e.moduli]
    finally:
        e.close()


@pytest.mark.parametrize("magic", [b"FHELINEK", b"FHELINEC"])
@pytest.mark.parametrize("word88,stride", [(0, 1), (2, 2)])
def test_header_word_88_is_the_stride(fa, tmp_path, toy10, magic, word88, stride):
    cfg, moduli = toy10
    p = tmp_path / "set.evk"
    p.write_bytes(_build_header(cfg, moduli, word88, magic, boot=(3, 3, 1024, 28, 3, 47, 10)))
    assert fa.Engine.eval_keys_interleave(str(p)) == stride
    got, boot, n = fa.Engine.eval_keys_params(str(p))
    assert got == cfg and n == 0
    assert got["log_slots"] == 10 and boot["slots"] == 1024      # both stay logical


@pytest.mark.parametrize("word88", [1, 3, 4, 6, 1 << 40, 1 << 54, 1 << 63])
def test_header_word_88_refusals(fa, tmp_path, toy10, word88):
    """1 is written as 0; no power of two; 4 x 1024 slots exceed N/2 = 2048; 2^54 and 2^63 shifted left by log_slots = 10 wrap to 0
    in 64 bits, and so does their low half as a stride"""
    cfg, moduli = toy10
    p = tmp_path / "bad.evk"
    p.write_bytes(_build_header(cfg, moduli, word88))
    assert _code(fa, lambda: fa.Engine.eval_keys_interleave(str(p))) == ERR_ARG
    assert _code(fa, lambda: fa.Engine.eval_keys_params(str(p))) == ERR_ARG


@pytest.mark.parametrize("s", [1, 2, 4])
def test_python_helpers_are_inverse(fa, s):
    rng = np.random.default_rng(s)
    z = rng.normal(size=(s, 48))
    w = fa.interleave(z)
    assert w.shape == (48 * s,)
    for i in range(s):
        assert np.array_equal(w[i::s], z[i])                     # w[s k + i] = z_i[k]
    assert np.array_equal(fa.deinterleave(w, s), z)
    assert np.array_equal(fa.interleave(fa.deinterleave(w, s)), w)

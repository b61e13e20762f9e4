"""Device transport, the refusals (include/fhelin.h "Device transport"): every argument and every metadata row is checked on the
host before anything is allocated or launched, so a host-only context gives FHELIN_ERR_ARG with a message and leaves `outs` alone;
only frames that pass reach the device (FHELIN_ERR_NO_DEVICE here).  The wrapped-handle refusal needs a handle, and so a GPU: it is
the one test of this file marked gpu."""
import ctypes as C
import types

import numpy as np
import pytest

ERR_ARG, ERR_NO_DEVICE = 1, 2
RAW, PACKED = 0, 1
FAKE_BUFFER = 0x10000          # never dereferenced: every call here is refused (or stops at the missing device) first


@pytest.fixture(scope="module")
def host(fa):
    e = fa.Engine("toy", device=-1)
    yield e
    e.close()


def _payload(e, npoly, ell, fmt):
    if fmt == RAW:
        return npoly * ell * e.N * 8
    return npoly * sum(e.N * int(q).bit_length() // 8 for q in e.q[:ell])


def _row(e, npoly=2, ell=3, deg=1, slots=1024, fmt=PACKED, payload=None):
    """a metadata row; the payload size of the shape it names where it names one (a wrong shape is refused before its size is looked at)"""
    if payload is None:
        shaped = all(isinstance(v, int) for v in (npoly, ell)) and 1 <= ell <= e.n_q
        payload = _payload(e, npoly, ell, fmt) if shaped else 16
    return [npoly, ell, deg, slots, 2.0 ** 52, 0.0, payload, fmt]


def _import(e, rows, stride=1 << 20, buf=FAKE_BUFFER):
    """the C call itself: (status, message, outs)"""
    meta = np.array(rows, dtype=np.float64).reshape(-1, 8)
    outs = (C.c_void_p * max(1, len(meta)))()
    rc = e.lib.fhelin_ct_import_device_many(e.h, C.c_void_p(buf), stride, meta.ctypes.data_as(C.POINTER(C.c_double)), len(meta), 0, None, outs)
    return rc, e.lib.fhelin_last_error().decode(), list(outs)


def test_a_good_frame_set_reaches_the_device_check(host):
    rc, msg, outs = _import(host, [_row(host), _row(host, npoly=3, ell=host.n_q, deg=2, fmt=RAW)])
    assert rc == ERR_NO_DEVICE and outs == [None, None], msg


@pytest.mark.parametrize("what,change,stride,word", [
    ("stride not a multiple of 16", {}, (1 << 20) + 8, "multiple of 16"),
    ("stride below a payload", {}, 4096, "above stride_bytes"),
    ("format 2", {"fmt": 2}, 1 << 20, "format"),
    ("ell n_q + 1", {"ell": 7}, 1 << 20, "ell"),
    ("ell 0", {"ell": 0}, 1 << 20, "ell"),
    ("npoly 1", {"npoly": 1}, 1 << 20, "npoly"),
    ("npoly 4", {"npoly": 4}, 1 << 20, "npoly"),
    ("deg 3", {"deg": 3}, 1 << 20, "deg"),
    ("deg 0", {"deg": 0}, 1 << 20, "deg"),
    ("payload_bytes 8 more", {"payload": +8}, 1 << 20, "payload_bytes"),
    ("payload_bytes 8 fewer", {"payload": -8}, 1 << 20, "payload_bytes"),
    ("slots not a power of two", {"slots": 1000}, 1 << 20, "slots"),
    ("npoly 2.5", {"npoly": 2.5}, 1 << 20, "npoly"),
    ("ell NaN", {"ell": float("nan")}, 1 << 20, "ell"),
])
def test_import_refusals(host, what, change, stride, word):
    e = host
    assert e.n_q == 6
    kw = dict(change)
    if "payload" in kw:
        kw["payload"] = _payload(e, 2, 3, PACKED) + kw["payload"]
    if "fmt" in kw:                                                # the size of format 1, so that only the format is wrong
        kw["payload"] = _payload(e, 2, 3, PACKED)
    good = _row(e)
    for rows in ([_row(e, **kw)], [good, _row(e, **kw)]):          # alone, and behind a good frame: all or nothing
        rc, msg, outs = _import(e, rows, stride)
        assert rc == ERR_ARG, what
        assert word in msg, (what, msg)
        assert all(o is None for o in outs), what
    if len(change):
        assert "frame 1" in _import(e, [good, _row(e, **kw)], stride)[1]


def test_import_argument_refusals(host):
    e = host
    assert _import(e, [_row(e)], buf=FAKE_BUFFER + 8)[0] == ERR_ARG          # the buffer is not 16-byte aligned
    assert _import(e, [_row(e)], buf=0)[0] == ERR_ARG
    meta = np.array([_row(e)], dtype=np.float64)
    assert e.lib.fhelin_ct_import_device_many(e.h, C.c_void_p(FAKE_BUFFER), 1 << 20, meta.ctypes.data_as(C.POINTER(C.c_double)), 1, 0, None,
                                              None) == ERR_ARG
    assert e.lib.fhelin_ct_import_device_many(e.h, C.c_void_p(FAKE_BUFFER), 1 << 20, None, -1, 0, None, None) == ERR_ARG


def test_export_refusals_before_a_handle_is_looked_at(fa, host):
    e = host
    nothing = [types.SimpleNamespace(h=None)] * 2                  # two null handles: refused last of all
    cases = {
        "stride not a multiple of 16": ((1 << 20) + 4, 4 << 20, PACKED, "multiple of 16"),
        "stride 0": (0, 4 << 20, PACKED, "multiple of 16"),
        "cap_bytes below n strides": (1 << 20, (2 << 20) - 1, PACKED, "cap_bytes"),
        "format 2": (1 << 20, 2 << 20, 2, "format"),
        "format -1": (1 << 20, 2 << 20, -1, "format"),
        "null handles": (1 << 20, 2 << 20, RAW, "null ciphertext handle"),
    }
    for what, (stride, cap, fmt, word) in cases.items():
        with pytest.raises(fa.FhelinError) as ei:
            e.export_device_many(nothing, FAKE_BUFFER, stride, cap, fmt)
        assert ei.value.code == ERR_ARG and word in str(ei.value), (what, str(ei.value))
    with pytest.raises(fa.FhelinError) as ei:
        e.export_device_many(nothing, FAKE_BUFFER + 4, 1 << 20, 2 << 20, PACKED)
    assert ei.value.code == ERR_ARG and "aligned" in str(ei.value)
    with pytest.raises(fa.FhelinError) as ei:
        e.frame_bytes(nothing, 2)
    assert ei.value.code == ERR_ARG


def test_nothing_to_move_succeeds_and_does_nothing(host):
    e = host
    before = e.sync_count()
    assert e.frame_bytes([], PACKED) == ([], 0)
    assert e.export_device_many([], 0, 0, 0, PACKED).shape == (0, 8)
    assert e.export_device_many([], 0, 24, 0, 7).shape == (0, 8)   # nothing is looked at
    assert e.import_device_many(0, 0, np.zeros((0, 8))) == []
    assert e.sync_count() == before == 0


@pytest.mark.gpu
def test_a_wrapped_handle_is_refused(fa):
    import torch
    e = fa.Engine("toy13", seed=31, log_n=15, n_q=5, n_p=2, dnum=3, log_slots=14, hamming=64)   # the smallest ring of the wrapped layout
    try:
        e.keygen()
        rng = np.random.default_rng(6)
        S = 2
        ws = e.client_ingest_wrapped(cls=rng.uniform(-1, 1, 128), pos=rng.uniform(-1, 1, (S, 128)), E_w=rng.uniform(-0.1, 0.1, (32, S + 1)),
                                     E_b=rng.uniform(-0.1, 0.1, 32), F_w=rng.uniform(-0.1, 0.1, (32, S + 1)), F_b=rng.uniform(-0.1, 0.1, 32),
                                     emb=rng.uniform(-1, 1, (S, 128)))
        assert ws[0].wrapped_info()["count"] > 0
        plain = e.encrypt(rng.uniform(-1, 1, 16))
        stride = e.frame_bytes([plain], RAW)[1] + e.N * 8 * 2      # room for the wrapped handle's extra limb: only its kind is wrong
        buf = torch.full((2, stride), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for fmt in (RAW, PACKED):
            with pytest.raises(fa.FhelinError) as ei:
                e.export_device_many([plain, ws[0]], buf.data_ptr(), stride, 2 * stride, fmt)
            assert ei.value.code == ERR_ARG and "wrapped" in str(ei.value) and "handle 1" in str(ei.value)
            with pytest.raises(fa.FhelinError) as ei:
                e.frame_bytes([ws[0]], fmt)
            assert ei.value.code == ERR_ARG
        assert (buf.cpu().numpy() == 0xA5).all()                   # nothing was written, the good handle's frame included
    finally:
        e.close()

"""Wrapped inputs of interleaved samples on the host (include/fhelin.h "Interleaved samples"): the entry point exists, is bound, and
refuses on its arguments alone - before any device work - what it must.  No device needed."""
import ctypes as C

import numpy as np

ERR_ARG = 1


def test_entry_point_exists(fa):
    assert hasattr(fa.load_library(), "fhelin_client_ingest_wrapped_interleaved")
    assert hasattr(fa.Engine, "client_ingest_wrapped_interleaved")


def _call(e, n_samples, ptrs, S=3, outs=True):
    a = [np.zeros(128), np.zeros((S, 128)), np.zeros((32, S + 1)), np.zeros(32), np.zeros((32, S + 1)), np.zeros(32)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    o = (C.c_void_p * (64 + S + 1))()
    n_out = C.c_int32(-1)
    rc = e.lib.fhelin_client_ingest_wrapped_interleaved(e.h, n_samples, ptrs, None, None, 0, S, *[p(x) for x in a], S + 1, 0, None,
                                                        o if outs else None, C.byref(n_out), None)
    return rc, n_out.value, [h for h in o if h]


def test_refusals_without_a_device(fa):
    e = fa.Engine("toy", device=-1, log_slots=8, interleave=2)
    try:
        xs = [np.zeros((3, 128)), np.zeros((3, 128))]
        two = (C.c_void_p * 2)(*[x.ctypes.data for x in xs])
        assert _call(e, 2, two, outs=False)[0] == ERR_ARG                         # a null argument
        assert _call(e, 2, None)[0] == ERR_ARG                                    # neither embeddings nor tokens
        for n in (1, 3, 4):                                                       # one sample per lane
            assert _call(e, n, two) == (ERR_ARG, 0, []), n
        rc, n_out, left = _call(e, 2, two)                                        # the right count: refused for want of keys and a device
        assert rc != 0 and n_out == 0 and left == []
    finally:
        e.close()

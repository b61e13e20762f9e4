"""ctypes binding of include/fhelin.h (test / bench harness only; the product is the .so)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class FhelinError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fhelin error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [
        ("log_n", C.c_int32), ("n_q", C.c_int32), ("first_bits", C.c_int32), ("scale_bits", C.c_int32),
        ("n_p", C.c_int32), ("special_bits", C.c_int32), ("dnum", C.c_int32), ("log_slots", C.c_int32),
        ("hamming", C.c_int32), ("device", C.c_int32), ("seed", C.c_uint64),
    ]


# Parameter presets.  "reference" = literal values of reference src/FHEController.cpp:6-35 (N=2^15, depth 27
# -> 28 Q limbs, dnum 4 -> alpha 7, 7 special primes); "bench" = BASELINE.json synthetic config
# (N=2^16, 24 limbs, k=6); "deep" = config 5 (N=2^17, 30 limbs, k=8); "toy*" = small rings for fast tests.
PRESETS = {
    "bench": dict(log_n=16, n_q=24, first_bits=55, scale_bits=52, n_p=6, special_bits=60, dnum=4, log_slots=14, hamming=192),
    "reference": dict(log_n=15, n_q=28, first_bits=55, scale_bits=52, n_p=7, special_bits=60, dnum=4, log_slots=14, hamming=192),
    "deep": dict(log_n=17, n_q=30, first_bits=55, scale_bits=52, n_p=8, special_bits=60, dnum=4, log_slots=14, hamming=192),
    "toy": dict(log_n=12, n_q=6, first_bits=55, scale_bits=52, n_p=2, special_bits=60, dnum=3, log_slots=11, hamming=64),
    "boot12": dict(log_n=12, n_q=22, first_bits=55, scale_bits=52, n_p=6, special_bits=60, dnum=4, log_slots=10, hamming=64),
    "toy13": dict(log_n=13, n_q=7, first_bits=55, scale_bits=52, n_p=3, special_bits=60, dnum=3, log_slots=12, hamming=64),
}


def circuit_rotation_indices():
    """The rotation keys a client generates for the Linformer circuit: the +-2^i set the reference's composites rotate by
    (the shim's generate_rotation_keys extends main.cpp's list to it, quirk Q3), plus +-3*2^i, with which two steps of a
    rotate-and-sum tree run as one merged key switch (Evaluator::rotate_sum_batch), plus +-5s and +-7s for the tree units
    s in {1, 8, 128, 512, 1024}, with which three steps do."""
    r = set()
    for i in range(14):
        r.update((1 << i, -(1 << i)))
    for i in range(13):
        r.update((3 << i, -(3 << i)))
    for s in (1, 8, 128, 512, 1024):      # three tree steps as one merged key switch: the keys of s..7s (6s = 3*2s is above)
        r.update((5 * s, -5 * s, 7 * s, -7 * s))
    return sorted(r)


def library_path():
    # FHELIN_LIB: an alternative build of the same library (A/B measurements of kernel variants: tools/build_variant.sh)
    return os.environ.get("FHELIN_LIB") or os.path.join(_HERE, "libfhelin_amd.so")


def load_library():
    """Load libfhelin_amd.so; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise FhelinError(-1, f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp, i32, u64p, f32p = C.c_void_p, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    sigs = {
        "fhelin_last_error": (C.c_char_p, []),
        "fhelin_version": (C.c_char_p, []),
        "fhelin_ctx_create": (i32, [C.POINTER(Params), C.POINTER(vp)]),
        "fhelin_ctx_create_seeded": (i32, [C.POINTER(Params), vp, C.POINTER(vp)]),
        "fhelin_ctx_secret_seed": (i32, [vp, vp]),
        "fhelin_prng_block": (i32, [vp, C.c_uint64, C.c_uint64, vp]),
        "fhelin_ctx_destroy": (None, [vp]),
        "fhelin_ctx_info": (i32, [vp, C.POINTER(Params), C.POINTER(i32), C.POINTER(i32)]),
        "fhelin_ctx_moduli": (i32, [vp, u64p, i32]),
        "fhelin_ctx_roots": (i32, [vp, u64p, i32]),
        "fhelin_ctx_scaling_factors": (i32, [vp, C.POINTER(C.c_double), i32]),
        "fhelin_ctx_set_stream": (i32, [vp, vp]),
        "fhelin_ctx_set_lazy_rows": (i32, [vp, i32]),
        "fhelin_ct_force": (i32, [vp, C.POINTER(vp), i32]),
        "fhelin_level_plan_begin": (i32, [vp, i32]),
        "fhelin_level_plan_seek": (i32, [vp, i32]),
        "fhelin_level_plan_tell": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "fhelin_level_plan_end": (i32, [vp, C.POINTER(i32)]),
        "fhelin_level_plan_get": (i32, [vp, C.POINTER(i32), i32, C.POINTER(i32)]),
        "fhelin_level_plan_set": (i32, [vp, C.POINTER(i32), i32]),
        "fhelin_sync": (i32, [vp]),
        "fhelin_ctx_set_lane": (i32, [vp, i32]),
        "fhelin_ctx_lane_wait": (i32, [vp, i32]),
        "fhelin_ctx_lane_mark": (i32, [vp]),
        "fhelin_ctx_lane_wait_mark": (i32, [vp, i32]),
        "fhelin_ctx_lanes_fork": (i32, [vp]),
        "fhelin_ctx_lanes_join": (i32, [vp]),
        "fhelin_ctx_trim": (i32, [vp]),
        "fhelin_timer_start": (i32, [vp]),
        "fhelin_timer_stop": (i32, [vp, f32p]),
        "fhelin_dev_alloc": (i32, [vp, C.c_size_t, C.POINTER(vp)]),
        "fhelin_dev_free": (i32, [vp, vp]),
        "fhelin_dev_upload": (i32, [vp, vp, vp, C.c_size_t]),
        "fhelin_dev_download": (i32, [vp, vp, vp, C.c_size_t]),
        "fhelin_ntt": (i32, [vp, vp, i32, i32, i32, i32]),
        "fhelin_stats": (i32, [vp, u64p, i32, i32]),
        "fhelin_debug_pool_selftest": (i32, [C.c_uint64, i32, C.c_uint64, u64p, i32]),
        "fhelin_debug_pool_fill_stats": (i32, [vp, u64p, u64p]),
        "fhelin_debug_pool_fill_selftest": (i32, [C.c_uint64, i32, C.c_uint32, u64p, i32]),
        "fhelin_keygen": (i32, [vp]),
        "fhelin_gen_relin_key": (i32, [vp]),
        "fhelin_gen_rotation_keys": (i32, [vp, C.POINTER(i32), i32]),
        "fhelin_gen_conj_key": (i32, [vp]),
        "fhelin_secret_export": (i32, [vp, vp, C.c_size_t]),
        "fhelin_secret_import": (i32, [vp, vp, C.c_size_t]),
        "fhelin_key_export": (i32, [vp, i32, i32, vp, C.c_size_t]),
        "fhelin_key_import": (i32, [vp, i32, i32, vp, C.c_size_t]),
        "fhelin_ctx_set_key_caps": (i32, [vp, C.POINTER(i32), u64p, C.POINTER(i32), i32]),
        "fhelin_key_info": (i32, [vp, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "fhelin_key_usage_begin": (i32, [vp]),
        "fhelin_key_usage_end": (i32, [vp, C.POINTER(i32), u64p, C.POINTER(i32), i32, C.POINTER(i32)]),
        "fhelin_encode": (i32, [vp, C.POINTER(C.c_double), i32, i32, i32, C.POINTER(vp)]),
        "fhelin_pt_free": (None, [vp]),
        "fhelin_pt_export": (i32, [vp, vp, i32, C.c_double, C.c_double, vp, C.c_size_t]),
        "fhelin_rotate_each_sum": (i32, [vp, C.POINTER(vp), C.POINTER(i32), i32, C.POINTER(vp)]),
        "fhelin_raw_modraise": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_raw_phase": (i32, [vp, vp, C.POINTER(vp)]),
        "fhelin_encrypt": (i32, [vp, vp, C.POINTER(vp)]),
        "fhelin_encrypt_batch": (i32, [vp, C.POINTER(C.c_double), i32, i32, i32, i32, C.POINTER(vp)]),
        "fhelin_ctx_set_host_encode": (i32, [vp, i32]),
        "fhelin_client_ingest": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(vp), vp]),
        "fhelin_debug_sample": (i32, [vp, i32, i32, vp, C.c_size_t]),
        "fhelin_decrypt": (i32, [vp, vp, C.POINTER(C.c_double), i32]),
        "fhelin_ct_import": (i32, [vp, vp, i32, i32, i32, C.c_double, i32, C.POINTER(vp)]),
        "fhelin_ct_export": (i32, [vp, vp, vp, C.c_size_t]),
        "fhelin_ct_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(i32)]),
        "fhelin_ct_export_device": (i32, [vp, vp, vp, C.c_size_t]),
        "fhelin_ct_import_device": (i32, [vp, vp, i32, i32, i32, C.c_double, C.c_double, i32, C.POINTER(vp)]),
        "fhelin_ct_scale": (i32, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "fhelin_fc_unwrapRepeatedLarge_range": (i32, [vp, C.POINTER(vp), i32, i32, i32, i32, C.POINTER(vp)]),
        "fhelin_ct_clone": (i32, [vp, vp, C.POINTER(vp)]),
        "fhelin_ct_free": (None, [vp]),
        "fhelin_add": (i32, [vp, vp, vp, C.POINTER(vp)]),
        "fhelin_sub": (i32, [vp, vp, vp, C.POINTER(vp)]),
        "fhelin_negate": (i32, [vp, vp, C.POINTER(vp)]),
        "fhelin_add_plain": (i32, [vp, vp, vp, C.POINTER(vp)]),
        "fhelin_mult_plain": (i32, [vp, vp, vp, C.POINTER(vp)]),
        "fhelin_mult": (i32, [vp, vp, vp, C.POINTER(vp)]),
        "fhelin_rotate": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_rotate_many": (i32, [vp, vp, C.POINTER(i32), i32, C.POINTER(vp)]),
        "fhelin_rotate_each": (i32, [vp, C.POINTER(vp), C.POINTER(i32), i32, C.POINTER(vp)]),
        "fhelin_rotate_sum": (i32, [vp, C.POINTER(vp), i32, C.POINTER(i32), i32, C.POINTER(vp)]),
        "fhelin_hoisted_dot": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(i32), i32, i32, C.POINTER(vp)]),
        "fhelin_rescale": (i32, [vp, vp, C.POINTER(vp)]),
        "fhelin_rotate_batch": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_rescale_batch": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_mult_plain_batch": (i32, [vp, C.POINTER(vp), i32, vp, C.POINTER(vp)]),
        "fhelin_mult_batch": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_add_batch": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_mult_affine_batch": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, C.POINTER(i32), C.POINTER(C.c_double), C.POINTER(vp),
                                           C.POINTER(i32), C.POINTER(vp)]),
        "fhelin_level_reduce": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_raw_rescale": (i32, [vp, vp, C.POINTER(vp)]),
        "fhelin_raw_rotate": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_raw_mult_relin": (i32, [vp, vp, vp, C.POINTER(vp)]),
        "fhelin_fc_mult_const": (i32, [vp, vp, C.c_double, C.POINTER(vp)]),
        "fhelin_fc_mask": (i32, [vp, vp, i32, i32, i32, C.c_double, C.POINTER(vp)]),
        "fhelin_fc_rotsum": (i32, [vp, vp, i32, i32, C.POINTER(vp)]),
        "fhelin_fc_repeat": (i32, [vp, vp, i32, i32, C.POINTER(vp)]),
        "fhelin_fc_add_many": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_fc_matmul_pt": (i32, [vp, C.POINTER(vp), i32, vp, vp, i32, i32, C.POINTER(vp)]),
        "fhelin_fc_matmul_ct": (i32, [vp, C.POINTER(vp), i32, vp, i32, i32, C.POINTER(vp)]),
        "fhelin_fc_matmulRElarge": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp), i32, vp, C.c_double, C.POINTER(vp)]),
        "fhelin_fc_matmulCRlarge": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp), vp, C.POINTER(vp)]),
        "fhelin_fc_matmulScores": (i32, [vp, C.POINTER(vp), i32, vp, C.POINTER(vp)]),
        "fhelin_fc_wrapUpRepeated": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_fc_wrapUpExpanded": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_fc_unwrapExpanded": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_fc_unwrapScoresExpanded": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_fc_unwrap_512_in_4_128": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_fc_unwrapRepeatedLarge": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_fc_generate_containers": (i32, [vp, C.POINTER(vp), i32, vp, C.POINTER(vp), C.POINTER(i32)]),
        "fhelin_fc_wrap_containers": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_mult_real": (i32, [vp, vp, C.c_double, C.POINTER(vp)]),
        "fhelin_add_real": (i32, [vp, vp, C.c_double, C.POINTER(vp)]),
        "fhelin_mult_many": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_lincomb": (i32, [vp, C.POINTER(vp), C.POINTER(C.c_double), i32, C.c_double, C.POINTER(vp)]),
        "fhelin_eval_poly": (i32, [vp, vp, C.POINTER(C.c_double), i32, C.POINTER(vp)]),
        "fhelin_eval_chebyshev": (i32, [vp, vp, C.POINTER(C.c_double), i32, C.c_double, C.c_double, C.POINTER(vp)]),
        "fhelin_eval_chebyshev_batch": (i32, [vp, C.POINTER(vp), i32, C.POINTER(C.c_double), i32, C.c_double, C.c_double, C.POINTER(vp)]),
        "fhelin_bootstrap_setup": (i32, [vp, i32, i32, i32]),
        "fhelin_bootstrap": (i32, [vp, vp, C.POINTER(vp)]),
        "fhelin_bootstrap_config": (i32, [vp, i32, i32, i32, i32]),
        "fhelin_bootstrap_partial": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_bootstrap_drop": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_bootstrap_batch": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_bootstrap_iter": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_bootstrap_iter_batch": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_bootstrap_iter_drop": (i32, [vp, vp, i32, i32, C.POINTER(vp)]),
        "fhelin_bootstrap_pair": (i32, [vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]),
        "fhelin_bootstrap_paired_batch": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_bootstrap_pair_drop": (i32, [vp, vp, vp, i32, C.POINTER(vp), C.POINTER(vp)]),
        "fhelin_bootstrap_pair_partial": (i32, [vp, vp, vp, i32, C.POINTER(vp)]),
        "fhelin_ctx_set_bootstrap_pairing": (i32, [vp, i32]),
        "fhelin_ctx_bootstrap_pairing": (i32, [vp, C.POINTER(i32)]),
        "fhelin_ctx_set_bootstrap_lt": (i32, [vp, i32, i32]),
        "fhelin_ctx_bootstrap_lt": (i32, [vp, C.POINTER(i32), C.POINTER(i32)]),
        "fhelin_ctx_set_bootstrap_sparse_secret": (i32, [vp, i32]),
        "fhelin_ctx_bootstrap_sparse_secret": (i32, [vp, C.POINTER(i32)]),
        "fhelin_debug_boot_sparse_secret": (i32, [vp, C.c_void_p, C.c_size_t]),
        "fhelin_debug_cheb_depth": (i32, [i32, C.POINTER(i32)]),
        "fhelin_debug_pair_pack": (i32, [vp, C.POINTER(vp), C.POINTER(vp), u64p, u64p, i32, C.POINTER(vp)]),
        "fhelin_debug_pair_split": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(vp)]),
        "fhelin_bootstrap_describe": (i32, [vp, C.POINTER(i32), i32, C.POINTER(i32)]),
        "fhelin_bootstrap_diag": (i32, [vp, i32, i32, i32, C.POINTER(vp)]),
        "fhelin_bootstrap_cheb": (i32, [vp, C.POINTER(C.c_double), i32, C.POINTER(i32)]),
        "fhelin_fcb_matmulScores": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_fcb_matmul_ct": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, i32, i32, C.POINTER(vp)]),
        "fhelin_fcb_wrapUpRepeated": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_fcb_wrapUpExpanded": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_fcb_unwrapExpanded": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_fcb_unwrapRepeatedLarge": (i32, [vp, C.POINTER(vp), i32, i32, i32, C.POINTER(vp)]),
        "fhelin_fcb_generate_containers": (i32, [vp, C.POINTER(vp), i32, i32, vp, C.POINTER(vp), C.POINTER(i32)]),
        "fhelin_fc_rotsum_batch": (i32, [vp, C.POINTER(vp), i32, i32, i32, i32, C.POINTER(vp)]),
        "fhelin_add_plain_batch": (i32, [vp, C.POINTER(vp), i32, vp, C.POINTER(vp)]),
        "fhelin_eval_poly_batch": (i32, [vp, C.POINTER(vp), i32, C.POINTER(C.c_double), i32, C.POINTER(vp)]),
        "fhelin_mult_many_batch": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_evalkeys_save": (i32, [vp, C.c_char_p]),
        "fhelin_evalkeys_params": (i32, [C.c_char_p, C.POINTER(Params)]),
        "fhelin_evalkeys_info": (i32, [C.c_char_p, C.POINTER(i32), C.POINTER(i32)]),
        "fhelin_evalkeys_load": (i32, [vp, C.c_char_p]),
        "fhelin_evalkeys_save_compact": (i32, [vp, C.c_char_p]),
        "fhelin_evalkeys_save_packed": (i32, [vp, C.c_char_p, i32]),
        "fhelin_ctx_set_seeded_keys": (i32, [vp, i32]),
        "fhelin_ctx_key_set_seed": (i32, [vp, vp]),
        "fhelin_debug_key_digest": (i32, [vp, vp, i32, i32, C.POINTER(C.c_uint64), C.POINTER(i32)]),
        "fhelin_ctx_set_seeded_encryption": (i32, [vp, i32]),
        "fhelin_ct_compact_bytes": (i32, [vp, C.POINTER(C.c_size_t)]),
        "fhelin_ct_export_compact": (i32, [vp, vp, vp, C.c_size_t]),
        "fhelin_compact_info": (i32, [vp, C.c_size_t, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "fhelin_ct_import_compact": (i32, [vp, C.POINTER(vp), C.POINTER(C.c_size_t), i32, C.POINTER(vp)]),
        "fhelin_ct_packed_bytes": (i32, [vp, vp, i32, C.POINTER(C.c_size_t)]),
        "fhelin_ct_export_packed": (i32, [vp, vp, i32, vp, C.c_size_t]),
        "fhelin_packed_info": (i32, [vp, C.c_size_t] + [C.POINTER(i32)] * 6),
        "fhelin_ct_import_packed": (i32, [vp, C.POINTER(vp), C.POINTER(C.c_size_t), i32, C.POINTER(vp)]),
        "fhelin_debug_pack": (i32, [vp, vp, vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "fhelin_debug_unpack": (i32, [vp, vp, C.c_size_t, vp, i32, vp]),
        "fhelin_debug_pack_rate": (i32, [vp, vp, i32, i32, f32p]),
        "fhelin_debug_seeded_expand": (i32, [vp, vp, C.c_uint64, i32, i32, i32, vp, f32p]),
        "fhelin_ct_frame_bytes": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "fhelin_ct_export_device_many": (i32, [vp, C.POINTER(vp), i32, i32, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), vp]),
        "fhelin_ct_import_device_many": (i32, [vp, vp, C.c_size_t, C.POINTER(C.c_double), i32, i32, vp, C.POINTER(vp)]),
        "fhelin_debug_sync_count": (i32, [vp, u64p]),
        "fhelin_debug_ct_addr": (i32, [vp, u64p, u64p]),
        "fhelin_client_ingest_wrapped": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, C.POINTER(vp),
                                               C.POINTER(i32), vp]),
        "fhelin_client_ingest_wrapped_interleaved": (i32, [vp, i32, C.POINTER(vp), C.POINTER(vp), vp, i32, i32, vp, vp, vp, vp, vp, vp, i32,
                                                           i32, vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp)]),
        "fhelin_wrapped_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), vp, i32]),
        "fhelin_unwrap_inputs": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_sanitize": (i32, [vp, C.POINTER(vp), i32, vp, i32, i32, C.POINTER(vp)]),
        "fhelin_debug_flood": (i32, [vp, vp, C.c_uint64, i32, i32, vp, C.c_size_t]),
        "fhelin_decrypt_flooded": (i32, [vp, vp, i32, C.POINTER(C.c_double), i32]),
        "fhelin_debug_sampler_peek": (i32, [vp, i32, vp, u64p]),
        "fhelin_debug_pt_from_residues": (i32, [vp, vp, i32, C.POINTER(vp)]),
        "fhelin_debug_pt_from_residues_full": (i32, [vp, vp, C.c_double, C.c_double, C.POINTER(vp)]),
        "fhelin_lt_create": (i32, [vp, C.POINTER(C.c_double), C.POINTER(i32), i32, i32, i32, C.POINTER(vp)]),
        "fhelin_lt_create_pts": (i32, [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), i32, i32, C.POINTER(vp)]),
        "fhelin_lt_info": (i32, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "fhelin_lt_rotations": (i32, [vp, C.POINTER(i32), i32, C.POINTER(i32)]),
        "fhelin_lt_apply": (i32, [vp, vp, C.POINTER(vp), i32, i32, C.POINTER(vp)]),
        "fhelin_lt_encoding_bytes": (i32, [vp, C.POINTER(C.c_uint64)]),
        "fhelin_lt_free": (None, [vp]),
        "fhelin_debug_dot_plain": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_debug_dot_groups": (i32, [vp, C.POINTER(vp), i32, i32, C.POINTER(vp), i32, C.POINTER(vp)]),
        "fhelin_debug_dot_cyclic": (i32, [vp, C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(vp)]),
        "fhelin_debug_dot_window": (i32, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32]),
        "fhelin_debug_rotate_many_batch": (i32, [vp, C.POINTER(vp), i32, C.POINTER(i32), i32, C.POINTER(vp)]),
        "fhelin_debug_ks_accp": (i32, [vp, vp, i32, i32, C.POINTER(i32), i32, vp]),
        "fhelin_debug_ks_accq": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
        "fhelin_ctx_set_interleave": (i32, [vp, i32]),
        "fhelin_ctx_interleave": (i32, [vp, C.POINTER(i32)]),
        "fhelin_evalkeys_interleave": (i32, [C.c_char_p, C.POINTER(i32)]),
        "fhelin_encrypt_interleaved_batch": (i32, [vp, C.POINTER(C.c_double), i32, i32, i32, i32, C.POINTER(vp)]),
        "fhelin_decrypt_interleaved": (i32, [vp, vp, i32, C.POINTER(C.c_double), i32]),
        "fhelin_decrypt_batch": (i32, [vp, C.POINTER(vp), i32, i32, i32, C.POINTER(i32), i32, C.POINTER(C.c_double), i32]),
        "fhelin_ctx_set_device_decode": (i32, [vp, i32]),
        "fhelin_client_ingest_interleaved": (i32, [vp, i32, C.POINTER(vp), C.POINTER(vp), vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32,
                                                   C.POINTER(vp), C.POINTER(vp)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def compact_info(blob):
    """header of a compact ciphertext (include/fhelin.h "Compact ciphertexts"), validated against itself and its size:
    dict(log_n, ell, deg, slots); host-only"""
    lib = load_library()
    b = bytes(blob)
    v = [C.c_int32() for _ in range(4)]
    rc = lib.fhelin_compact_info(C.c_char_p(b), len(b), *[C.byref(x) for x in v])
    if rc != 0:
        raise FhelinError(rc, lib.fhelin_last_error().decode())
    return dict(zip(("log_n", "ell", "deg", "slots"), (x.value for x in v)))


def cheb_depth(degree):
    """the levels the bootstrap's depth counts for a cosine fit of this degree (fhelin_debug_cheb_depth; host only)"""
    lib = load_library()
    out = C.c_int32()
    rc = lib.fhelin_debug_cheb_depth(int(degree), C.byref(out))
    if rc != 0:
        raise FhelinError(rc, lib.fhelin_last_error().decode())
    return out.value


def packed_info(blob):
    """header of a packed ciphertext blob (include/fhelin.h "Packed formats"), validated against itself and the exact size its own
    moduli give: dict(log_n, ell, deg, slots, stored, count); host-only"""
    lib = load_library()
    b = bytes(blob)
    v = [C.c_int32() for _ in range(6)]
    rc = lib.fhelin_packed_info(C.c_char_p(b), len(b), *[C.byref(x) for x in v])
    if rc != 0:
        raise FhelinError(rc, lib.fhelin_last_error().decode())
    return dict(zip(("log_n", "ell", "deg", "slots", "stored", "count"), (x.value for x in v)))


def interleave(vectors):
    """`stride` sample vectors [stride][n] -> the physical slot vector [n * stride] of an interleaved ciphertext (include/fhelin.h
    "Interleaved samples"): slot stride * k + i = vectors[i][k]"""
    v = np.asarray(vectors)
    assert v.ndim == 2
    return np.ascontiguousarray(v.T).reshape(-1)


def deinterleave(physical, stride):
    """the inverse of interleave: a physical slot vector [n * stride] -> [stride][n]"""
    w = np.asarray(physical)
    assert w.ndim == 1 and w.size % stride == 0
    return np.ascontiguousarray(w.reshape(-1, stride).T)


def _np_u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(C.c_void_p)


def caps_from_usage(table, n_q, margin=0):
    """A usage table (Engine.key_usage: (kind, galois, max_ell) per key that was used) as the cap table Engine.set_key_caps takes:
    every key capped at the most limbs the recorded pass switched it at (+ margin, at most n_q).  Keys the pass never used have no
    entry and stay uncapped.  The caps hold for the recorded program under the recorded level plan only: a pass that goes higher is
    refused with FHELIN_ERR_KEY."""
    return [(int(k), int(g), min(int(n_q), int(m) + int(margin))) for k, g, m in table]


class _KeyUsage:
    def __init__(self, eng):
        self.eng = eng
        self.table = None

    def __enter__(self):
        self.eng._ck(self.eng.lib.fhelin_key_usage_begin(self.eng.h))
        return self

    def __exit__(self, exc_type, exc, tb):
        n = C.c_int32(0)
        rc = self.eng.lib.fhelin_key_usage_end(self.eng.h, None, None, None, 0, C.byref(n))
        if exc_type is not None:
            return False        # the block's own error is the one to report; the recording is over either way
        self.eng._ck(rc)
        m = max(1, n.value)
        kind, gal, cap = (C.c_int32 * m)(), (C.c_uint64 * m)(), (C.c_int32 * m)()
        # the recorder has stopped; its table stays readable until the next begin
        self.eng._ck(self.eng.lib.fhelin_key_usage_end(self.eng.h, kind, gal, cap, n.value, C.byref(n)))
        self.table = [(kind[i], gal[i], cap[i]) for i in range(n.value)]
        return False


class DevBuf:
    """A raw device allocation owned by an Engine."""

    def __init__(self, eng, nbytes):
        self.eng, self.nbytes = eng, int(nbytes)
        p = C.c_void_p()
        eng._ck(eng.lib.fhelin_dev_alloc(eng.h, self.nbytes, C.byref(p)))
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.eng._ck(self.eng.lib.fhelin_dev_upload(self.eng.h, self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return self

    def download(self, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.eng._ck(self.eng.lib.fhelin_dev_download(self.eng.h, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.eng._ck(self.eng.lib.fhelin_dev_free(self.eng.h, self.ptr))
            self.ptr = None


class Engine:
    """One fhelin context (one GPU, one stream)."""

    def __init__(self, preset="bench", device=0, seed=0, seed_bytes=None, interleave=1, **overrides):
        """seed=0 (default): keys from 256 bits of OS entropy.  seed != 0: deterministic TEST seed.  seed_bytes: an explicit
        32-byte secret seed (re-creating a client's keys).  interleave: the slot stride (include/fhelin.h "Interleaved samples"): that
        many samples per ciphertext; 1 (default) leaves the context as it is (set_interleave(1) sets it explicitly)."""
        self.lib = load_library()
        cfg = dict(PRESETS[preset]) if isinstance(preset, str) else dict(preset)
        cfg.update(overrides)
        self.params = Params(device=device, seed=seed, **cfg)
        h = C.c_void_p()
        if seed_bytes is not None:
            assert len(seed_bytes) == 32
            sb = (C.c_uint8 * 32)(*bytes(seed_bytes))
            rc = self.lib.fhelin_ctx_create_seeded(C.byref(self.params), sb, C.byref(h))
        else:
            rc = self.lib.fhelin_ctx_create(C.byref(self.params), C.byref(h))
        if rc != 0:
            raise FhelinError(rc, self.lib.fhelin_last_error().decode())
        self.h = h
        if self.params.n_p < 0:      # derived by the library (OpenFHE's sizeP rule): read the resolved parameters back
            rc = self.lib.fhelin_ctx_info(self.h, C.byref(self.params), None, None)
            if rc != 0:
                raise FhelinError(rc, self.lib.fhelin_last_error().decode())
        self.log_n, self.N = self.params.log_n, 1 << self.params.log_n
        self.n_q, self.n_p = self.params.n_q, self.params.n_p
        nl = self.n_q + self.n_p
        m = np.zeros(nl, dtype=np.uint64)
        self._ck(self.lib.fhelin_ctx_moduli(self.h, m.ctypes.data_as(C.POINTER(C.c_uint64)), nl))
        r = np.zeros(nl, dtype=np.uint64)
        self._ck(self.lib.fhelin_ctx_roots(self.h, r.ctypes.data_as(C.POINTER(C.c_uint64)), nl))
        self.moduli, self.roots = m, r
        self.q, self.p = m[: self.n_q], m[self.n_q:]
        self.psi_q, self.psi_p = r[: self.n_q], r[self.n_q:]
        sf = np.zeros(self.n_q, dtype=np.float64)
        self._ck(self.lib.fhelin_ctx_scaling_factors(self.h, sf.ctypes.data_as(C.POINTER(C.c_double)), self.n_q))
        self.scaling_factors = sf
        a, d = C.c_int32(), C.c_int32()
        self._ck(self.lib.fhelin_ctx_info(self.h, None, C.byref(a), C.byref(d)))
        self.alpha, self.has_device = a.value, bool(d.value)
        self.lazy_heavy = os.environ.get("FHELIN_LAZY_HEAVY", "1") != "0"
        self.lazy_rows_on = os.environ.get("FHELIN_LAZY_ROWS", "1") != "0"   # the library reads the same knob (capi.cpp)
        if interleave != 1:
            try:
                self.set_interleave(interleave)
            except Exception:
                self.close()
                raise

    def _ck(self, rc):
        if rc != 0:
            raise FhelinError(rc, self.lib.fhelin_last_error().decode())

    # ---- interleaved samples (include/fhelin.h "Interleaved samples")
    def set_interleave(self, stride):
        """the slot stride: `stride` samples per ciphertext; before the first key, plaintext, ciphertext or bootstrap set-up"""
        self._ck(self.lib.fhelin_ctx_set_interleave(self.h, int(stride)))

    @property
    def interleave(self):
        s = C.c_int32()
        self._ck(self.lib.fhelin_ctx_interleave(self.h, C.byref(s)))
        return s.value

    @staticmethod
    def eval_keys_interleave(path):
        """the stride a key set was written at; host-only"""
        lib = load_library()
        s = C.c_int32()
        rc = lib.fhelin_evalkeys_interleave(os.fsencode(path), C.byref(s))
        if rc != 0:
            raise FhelinError(rc, lib.fhelin_last_error().decode())
        return s.value

    def encrypt_interleaved_batch(self, rows, level=0, slots=0):
        """rows [n_vec][stride][n_per] -> n_vec fresh ciphertexts, sample i of a row in the physical slots = i mod stride"""
        a = np.ascontiguousarray(rows, dtype=np.float64)
        assert a.ndim == 3 and a.shape[1] == self.interleave
        outs = self._outs(a.shape[0])
        self._ck(self.lib.fhelin_encrypt_interleaved_batch(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0], a.shape[2], level,
                                                           slots, outs))
        return self._cts(outs, a.shape[0])

    def decrypt_interleaved(self, ct, slots=0, flood_bits=0):
        """every sample of a ciphertext: [stride][slots]"""
        n = slots or ct.slots or (1 << self.params.log_slots)
        out = np.empty((self.interleave, n), dtype=np.float64)
        self._ck(self.lib.fhelin_decrypt_interleaved(self.h, ct.h, int(flood_bits), out.ctypes.data_as(C.POINTER(C.c_double)), n))
        return out

    def client_ingest_interleaved(self, cls, pos, E_w, E_b, F_w, F_b, embs=None, tokens=None, table=None, level=0, want_proj=False):
        """client_ingest for `stride` samples of one length that share every ciphertext: embs (or tokens) is the list of the samples'
        embeddings (token ids).  Returns the group's {"inputs_E", "inputs_F", "inputs"} (+ per-sample lists x_in, proj if want_proj)"""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        cls, pos, E_w, E_b, F_w, F_b = f(cls), f(pos), f(E_w), f(E_b), f(F_w), f(F_b)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        if embs is not None:
            xs = [f(e) for e in embs]
            S, tab, vocab = xs[0].shape[0], None, 0
            if any(x.shape != (S, 128) for x in xs):
                raise FhelinError(1, "client_ingest_interleaved: the samples of a group have one length, rows of 128")
        else:
            xs = [np.ascontiguousarray(t, dtype=np.int32) for t in tokens]
            tab = f(table)
            S, vocab = xs[0].shape[0], tab.shape[0]
            if any(x.shape != (S,) for x in xs):
                raise FhelinError(1, "client_ingest_interleaved: the samples of a group have one length")
        if pos.shape[0] < S or pos.shape[1] != 128 or E_w.shape != F_w.shape or E_w.shape[0] != 32 or E_w.shape[1] < S + 1 or cls.size != 128 \
                or E_b.size != 32 or F_b.size != 32:
            raise FhelinError(1, "client_ingest_interleaved: pos needs >= S rows of 128, E_w / F_w [32][>= S + 1], E_b / F_b [32], cls [128]")
        ns = len(xs)
        ptrs = (C.c_void_p * ns)(*[x.ctypes.data for x in xs])
        n = 64 + S + 1
        outs = self._outs(n)
        proj = [np.empty((S + 1 + 64, 128)) for _ in range(ns)] if want_proj else None
        pp = (C.c_void_p * ns)(*[a.ctypes.data for a in proj]) if want_proj else None
        self._ck(self.lib.fhelin_client_ingest_interleaved(self.h, ns, ptrs if embs is not None else None, ptrs if embs is None else None,
                                                           p(tab), vocab, S, p(cls), p(pos), p(E_w), p(E_b), p(F_w), p(F_b), E_w.shape[1],
                                                           level, outs, pp))
        cts = self._cts(outs, n)
        res = {"inputs_E": cts[:32], "inputs_F": cts[32:64], "inputs": cts[64:]}
        if want_proj:
            res["x_in"], res["proj"] = [a[:S + 1] for a in proj], [a[S + 1:] for a in proj]
        return res

    def client_ingest_wrapped_interleaved(self, cls, pos, E_w, E_b, F_w, F_b, embs=None, tokens=None, table=None, level=0, targets=None,
                                          want_proj=False):
        """client_ingest_wrapped for `stride` samples of one length: the group's wrapped handles, the same inputs of every sample in one
        ciphertext (a group costs the bytes of one sample); embs (or tokens) is the list of the samples' embeddings (token ids),
        targets [64 + S + 1] (optional) is shared.  want_proj: (handles, [x_in per sample], [proj per sample])"""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        cls, pos, E_w, E_b, F_w, F_b = f(cls), f(pos), f(E_w), f(E_b), f(F_w), f(F_b)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        if embs is not None:
            xs = [f(e) if e is not None else None for e in embs]
            tab, vocab = None, 0
            shape = lambda S: (S, 128)
        else:
            xs = [np.ascontiguousarray(t, dtype=np.int32) if t is not None else None for t in tokens]
            tab = f(table)
            vocab = tab.shape[0]
            shape = lambda S: (S,)
        first = next((x for x in xs if x is not None), None)
        S = first.shape[0] if first is not None else 1
        if any(x is not None and x.shape != shape(S) for x in xs):
            raise FhelinError(1, "client_ingest_wrapped_interleaved: the samples of a group have one length" + (", rows of 128" if embs is not None else ""))
        if pos.shape[0] < S or pos.shape[1] != 128 or E_w.shape != F_w.shape or E_w.shape[0] != 32 or E_w.shape[1] < S + 1 or cls.size != 128 \
                or E_b.size != 32 or F_b.size != 32:
            raise FhelinError(1, "client_ingest_wrapped_interleaved: pos needs >= S rows of 128, E_w / F_w [32][>= S + 1], E_b / F_b [32], cls [128]")
        ns = len(xs)
        ptrs = (C.c_void_p * max(ns, 1))(*[x.ctypes.data if x is not None else None for x in xs])
        n = 64 + S + 1
        tg = None
        if targets is not None:
            tg = np.ascontiguousarray(targets, dtype=np.int32)
            if tg.size != n:
                raise FhelinError(1, "client_ingest_wrapped_interleaved: one target per input")
        outs = self._outs(n)
        n_out = C.c_int32()
        proj = [np.empty((S + 1 + 64, 128)) for _ in range(ns)] if want_proj else None
        pp = (C.c_void_p * max(ns, 1))(*[a.ctypes.data for a in proj]) if want_proj else None
        self._ck(self.lib.fhelin_client_ingest_wrapped_interleaved(self.h, ns, ptrs if embs is not None else None,
                                                                   ptrs if embs is None else None, p(tab), vocab, S, p(cls), p(pos), p(E_w),
                                                                   p(E_b), p(F_w), p(F_b), E_w.shape[1], level, p(tg), outs,
                                                                   C.byref(n_out), pp))
        cts = self._cts(outs, n_out.value)
        return (cts, [a[:S + 1] for a in proj], [a[S + 1:] for a in proj]) if want_proj else cts

    def set_lazy_rows(self, on):
        """deferred evaluation of the rows of matmul_pt / unwrapExpanded (default on)"""
        self._ck(self.lib.fhelin_ctx_set_lazy_rows(self.h, 1 if on else 0))
        self.lazy_rows_on = bool(on)

    # level plan (include/fhelin.h fhelin_level_plan_*): record one pass of a straight-line driver, apply to later ones
    def force(self, cts):
        """evaluate exactly the deferred rows among `cts` now, one batched call per producing call"""
        cts = list(cts)
        if cts:
            self._ck(self.lib.fhelin_ct_force(self.h, self._harr(cts), len(cts)))

    def level_plan_begin(self, mode, first_source=0):
        """mode: "record", "apply" or "off"; the pass starts at the program's first source unless first_source says otherwise
        (apply only: a server pass that starts after the client's encryptions)"""
        self._ck(self.lib.fhelin_level_plan_begin(self.h, {"off": 0, "record": 1, "apply": 2}[mode]))
        if first_source:
            self._ck(self.lib.fhelin_level_plan_seek(self.h, int(first_source)))

    def level_plan_tell(self):
        """(mode, index of the next source call): mode "off" / "record" / "apply" """
        m, k = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.fhelin_level_plan_tell(self.h, C.byref(m), C.byref(k)))
        return ("off", "record", "apply")[m.value], k.value

    def level_plan_seek(self, source):
        self._ck(self.lib.fhelin_level_plan_seek(self.h, int(source)))

    def level_plan_end(self):
        """ends the pass (a recording pass derives the plan); returns the plan: limbs per source, -1 = as asked"""
        n = C.c_int32(0)
        self._ck(self.lib.fhelin_level_plan_end(self.h, C.byref(n)))
        return self.level_plan()

    def level_plan(self):
        n = C.c_int32(0)
        self._ck(self.lib.fhelin_level_plan_get(self.h, None, 0, C.byref(n)))
        buf = (C.c_int32 * max(1, n.value))()
        self._ck(self.lib.fhelin_level_plan_get(self.h, buf, n.value, C.byref(n)))
        return list(buf[:n.value])

    def set_level_plan(self, target):
        arr = (C.c_int32 * len(target))(*[int(t) for t in target])
        self._ck(self.lib.fhelin_level_plan_set(self.h, arr, len(target)))

    def secret_seed(self):
        out = (C.c_uint8 * 32)()
        self._ck(self.lib.fhelin_ctx_secret_seed(self.h, out))
        return bytes(out)

    def close(self):
        if getattr(self, "h", None):
            self.lib.fhelin_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- raw buffers / kernels
    def buf(self, nbytes):
        return DevBuf(self, nbytes)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        return DevBuf(self, arr.nbytes).upload(arr)

    def sync(self):
        self._ck(self.lib.fhelin_sync(self.h))

    def set_lane(self, k):
        """subsequent calls launch on lane k's stream (0 = the main stream) and allocate from its arena"""
        self._ck(self.lib.fhelin_ctx_set_lane(self.h, int(k)))

    def lane_wait(self, from_lane):
        """the current lane's stream waits for everything issued under from_lane so far"""
        self._ck(self.lib.fhelin_ctx_lane_wait(self.h, int(from_lane)))

    def lane_mark(self):
        self._ck(self.lib.fhelin_ctx_lane_mark(self.h))

    def lane_wait_mark(self, from_lane):
        self._ck(self.lib.fhelin_ctx_lane_wait_mark(self.h, int(from_lane)))

    def lanes_fork(self):
        self._ck(self.lib.fhelin_ctx_lanes_fork(self.h))

    def lanes_join(self):
        self._ck(self.lib.fhelin_ctx_lanes_join(self.h))

    def trim(self):
        """release the device memory the caching pool holds but does not use"""
        self._ck(self.lib.fhelin_ctx_trim(self.h))

    def timer_start(self):
        self._ck(self.lib.fhelin_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._ck(self.lib.fhelin_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def ntt(self, buf, nvec, limb_first=0, limb_count=None, inverse=False):
        if limb_count is None:
            limb_count = self.n_q
        self._ck(self.lib.fhelin_ntt(self.h, buf.ptr, nvec, limb_first, limb_count, 1 if inverse else 0))

    def stats(self, reset=False):
        out = np.zeros(16, dtype=np.uint64)
        self._ck(self.lib.fhelin_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 16, 1 if reset else 0))
        keys = ["limb_ntt", "keyswitch", "keyswitch_limbs", "rescale", "ct_pt_mult", "bootstrap", "encode", "rescale_limbs", "ct_pt_limbs",
                "pool_malloc_calls", "pool_malloc_bytes", "pool_malloc_ns", "pool_reserved_bytes", "pool_live_peak_bytes",
                "pool_reserved_peak_bytes", "pool_trims"]
        return {k: int(v) for k, v in zip(keys, out)}

    def pool_fill_stats(self):
        """(blocks, bytes) the device pool has filled under FHELIN_POOL_FILL (a test aid; both 0 with the knob off)"""
        blocks, nbytes = C.c_uint64(), C.c_uint64()
        self._ck(self.lib.fhelin_debug_pool_fill_stats(self.h, C.byref(blocks), C.byref(nbytes)))
        return blocks.value, nbytes.value

    def cache_stats(self):
        """the plaintext cache of fhelin_encode and the pool's bytes in use right now (fhelin_stats [16..18]; not part of stats(),
        whose keys are per-sample operation counters)"""
        out = np.zeros(19, dtype=np.uint64)
        self._ck(self.lib.fhelin_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), 19, 0))
        return {"pt_cache_bytes": int(out[16]), "pool_live_bytes": int(out[17]), "pt_cache_entries": int(out[18])}

    # ---- keys
    def keygen(self):
        self._ck(self.lib.fhelin_keygen(self.h))

    def gen_relin_key(self):
        self._ck(self.lib.fhelin_gen_relin_key(self.h))

    def gen_rotation_keys(self, indices):
        arr = (C.c_int32 * len(indices))(*indices)
        self._ck(self.lib.fhelin_gen_rotation_keys(self.h, arr, len(indices)))

    def gen_conj_key(self):
        self._ck(self.lib.fhelin_gen_conj_key(self.h))

    @property
    def n_limbs(self):
        return self.n_q + self.n_p

    @property
    def dnum_digits(self):
        return -(-self.n_q // self.alpha)

    def secret_export(self):
        out = np.empty((self.n_limbs, self.N), dtype=np.uint64)
        self._ck(self.lib.fhelin_secret_export(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def secret_import(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        self._ck(self.lib.fhelin_secret_import(self.h, arr.ctypes.data_as(C.c_void_p), arr.size))

    def key_export(self, kind, index=0):
        """[digits][2][n_q + n_p][N]; a level-capped key has digits_at(max_ell) digits and its absent rows zero.  kind 0 relinearisation,
        1 rotation by index, 2 conjugation, 3 / 4 the to-sparse and from-sparse keys of sparse-secret bootstrapping"""
        out = np.empty((self.key_info(kind, index)["digits"], 2, self.n_limbs, self.N), dtype=np.uint64)
        self._ck(self.lib.fhelin_key_export(self.h, kind, index, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    # ---- level-capped keys (include/fhelin.h "Level-capped keys")
    def set_key_caps(self, table):
        """table: (kind, galois, max_ell) entries - kind 1 relinearisation (galois 0), 2 rotation, 3 conjugation (galois 2N-1), as
        key_usage() returns them; every matching key generated afterwards holds only what a switch at <= max_ell limbs reads"""
        table = [tuple(int(v) for v in e) for e in table]
        n = len(table)
        kind = (C.c_int32 * max(1, n))(*[e[0] for e in table])
        gal = (C.c_uint64 * max(1, n))(*[e[1] for e in table])
        cap = (C.c_int32 * max(1, n))(*[e[2] for e in table])
        self._ck(self.lib.fhelin_ctx_set_key_caps(self.h, kind, gal, cap, n))

    def key_info(self, kind, index=0):
        """digits held, max_ell and seeded flag of a key; kind / index as key_export"""
        d, m, s = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.lib.fhelin_key_info(self.h, kind, index, C.byref(d), C.byref(m), C.byref(s)))
        return {"digits": d.value, "max_ell": m.value, "seeded": bool(s.value)}

    def key_usage(self):
        """context manager: records, for every key, the most limbs it is switched at inside the block; the table (a list of
        (kind, galois, max_ell), sorted, the encoding of set_key_caps) is in `.table` once the block has ended.  Everything deferred is
        evaluated when the block ends."""
        return _KeyUsage(self)

    def galois_of(self, index):
        """Galois element of a rotation index at interleave stride 1: 5^index mod 2N"""
        return pow(5, index % (self.N // 2), 2 * self.N)

    def key_import(self, kind, index, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        assert arr.shape == (self.dnum_digits, 2, self.n_limbs, self.N)
        self._ck(self.lib.fhelin_key_import(self.h, kind, index, arr.ctypes.data_as(C.c_void_p), arr.size))

    # ---- evaluation-key sets (include/fhelin.h "Evaluation-key sets")
    def save_eval_keys(self, path, compact=False):
        """write the public parameters and every public key this context holds (never the secret) to `path`.  compact: the b
        halves and the key-set seed only (every key must be seeded: set_seeded_keys before keygen)"""
        fn = self.lib.fhelin_evalkeys_save_compact if compact else self.lib.fhelin_evalkeys_save
        self._ck(fn(self.h, os.fsencode(path)))

    # ---- seeded evaluation keys (include/fhelin.h "Seeded evaluation keys")
    def set_seeded_keys(self, on):
        """on: keygen draws a public key-set seed and every key's a half is its expansion (call before keygen)"""
        self._ck(self.lib.fhelin_ctx_set_seeded_keys(self.h, 1 if on else 0))

    def key_set_seed(self):
        """the public 32-byte key-set seed of a seeded-key context (or one loaded from a compact set)"""
        out = (C.c_uint8 * 32)()
        self._ck(self.lib.fhelin_ctx_key_set_seed(self.h, out))
        return bytes(out)

    @staticmethod
    def eval_keys_params(path):
        """(parameter dict, bootstrap dict or None, key count) of a set's header; host-only"""
        lib = load_library()
        prm, boot, n = Params(), (C.c_int32 * 7)(), C.c_int32()
        for rc in (lib.fhelin_evalkeys_params(os.fsencode(path), C.byref(prm)),
                   lib.fhelin_evalkeys_info(os.fsencode(path), boot, C.byref(n))):
            if rc != 0:
                raise FhelinError(rc, lib.fhelin_last_error().decode())
        cfg = {k: getattr(prm, k) for k in ("log_n", "n_q", "first_bits", "scale_bits", "n_p", "special_bits", "dnum", "log_slots", "hamming")}
        b = list(boot)
        bt = dict(zip(("budget_enc", "budget_dec", "slots", "K", "R", "cheb_degree", "correction"), b)) if b[2] > 0 else None
        return cfg, bt, n.value

    @classmethod
    def from_eval_keys(cls, path, device=0, seed=0):
        """an EVALUATION context (no secret) from a set written by save_eval_keys (full or compact): the header's parameters, its keys, and the
        client's bootstrapping set up again from them when the client had set it up.  seed: this context's own generator
        (public-key encryption randomness), 0 = OS entropy."""
        cfg, boot, _ = cls.eval_keys_params(path)
        eng = cls(cfg, device=device, seed=seed)
        try:
            eng._ck(eng.lib.fhelin_evalkeys_load(eng.h, os.fsencode(path)))
            if boot is not None:
                eng.bootstrap_setup(boot["budget_enc"], boot["budget_dec"], boot["slots"])
        except Exception:
            eng.close()
            raise
        return eng

    def load_eval_keys(self, path):
        """load a set into this (fresh) context; it becomes an evaluation context"""
        self._ck(self.lib.fhelin_evalkeys_load(self.h, os.fsencode(path)))

    def debug_key_digest(self, words, limb_first=0):
        """the device digest kernel on limb vectors words[n][N]: (digests[n] uint64, ok[n] bool)"""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        n = w.shape[0]
        assert w.shape == (n, self.N)
        d, ok = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        self._ck(self.lib.fhelin_debug_key_digest(self.h, w.ctypes.data_as(C.c_void_p), n, int(limb_first),
                                                  d.ctypes.data_as(C.POINTER(C.c_uint64)), ok.ctypes.data_as(C.POINTER(C.c_int32))))
        return d, ok.astype(bool)

    # ---- seeded encryption / compact ciphertexts (include/fhelin.h "Compact ciphertexts")
    def set_seeded_encryption(self, on):
        """on: encrypt / encrypt_batch / client_ingest encrypt with the secret key, c1 expanded from a per-call public seed"""
        self._ck(self.lib.fhelin_ctx_set_seeded_encryption(self.h, 1 if on else 0))

    def import_compact(self, blobs):
        """compact blobs (Ct.export_compact) -> handles, all in one call; all or nothing"""
        bs = [bytes(b) for b in blobs]
        n = len(bs)
        ptrs = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bs])
        sizes = (C.c_size_t * max(n, 1))(*[len(b) for b in bs])
        outs = self._outs(n)
        self._ck(self.lib.fhelin_ct_import_compact(self.h, ptrs, sizes, n, outs))
        return self._cts(outs, n)

    # ---- packed formats (include/fhelin.h "Packed formats")
    def save_evalkeys_packed(self, path, compact=False):
        """save_eval_keys with every residue at its modulus width ("FHELINEP"); from_eval_keys reads it like the other two formats"""
        self._ck(self.lib.fhelin_evalkeys_save_packed(self.h, str(path).encode(), 1 if compact else 0))

    def import_packed(self, blobs):
        """packed blobs (Ct.export_packed, seeded or full) -> handles, all in one call; all or nothing"""
        bs = [bytes(b) for b in blobs]
        n = len(bs)
        ptrs = (C.c_void_p * max(n, 1))(*[C.cast(C.c_char_p(b), C.c_void_p) for b in bs])
        sizes = (C.c_size_t * max(n, 1))(*[len(b) for b in bs])
        outs = self._outs(n)
        self._ck(self.lib.fhelin_ct_import_packed(self.h, ptrs, sizes, n, outs))
        return self._cts(outs, n)

    def debug_pack(self, words, widths):
        """the pack kernel alone: words [n_vec][N] (each below 2^widths[i]) -> the packed vectors back to back, one u64 array"""
        w, wp = _np_u64(words)
        assert w.ndim == 2 and w.shape[1] == self.N
        wd = np.ascontiguousarray(widths, dtype=np.int32)
        assert wd.shape == (w.shape[0],)
        cap = int(self.N // 64 * 64 * w.shape[0])
        out = np.empty(cap, dtype=np.uint64)
        n = C.c_size_t()
        self._ck(self.lib.fhelin_debug_pack(self.h, wp, wd.ctypes.data_as(C.c_void_p), w.shape[0], out.ctypes.data_as(C.c_void_p), cap,
                                            C.byref(n)))
        return out[:n.value].copy()

    def debug_unpack(self, packed, widths):
        """the unpack kernel alone: packed vectors back to back -> [n_vec][N]"""
        p, pp = _np_u64(packed)
        wd = np.ascontiguousarray(widths, dtype=np.int32)
        out = np.empty((wd.size, self.N), dtype=np.uint64)
        self._ck(self.lib.fhelin_debug_unpack(self.h, pp, p.size, wd.ctypes.data_as(C.c_void_p), wd.size, out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_pack_rate(self, widths, reps=5):
        """device-event times of pack, copy, unpack, copy (the copy: the same unpacked bytes, device to device) in turn: ms [reps][4]"""
        wd = np.ascontiguousarray(widths, dtype=np.int32)
        ms = np.zeros((int(reps), 4), dtype=np.float32)
        self._ck(self.lib.fhelin_debug_pack_rate(self.h, wd.ctypes.data_as(C.c_void_p), wd.size, int(reps),
                                                 ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms

    def debug_seeded_expand(self, seed, nonce0, ell, n_ct=1, reps=0, download=True):
        """the expansion kernel alone: (c1 [n_ct][ell][N] or None, mean ms per launch over `reps` timed launches)"""
        sb = (C.c_uint8 * 32)(*bytes(seed))
        out = np.empty((n_ct, ell, self.N), dtype=np.uint64) if download else None
        ms = C.c_float()
        self._ck(self.lib.fhelin_debug_seeded_expand(self.h, sb, nonce0, ell, n_ct, reps,
                                                     out.ctypes.data_as(C.c_void_p) if download else None, C.byref(ms)))
        return out, ms.value

    # ---- plaintexts / ciphertexts
    def encode(self, vals, level=0, slots=0):
        v = np.ascontiguousarray(vals, dtype=np.float64)
        h = C.c_void_p()
        self._ck(self.lib.fhelin_encode(self.h, v.ctypes.data_as(C.POINTER(C.c_double)), v.size, level, slots, C.byref(h)))
        return Pt(self, h)

    def encrypt(self, vals, level=0, slots=0):
        pt = vals if isinstance(vals, Pt) else self.encode(vals, level, slots)
        h = C.c_void_p()
        self._ck(self.lib.fhelin_encrypt(self.h, pt.h, C.byref(h)))
        return Ct(self, h)

    def encrypt_batch(self, rows, level=0, slots=0):
        """rows [n_vec][n_per] -> n_vec fresh ciphertexts: encode + sample + combine as batched GPU kernels"""
        a = np.ascontiguousarray(rows, dtype=np.float64)
        assert a.ndim == 2
        outs = self._outs(a.shape[0])
        self._ck(self.lib.fhelin_encrypt_batch(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.shape[0], a.shape[1], level, slots, outs))
        return self._cts(outs, a.shape[0])

    def client_ingest(self, cls, pos, E_w, E_b, F_w, F_b, emb=None, tokens=None, table=None, level=0, want_proj=False):
        """one sample's client side on the device: (embedding gather,) positional embedding, Linformer projections, expanded packing,
        encode + encrypt.  Returns {"inputs_E": 32 cts, "inputs_F": 32 cts, "inputs": S+1 cts} (+ x_in, proj if want_proj)"""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        cls, pos, E_w, E_b, F_w, F_b = f(cls), f(pos), f(E_w), f(E_b), f(F_w), f(F_b)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        if emb is not None:
            emb = f(emb)
            S, tok, tab, vocab = emb.shape[0], None, None, 0
        else:
            tok = np.ascontiguousarray(tokens, dtype=np.int32)
            tab = f(table)
            S, vocab = tok.shape[0], tab.shape[0]
        if pos.shape[0] < S or pos.shape[1] != 128 or E_w.shape != F_w.shape or E_w.shape[0] != 32 or E_w.shape[1] < S + 1 or cls.size != 128 \
                or E_b.size != 32 or F_b.size != 32:
            raise FhelinError(1, "client_ingest: pos needs >= S rows of 128, E_w / F_w [32][>= S + 1], E_b / F_b [32], cls [128]")
        n = 64 + S + 1
        outs = self._outs(n)
        proj = np.empty((S + 1 + 64, 128)) if want_proj else None
        self._ck(self.lib.fhelin_client_ingest(self.h, p(emb), p(tok), p(tab), vocab, S, p(cls), p(pos), p(E_w), p(E_b), p(F_w), p(F_b),
                                               E_w.shape[1], level, outs, p(proj)))
        cts = self._cts(outs, n)
        res = {"inputs_E": cts[:32], "inputs_F": cts[32:64], "inputs": cts[64:]}
        if want_proj:
            res["x_in"], res["proj"] = proj[:S + 1], proj[S + 1:]
        return res

    def client_ingest_wrapped(self, cls, pos, E_w, E_b, F_w, F_b, emb=None, tokens=None, table=None, level=0, targets=None, want_proj=False):
        """client_ingest's sample as wrapped ciphertexts (include/fhelin.h "Wrapped inputs"): a list of wrapped handles (<= 128 inputs
        each); targets [64 + S + 1] (optional): limbs per input.  want_proj: (handles, x_in, proj)"""
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        cls, pos, E_w, E_b, F_w, F_b = f(cls), f(pos), f(E_w), f(E_b), f(F_w), f(F_b)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        if emb is not None:
            emb = f(emb)
            S, tok, tab, vocab = emb.shape[0], None, None, 0
        else:
            tok = np.ascontiguousarray(tokens, dtype=np.int32)
            tab = f(table)
            S, vocab = tok.shape[0], tab.shape[0]
        if pos.shape[0] < S or pos.shape[1] != 128 or E_w.shape != F_w.shape or E_w.shape[0] != 32 or E_w.shape[1] < S + 1 or cls.size != 128 \
                or E_b.size != 32 or F_b.size != 32:
            raise FhelinError(1, "client_ingest_wrapped: pos needs >= S rows of 128, E_w / F_w [32][>= S + 1], E_b / F_b [32], cls [128]")
        n = 64 + S + 1
        tg = None
        if targets is not None:
            tg = np.ascontiguousarray(targets, dtype=np.int32)
            if tg.size != n:
                raise FhelinError(1, "client_ingest_wrapped: one target per input")
        outs = self._outs(n)
        n_out = C.c_int32()
        proj = np.empty((S + 1 + 64, 128)) if want_proj else None
        self._ck(self.lib.fhelin_client_ingest_wrapped(self.h, p(emb), p(tok), p(tab), vocab, S, p(cls), p(pos), p(E_w), p(E_b), p(F_w),
                                                       p(F_b), E_w.shape[1], level, p(tg), outs, C.byref(n_out), p(proj)))
        cts = self._cts(outs, n_out.value)
        return (cts, proj[:S + 1], proj[S + 1:]) if want_proj else cts

    def unwrap_inputs(self, wrapped):
        """wrapped handles of one or more samples -> their expanded inputs, sample by sample in read order"""
        ws = list(wrapped)
        total = sum(w.wrapped_info()["count"] for w in ws)
        arr = (C.c_void_p * max(len(ws), 1))(*[w.h for w in ws])
        outs = self._outs(total)
        self._ck(self.lib.fhelin_unwrap_inputs(self.h, arr, len(ws), outs))
        return self._cts(outs, total)

    # ---- sanitised replies (include/fhelin.h "Sanitised replies")
    def sanitize(self, cts, mask=None, flood_bits=0, out_ell=2):
        """the reply form of result ciphertexts: degree 2 rescaled, the optional 0/1 mask (a Pt, or slot values) applied, the first
        out_ell limbs kept, a fresh public-key encryption of zero and a flood term uniform on [-2^flood_bits, 2^flood_bits) added -
        one fused launch for the whole list.  A single Ct gives a single Ct.  Works on an evaluation context."""
        single = isinstance(cts, Ct)
        v = [cts] if single else list(cts)
        pt = None
        if mask is not None:
            pt = mask if isinstance(mask, Pt) else self.encode(mask)
        outs = self._outs(len(v))
        arr = (C.c_void_p * max(len(v), 1))(*[c.h for c in v])
        self._ck(self.lib.fhelin_sanitize(self.h, arr, len(v), pt.h if pt is not None else None, int(flood_bits), int(out_ell), outs))
        r = self._cts(outs, len(v))
        return r[0] if single else r

    def debug_flood(self, key, stream, flood_bits, ell=None):
        """the wide sampler alone for an explicit 32-byte ChaCha20 key and stream: residues [ell][N], coefficient form"""
        ell = self.n_q if ell is None else int(ell)
        kb = (C.c_uint8 * 32)(*bytes(key))
        out = np.empty((max(ell, 0), self.N), dtype=np.uint64)
        self._ck(self.lib.fhelin_debug_flood(self.h, kb, int(stream), int(flood_bits), ell, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def debug_sampler_peek(self, n_keys=1):
        """test hook (include/fhelin.h "Sampler streams"): (keys uint32 [n_keys][8] that the next n_keys sampler-key draws will give,
        the current sampler call counter); consumes nothing; host-only"""
        keys = np.zeros((int(n_keys), 8), dtype=np.uint32)
        calls = C.c_uint64()
        self._ck(self.lib.fhelin_debug_sampler_peek(self.h, int(n_keys), keys.ctypes.data_as(C.c_void_p) if keys.size else None,
                                                    C.byref(calls)))
        return keys, int(calls.value)

    def decrypt_flooded(self, ct, flood_bits, slots=0):
        """noise-flooding decryption: decrypt with one flood polynomial added to the phase before the download; flood_bits=0 is decrypt"""
        n = slots or ct.slots or (1 << self.params.log_slots)
        out = np.empty(n, dtype=np.float64)
        self._ck(self.lib.fhelin_decrypt_flooded(self.h, ct.h, int(flood_bits), out.ctypes.data_as(C.POINTER(C.c_double)), n))
        return out

    def set_host_encode(self, on):
        self._ck(self.lib.fhelin_ctx_set_host_encode(self.h, 1 if on else 0))

    def debug_sample(self, kind, n_poly=1):
        out = np.empty((n_poly, self.N), dtype=np.int64)
        self._ck(self.lib.fhelin_debug_sample(self.h, kind, n_poly, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def decrypt(self, ct, slots=0):
        n = slots or ct.slots or (1 << self.params.log_slots)
        out = np.empty(n, dtype=np.float64)
        self._ck(self.lib.fhelin_decrypt(self.h, ct.h, out.ctypes.data_as(C.POINTER(C.c_double)), n))
        return out

    def decrypt_batch(self, cts, slots=0, flood_bits=0, idx=None, all_lanes=False):
        """batched decryption (include/fhelin.h "Batched decryption"): the decoder on the device, one download and one synchronisation
        for the batch.  Returns [n][W] - row b is decrypt(cts[b]), bit for bit - or [n][stride][W] with all_lanes (decrypt_interleaved's
        order); W = slots, or len(idx) when idx (logical slot numbers) is given.  slots=0: the ciphertexts' own count, which must agree.
        flood_bits > 0: one key draw for the batch (a batch of one is decrypt_flooded)"""
        cts = list(cts)
        n = len(cts)
        lanes = self.interleave if all_lanes else 1
        ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        own = int(slots) or (cts[0].slots if n else 0) or (1 << self.params.log_slots)
        width = own if ix is None else ix.size
        out = np.empty((n, lanes, width), dtype=np.float64)
        arr = (C.c_void_p * max(n, 1))(*[c.h for c in cts])
        self._ck(self.lib.fhelin_decrypt_batch(self.h, arr, n, int(flood_bits), 1 if all_lanes else 0,
                                               None if ix is None else ix.ctypes.data_as(C.POINTER(C.c_int32)), 0 if ix is None else ix.size,
                                               out.ctypes.data_as(C.POINTER(C.c_double)), int(slots)))
        return out if all_lanes else out[:, 0, :]

    def set_device_decode(self, on):
        """decrypt, decrypt_flooded and decrypt_interleaved through the device decoder, as batches of one (default off; FHELIN_DEVICE_DECODE)"""
        self._ck(self.lib.fhelin_ctx_set_device_decode(self.h, 1 if on else 0))

    def ct_import(self, limbs, deg=1, scale=None, slots=0):
        limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
        npoly, ell, n = limbs.shape
        assert n == self.N
        if scale is None:
            scale = float(self.scaling_factors[self.n_q - ell])
        h = C.c_void_p()
        self._ck(self.lib.fhelin_ct_import(self.h, limbs.ctypes.data_as(C.c_void_p), npoly, ell, deg, scale, slots, C.byref(h)))
        return Ct(self, h)

    def _un(self, fn, a, *extra):
        h = C.c_void_p()
        self._ck(fn(self.h, a.h, *extra, C.byref(h)))
        return Ct(self, h)

    def add(self, a, b):
        return self._un(self.lib.fhelin_add_plain if isinstance(b, Pt) else self.lib.fhelin_add, a, b.h)

    def sub(self, a, b):
        return self._un(self.lib.fhelin_sub, a, b.h)

    def negate(self, a):
        return self._un(self.lib.fhelin_negate, a)

    def mult(self, a, b):
        return self._un(self.lib.fhelin_mult_plain if isinstance(b, Pt) else self.lib.fhelin_mult, a, b.h)

    def rotate(self, a, index):
        return self._un(self.lib.fhelin_rotate, a, index)

    def rotate_many(self, a, indices):
        """hoisted rotations of one ciphertext (one ModUp, bit-identical to rotate(a, i) for every i)"""
        idx = (C.c_int32 * len(indices))(*indices)
        outs = self._outs(len(indices))
        self._ck(self.lib.fhelin_rotate_many(self.h, a.h, idx, len(indices), outs))
        return self._cts(outs, len(indices))

    def rotate_each(self, v, indices):
        idx = (C.c_int32 * len(indices))(*indices)
        outs = self._outs(len(v))
        self._ck(self.lib.fhelin_rotate_each(self.h, self._harr(v), idx, len(v), outs))
        return self._cts(outs, len(v))

    def rotate_sum(self, v, indices):
        """v[i] + sum_r rot(v[i], indices[r]): one ModUp and one ModDown per row"""
        idx = (C.c_int32 * len(indices))(*indices)
        outs = self._outs(len(v))
        self._ck(self.lib.fhelin_rotate_sum(self.h, self._harr(v), len(v), idx, len(indices), outs))
        return self._cts(outs, len(v))

    def hoisted_dot(self, v, pts, indices, rescale=False):
        """v[i] * pts[0] + sum_r rot(v[i], indices[r]) * pts[r + 1]: one ModUp and one ModDown per row, plaintext products in the
        extended basis (plaintext-folded rotation keys); rescale: ModDown and rescale as one basis conversion"""
        assert len(pts) == len(indices) + 1
        idx = (C.c_int32 * len(indices))(*indices)
        parr = (C.c_void_p * len(pts))(*[p.h for p in pts])
        outs = self._outs(len(v))
        self._ck(self.lib.fhelin_hoisted_dot(self.h, self._harr(v), len(v), parr, idx, len(indices), int(bool(rescale)), outs))
        return self._cts(outs, len(v))

    def rotate_each_sum(self, v, indices):
        """sum_i rot(v[i], indices[i]): own ModUp per term, one shared ModDown per <= 7 terms"""
        idx = (C.c_int32 * len(indices))(*indices)
        h = C.c_void_p()
        self._ck(self.lib.fhelin_rotate_each_sum(self.h, self._harr(v), idx, len(v), C.byref(h)))
        return Ct(self, h)

    def raw_modraise(self, a, new_ell):
        return self._un(self.lib.fhelin_raw_modraise, a, new_ell)

    def raw_phase(self, a):
        return self._un(self.lib.fhelin_raw_phase, a)

    def pt_export(self, pt, ell, scale=0.0):
        """[ell][N] residues of the plaintext's encoding at (ell limbs, scale); scale 0 = Delta of that level.  `scale`
        may be a numpy longdouble: it travels exactly as hi + lo doubles."""
        out = np.empty((ell, self.N), dtype=np.uint64)     # ell = n_q + n_p (explicit scale): the encoding over the full key basis
        hi = float(scale)
        lo = float(np.longdouble(scale) - np.longdouble(hi))
        self._ck(self.lib.fhelin_pt_export(self.h, pt.h, ell, hi, lo, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def rescale(self, a):
        return self._un(self.lib.fhelin_rescale, a)

    # ---- leaf ops over independent rows (one launch set per chunk of rows of equal shape)
    def _rows(self, fn, v, *extra):
        outs = self._outs(len(v))
        self._ck(fn(self.h, self._harr(v), *extra, outs))
        return self._cts(outs, len(v))

    def rotate_batch(self, v, index):
        return self._rows(self.lib.fhelin_rotate_batch, v, len(v), index)

    def rescale_batch(self, v):
        return self._rows(self.lib.fhelin_rescale_batch, v, len(v))

    def mult_plain_batch(self, v, pt):
        return self._rows(self.lib.fhelin_mult_plain_batch, v, len(v), pt.h)

    def mult_batch(self, a, b):
        outs = self._outs(len(a))
        self._ck(self.lib.fhelin_mult_batch(self.h, self._harr(a), self._harr(b), len(a), outs))
        return self._cts(outs, len(a))

    def mult_affine_batch(self, a, b, f, cadd, addend=None, negate=None):
        """rescale(f[i] * a[i] * b[i] + cadd[i] +- addend[i]) through one batched key switch (addend[i] may be None); the residues of
        mult_batch, add_batch, add_real / sub, rescale"""
        n = len(a)
        outs = self._outs(n)
        fa = (C.c_int32 * n)(*[int(v) for v in f])
        ca = (C.c_double * n)(*[float(v) for v in cadd])
        ad = (C.c_void_p * n)(*[(x.h if x is not None else None) for x in (addend or [None] * n)])
        ng = (C.c_int32 * n)(*[int(bool(v)) for v in (negate or [0] * n)])
        self._ck(self.lib.fhelin_mult_affine_batch(self.h, self._harr(a), self._harr(b), n, fa, ca, ad, ng, outs))
        return self._cts(outs, n)

    def add_batch(self, a, b):
        outs = self._outs(len(a))
        self._ck(self.lib.fhelin_add_batch(self.h, self._harr(a), self._harr(b), len(a), outs))
        return self._cts(outs, len(a))

    def level_reduce(self, a, new_ell):
        return self._un(self.lib.fhelin_level_reduce, a, new_ell)

    def raw_rescale(self, a):
        return self._un(self.lib.fhelin_raw_rescale, a)

    def raw_rotate(self, a, index):
        return self._un(self.lib.fhelin_raw_rotate, a, index)

    def raw_mult_relin(self, a, b):
        return self._un(self.lib.fhelin_raw_mult_relin, a, b.h)

    # ---- test hooks: the plaintext inner-sum kernels on chosen residues (include/fhelin.h "test hooks")
    @staticmethod
    def _harr_opt(objs):
        return (C.c_void_p * len(objs))(*[(o.h if o is not None else None) for o in objs])

    def debug_pt_from_residues(self, residues):
        """a plaintext whose only encoding is residues [ell][N] (NTT form) at ell limbs and that limb count's own scale"""
        r = np.ascontiguousarray(residues, dtype=np.uint64)
        ell, n = r.shape
        assert n == self.N
        h = C.c_void_p()
        self._ck(self.lib.fhelin_debug_pt_from_residues(self.h, r.ctypes.data_as(C.c_void_p), ell, C.byref(h)))
        return Pt(self, h)

    def debug_pt_from_residues_full(self, residues, scale):
        """a plaintext whose only encoding is residues [n_q + n_p][N] over the full key basis at `scale` (may be a numpy longdouble)"""
        r = np.ascontiguousarray(residues, dtype=np.uint64)
        assert r.shape == (self.n_q + self.n_p, self.N)
        hi = float(scale)
        lo = float(np.longdouble(scale) - np.longdouble(hi))
        h = C.c_void_p()
        self._ck(self.lib.fhelin_debug_pt_from_residues_full(self.h, r.ctypes.data_as(C.c_void_p), hi, lo, C.byref(h)))
        return Pt(self, h)

    # ---- linear transforms (include/fhelin.h "Linear transforms")
    def lt_create(self, diags, indices, n1=0, slots=None):
        """the plan of out = sum_d diags[d] * rot(x, indices[d]); diags [n_diag][slots]; n1 = 0: the planner chooses the split"""
        slots = (1 << self.params.log_slots) if slots is None else int(slots)
        n = len(indices)
        d = np.ascontiguousarray(diags, dtype=np.float64).reshape(n, -1) if n else np.zeros((0, slots))
        assert n == 0 or d.shape[1] == slots
        idx = (C.c_int32 * max(n, 1))(*[int(i) for i in indices])
        h = C.c_void_p()
        self._ck(self.lib.fhelin_lt_create(self.h, d.ctypes.data_as(C.POINTER(C.c_double)), idx, n, slots, int(n1), C.byref(h)))
        return LinearTransform(self, h)

    def lt_create_pts(self, pts, baby, giant):
        """the plan from its terms: pts [n2][n1] of Pt (None = absent), baby [n1] (baby[0] == 0), giant [n2]"""
        n2, n1 = len(giant), len(baby)
        assert len(pts) == n2 and all(len(r) == n1 for r in pts)
        b = (C.c_int32 * n1)(*[int(i) for i in baby])
        g = (C.c_int32 * n2)(*[int(i) for i in giant])
        h = C.c_void_p()
        self._ck(self.lib.fhelin_lt_create_pts(self.h, self._harr_opt([p for r in pts for p in r]), b, g, n1, n2, C.byref(h)))
        return LinearTransform(self, h)

    def lt_apply(self, lt, v, rescale=False):
        """the transform of every ciphertext of v: one ModUp per row, one ModDown per giant-step group, rows of one shape batched"""
        outs = self._outs(max(len(v), 1))
        self._ck(self.lib.fhelin_lt_apply(self.h, lt.h, self._harr(v), len(v), int(bool(rescale)), outs))
        return self._cts(outs, len(v))

    def debug_dot_plain(self, cts, pts):
        """sum_i cts[i] * pts[i] (Evaluator::dot_plain)"""
        assert len(cts) == len(pts)
        h = C.c_void_p()
        self._ck(self.lib.fhelin_debug_dot_plain(self.h, self._harr(cts), self._harr(pts), len(cts), C.byref(h)))
        return Ct(self, h)

    def debug_dot_groups(self, cts, pts):
        """cts [nb][na], pts [ng][na] (None = term absent) -> outs [nb][ng], outs[x][g] = sum_b cts[x][b] * pts[g][b] in one launch"""
        nb, na, ng = len(cts), len(cts[0]), len(pts)
        assert all(len(r) == na for r in cts) and all(len(r) == na for r in pts)
        outs = self._outs(nb * ng)
        self._ck(self.lib.fhelin_debug_dot_groups(self.h, self._harr([c for r in cts for c in r]), nb, na,
                                                  self._harr_opt([p for r in pts for p in r]), ng, outs))
        flat = self._cts(outs, nb * ng)
        return [flat[x * ng:(x + 1) * ng] for x in range(nb)]

    def debug_dot_cyclic(self, cts, pts):
        """outs[k] = sum_i cts[i] * pts[(i + k) mod 32], k < 32 (Evaluator::dot_plain_cyclic)"""
        assert len(pts) == 32
        outs = self._outs(32)
        self._ck(self.lib.fhelin_debug_dot_cyclic(self.h, self._harr(cts), len(cts), self._harr(pts), outs))
        return self._cts(outs, 32)

    def debug_dot_window(self, cur, prev, pts, dest, accumulate=False):
        """dest[t] (+)= sum_j (j <= t ? cur[j] : prev[j]) * pts[(t - j) mod 32]; cur / prev entries may be None; dest is written in place"""
        assert len(cur) == len(prev) == len(pts) == len(dest) == 32
        self._ck(self.lib.fhelin_debug_dot_window(self.h, self._harr_opt(cur), self._harr_opt(prev), self._harr(pts), self._harr(dest),
                                                  int(bool(accumulate))))

    def debug_rotate_many_batch(self, cts, indices):
        """outs[i][k] = rot(cts[i], indices[k]): hoisted rotations of many inputs behind one ModUp (Evaluator::rotate_many_batch)"""
        n = len(indices)
        idx = (C.c_int32 * n)(*indices)
        outs = self._outs(len(cts) * n)
        self._ck(self.lib.fhelin_debug_rotate_many_batch(self.h, self._harr(cts), len(cts), idx, n, outs))
        flat = self._cts(outs, len(cts) * n)
        return [flat[i * n:(i + 1) * n] for i in range(len(cts))]

    def debug_ks_accp(self, digits, ell, indices=()):
        """INTT of the special-limb half of a key switch's inner product over the given digits [batch][beta][ell + n_p][N] (any values
        below 2^60): the identity form over the relinearisation key, or the merged form over `indices` (fhelin.h)"""
        d = np.ascontiguousarray(digits, dtype=np.uint64)
        batch, n = d.shape[0], len(indices)
        assert d.shape[2:] == (ell + self.n_p, self.N)
        idx = (C.c_int32 * max(n, 1))(*indices)
        out = np.empty((batch, 2, self.n_p, self.N), dtype=np.uint64)
        self._ck(self.lib.fhelin_debug_ks_accp(self.h, d.ctypes.data_as(C.c_void_p), ell, batch, idx, n, out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_ks_accq(self, digits, own, conv, ell, index=0):
        """(accQ - NTT(conv)) * P^-1 [batch][2][ell][N] with accQ the Q-limb half of a key switch's inner product over the given digits
        [batch][beta][ell + n_p][N] (any values below 2^60) and own limb [batch][ell][N], conv [batch][2][ell][N] in coefficient form:
        the identity form over the relinearisation key, or the gathered form of rotation `index` (fhelin.h)"""
        d = np.ascontiguousarray(digits, dtype=np.uint64)
        o = np.ascontiguousarray(own, dtype=np.uint64)
        cv = np.ascontiguousarray(conv, dtype=np.uint64)
        batch = d.shape[0]
        assert d.shape[2:] == (ell + self.n_p, self.N) and o.shape == (batch, ell, self.N) and cv.shape == (batch, 2, ell, self.N)
        out = np.empty((batch, 2, ell, self.N), dtype=np.uint64)
        vp = C.c_void_p
        self._ck(self.lib.fhelin_debug_ks_accq(self.h, d.ctypes.data_as(vp), o.ctypes.data_as(vp), cv.ctypes.data_as(vp), ell, batch, index,
                                               out.ctypes.data_as(vp)))
        return out

    # ---- FHEController composites (names follow the reference methods)
    @staticmethod
    def _harr(objs):
        return (C.c_void_p * len(objs))(*[o.h for o in objs])

    def _outs(self, n):
        return (C.c_void_p * n)()

    def _cts(self, arr, n):
        return [Ct(self, C.c_void_p(arr[i])) for i in range(n)]

    def mult_real(self, a, k):
        return self._un(self.lib.fhelin_mult_real, a, float(k))

    def add_real(self, a, k):
        return self._un(self.lib.fhelin_add_real, a, float(k))

    def mult_many(self, v):
        h = C.c_void_p()
        self._ck(self.lib.fhelin_mult_many(self.h, self._harr(v), len(v), C.byref(h)))
        return Ct(self, h)

    def lincomb(self, v, coeffs, c0=0.0):
        cf = np.ascontiguousarray(coeffs, dtype=np.float64)
        h = C.c_void_p()
        self._ck(self.lib.fhelin_lincomb(self.h, self._harr(v), cf.ctypes.data_as(C.POINTER(C.c_double)), len(v), float(c0), C.byref(h)))
        return Ct(self, h)

    def eval_poly(self, x, coeffs):
        cf = np.ascontiguousarray(coeffs, dtype=np.float64)
        return self._un(self.lib.fhelin_eval_poly, x, cf.ctypes.data_as(C.POINTER(C.c_double)), cf.size)

    def eval_chebyshev(self, x, coeffs, a=-1.0, b=1.0):
        cf = np.ascontiguousarray(coeffs, dtype=np.float64)
        return self._un(self.lib.fhelin_eval_chebyshev, x, cf.ctypes.data_as(C.POINTER(C.c_double)), cf.size, float(a), float(b))

    def eval_chebyshev_batch(self, xs, coeffs, a=-1.0, b=1.0):
        cf = np.ascontiguousarray(coeffs, dtype=np.float64)
        outs = self._outs(len(xs))
        self._ck(self.lib.fhelin_eval_chebyshev_batch(self.h, self._harr(xs), len(xs), cf.ctypes.data_as(C.POINTER(C.c_double)), cf.size,
                                                      float(a), float(b), outs))
        return self._cts(outs, len(xs))

    def bootstrap(self, a):
        return self._un(self.lib.fhelin_bootstrap, a)

    def bootstrap_setup(self, budget_enc=3, budget_dec=3, slots=0):
        self._ck(self.lib.fhelin_bootstrap_setup(self.h, budget_enc, budget_dec, slots))

    def bootstrap_config(self, K=28, R=3, cheb_degree=47, correction=10):
        """all four parameters are written, the defaults included: under set_bootstrap_sparse_secret a call that names only `correction`
        puts K and the degree back to 28 and 47 (still a correct bootstrap - the depth follows the degree - but at 15 levels again)"""
        self._ck(self.lib.fhelin_bootstrap_config(self.h, K, R, cheb_degree, correction))

    def bootstrap_batch(self, v):
        """EvalBootstrap on independent ciphertexts in one batched pipeline (same residues as bootstrap() one by one)"""
        outs = self._outs(len(v))
        self._ck(self.lib.fhelin_bootstrap_batch(self.h, self._harr(v), len(v), outs))
        return self._cts(outs, len(v))

    def bootstrap_drop(self, a, drop):
        """bootstrap raising to L+1-drop limbs only (what a level plan asks of a bootstrap)"""
        return self._un(self.lib.fhelin_bootstrap_drop, a, int(drop))

    def bootstrap_iter(self, a, precision):
        """iterative (two-pass) bootstrap, EvalBootstrap(a, 2, precision): about twice the bits of bootstrap(), one limb fewer
        (include/fhelin.h fhelin_bootstrap_iter; 1 <= precision <= 30, useful up to one bootstrap's precision)"""
        return self._un(self.lib.fhelin_bootstrap_iter, a, int(precision))

    def bootstrap_iter_batch(self, v, precision):
        """bootstrap_iter on independent ciphertexts, both bootstraps batched (same residues as bootstrap_iter() one by one)"""
        outs = self._outs(len(v))
        self._ck(self.lib.fhelin_bootstrap_iter_batch(self.h, self._harr(v), len(v), int(precision), outs))
        return self._cts(outs, len(v))

    def bootstrap_iter_drop(self, a, precision, drop):
        """bootstrap_iter with both bootstraps raising to L+1-drop limbs only"""
        return self._un(self.lib.fhelin_bootstrap_iter_drop, a, int(precision), int(drop))

    def bootstrap_pair(self, a, b):
        """two ciphertexts with REAL slot values through one bootstrap as a + i b (include/fhelin.h "Paired bootstrapping"): (a', b')"""
        ha, hb = C.c_void_p(), C.c_void_p()
        self._ck(self.lib.fhelin_bootstrap_pair(self.h, a.h, b.h, C.byref(ha), C.byref(hb)))
        return Ct(self, ha), Ct(self, hb)

    def bootstrap_paired_batch(self, v):
        """bootstrap_batch with consecutive inputs paired: ceil(n / 2) pipelines; an odd last input comes out as bootstrap() gives it"""
        outs = self._outs(max(len(v), 1))
        self._ck(self.lib.fhelin_bootstrap_paired_batch(self.h, self._harr(v), len(v), outs))
        return self._cts(outs, len(v))

    def bootstrap_pair_drop(self, a, b, drop):
        """bootstrap_pair raising to L+1-drop limbs only"""
        ha, hb = C.c_void_p(), C.c_void_p()
        self._ck(self.lib.fhelin_bootstrap_pair_drop(self.h, a.h, b.h, int(drop), C.byref(ha), C.byref(hb)))
        return Ct(self, ha), Ct(self, hb)

    def bootstrap_pair_partial(self, a, b, stage):
        """the pair's pipeline stopped after stage 1, 2 or 3 (as bootstrap_partial)"""
        h = C.c_void_p()
        self._ck(self.lib.fhelin_bootstrap_pair_partial(self.h, a.h, b.h, int(stage), C.byref(h)))
        return Ct(self, h)

    def set_bootstrap_pairing(self, on):
        """deferred bootstrap() calls that are ready together go through the paired pipeline (off by default; FHELIN_BOOT_PAIRS=1)"""
        self._ck(self.lib.fhelin_ctx_set_bootstrap_pairing(self.h, int(bool(on))))

    def bootstrap_pairing(self):
        on = C.c_int32()
        self._ck(self.lib.fhelin_ctx_bootstrap_pairing(self.h, C.byref(on)))
        return bool(on.value)

    def set_bootstrap_lt(self, on, n1=0):
        """the bootstrap's linear stages on the linear-transform engine (include/fhelin.h "Bootstrap linear stages"; off by default,
        FHELIN_BOOT_LT=1 / FHELIN_BOOT_LT_N1=k).  n1 = 0: the planner chooses per stage; 1..32 forces the baby-step count.  Binds at
        bootstrap_setup: FHELIN_ERR_STATE afterwards"""
        self._ck(self.lib.fhelin_ctx_set_bootstrap_lt(self.h, int(bool(on)), int(n1)))

    def bootstrap_lt(self):
        """(on, n1) of set_bootstrap_lt"""
        on, n1 = C.c_int32(), C.c_int32()
        self._ck(self.lib.fhelin_ctx_bootstrap_lt(self.h, C.byref(on), C.byref(n1)))
        return bool(on.value), n1.value

    def set_bootstrap_sparse_secret(self, hamming):
        """sparse-secret bootstrapping (include/fhelin.h "Sparse-secret bootstrapping"; off = 0 by default, FHELIN_BOOT_SPARSE_H=h): key
        switches to an ephemeral secret of this Hamming weight around the ModRaise - at 32, K = 12, a degree-28 cosine fit and 14 levels
        per bootstrap instead of 15, for two more key switches.  8 <= hamming <= N; binds at bootstrap_setup: FHELIN_ERR_STATE afterwards.
        Writes K, R and cheb_degree; a later bootstrap_config overrides them - ALL of them, its defaults included"""
        self._ck(self.lib.fhelin_ctx_set_bootstrap_sparse_secret(self.h, int(hamming)))

    def bootstrap_sparse_secret(self):
        """the Hamming weight of set_bootstrap_sparse_secret (0: off)"""
        h = C.c_int32()
        self._ck(self.lib.fhelin_ctx_bootstrap_sparse_secret(self.h, C.byref(h)))
        return h.value

    def boot_sparse_secret(self):
        """test hook: the coefficients (-1, 0, 1) of the ephemeral secret, int8 [N]; client contexts only, after bootstrap_setup"""
        out = np.empty(self.N, dtype=np.int8)
        self._ck(self.lib.fhelin_debug_boot_sparse_secret(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def debug_pair_pack(self, a, b, k0_a, k0_b):
        """outs[i] = k0_a[i] a[i] + X^(N/2) k0_b[i] b[i] on the two bottom limbs, every pair in one launch (launch_ew_pair_pack)"""
        n = len(a)
        assert len(b) == len(k0_a) == len(k0_b) == n
        ka, kb = (C.c_uint64 * n)(*[int(k) for k in k0_a]), (C.c_uint64 * n)(*[int(k) for k in k0_b])
        outs = self._outs(n)
        self._ck(self.lib.fhelin_debug_pair_pack(self.h, self._harr(a), self._harr(b), ka, kb, n, outs))
        return self._cts(outs, n)

    def debug_pair_split(self, w, wc):
        """(w[i] + wc[i], X^(N/2) (wc[i] - w[i])) for every pair in one launch (launch_ew_pair_split): (list of a, list of b)"""
        n = len(w)
        assert len(wc) == n
        oa, ob = self._outs(n), self._outs(n)
        self._ck(self.lib.fhelin_debug_pair_split(self.h, self._harr(w), self._harr(wc), n, oa, ob))
        return self._cts(oa, n), self._cts(ob, n)

    def bootstrap_describe(self):
        """the bootstrapping set-up as the residue-level oracle needs it: parameters + per linear stage the stage's slot count
        and its (giant, baby, diagonal plaintext) terms in evaluation order.  "lt": whether the stages run on the linear-transform
        engine (set_bootstrap_lt); then every stage also has "n1", "n2" of its split, and "lt_n1" (the n1 asked for) and
        "encoding_bytes" (device bytes of the stages' limb-sliced encodings so far) are set.  "sparse_h": the Hamming weight of
        sparse-secret bootstrapping's ephemeral secret (set_bootstrap_sparse_secret), 0 with the knob off"""
        n = C.c_int32()
        self._ck(self.lib.fhelin_bootstrap_describe(self.h, None, 0, C.byref(n)))
        d = (C.c_int32 * n.value)()
        self._ck(self.lib.fhelin_bootstrap_describe(self.h, d, n.value, C.byref(n)))
        d = list(d)
        out = dict(zip(("packed", "slots", "K", "R", "cheb_degree", "correction", "depth"), d[:7]))
        out["packed"] = bool(out["packed"])
        n_c2s, n_s2c = d[7], d[8]
        pos, stages = 9, []
        for k in range(n_c2s + n_s2c):
            which, idx = (0, k) if k < n_c2s else (1, k - n_c2s)
            st_slots, nt = d[pos], d[pos + 1]
            pos += 2
            terms = []
            for t in range(nt):
                h = C.c_void_p()
                self._ck(self.lib.fhelin_bootstrap_diag(self.h, which, idx, t, C.byref(h)))
                terms.append((d[pos], d[pos + 1], Pt(self, h)))
                pos += 2
            stages.append(dict(slots=st_slots, terms=terms))
        out["lt"] = pos < len(d) and d[pos] == 1
        if out["lt"]:
            out["lt_n1"] = d[pos + 1]
            pos += 2
            for st in stages:
                st["n1"], st["n2"] = d[pos], d[pos + 1]
                pos += 2
            out["encoding_bytes"] = (d[pos] & 0xffffffff) | ((d[pos + 1] & 0xffffffff) << 32)
            pos += 2
        out["sparse_h"] = d[pos + 1] if pos + 1 < len(d) and d[pos] == 2 else 0   # sparse-secret bootstrapping's trailer (2, h~)
        out["c2s"], out["s2c"] = stages[:n_c2s], stages[n_c2s:]
        cn = C.c_int32()
        self._ck(self.lib.fhelin_bootstrap_cheb(self.h, None, 0, C.byref(cn)))
        cf = (C.c_double * cn.value)()
        self._ck(self.lib.fhelin_bootstrap_cheb(self.h, cf, cn.value, C.byref(cn)))
        out["cheb"] = list(cf)
        return out

    def bootstrap_partial(self, a, stage):
        return self._un(self.lib.fhelin_bootstrap_partial, a, stage)

    def mult_const(self, a, d):
        return self._un(self.lib.fhelin_fc_mult_const, a, float(d))

    def mask_block(self, a, frm, to, v=1.0):
        return self._un(self.lib.fhelin_fc_mask, a, 0, frm, to, float(v))

    def mask_heads(self, a, v=1.0):
        return self._un(self.lib.fhelin_fc_mask, a, 1, 0, 0, float(v))

    def mask_heads_128(self, a, v=1.0):
        return self._un(self.lib.fhelin_fc_mask, a, 2, 0, 0, float(v))

    def mask_mod_n(self, a, n, padding=0):
        return self._un(self.lib.fhelin_fc_mask, a, 3, n, padding, 1.0)

    def mask_first_n(self, a, n, v=1.0):
        return self._un(self.lib.fhelin_fc_mask, a, 4, n, 0, float(v))

    def rotsum(self, a, slots, padding):
        return self._un(self.lib.fhelin_fc_rotsum, a, slots, padding)

    def repeat(self, a, slots, padding=1):
        return self._un(self.lib.fhelin_fc_repeat, a, slots, padding)

    def add_many(self, v):
        h = C.c_void_p()
        self._ck(self.lib.fhelin_fc_add_many(self.h, self._harr(v), len(v), C.byref(h)))
        return Ct(self, h)

    def matmul_pt(self, rows, w, bias, slots, padding):
        outs = self._outs(len(rows))
        self._ck(self.lib.fhelin_fc_matmul_pt(self.h, self._harr(rows), len(rows), w.h, bias.h if bias else None, slots, padding, outs))
        return self._cts(outs, len(rows))

    def matmulRE(self, rows, w, bias=None, row_size=128, padding=128):
        if isinstance(w, Ct):
            return self.matmul_ct(rows, w, row_size, padding)
        return self.matmul_pt(rows, w, bias, row_size, padding)

    def matmulCR(self, rows, w, bias=None):
        if isinstance(w, Ct):
            return self.matmul_ct(rows, w, 64, 1)
        return self.matmul_pt(rows, w, bias, 128, 1)

    def matmulCR_128(self, rows, w):
        return self.matmul_ct(rows, w, 128, 1)

    def matmul_ct(self, rows, w, slots, padding):
        outs = self._outs(len(rows))
        self._ck(self.lib.fhelin_fc_matmul_ct(self.h, self._harr(rows), len(rows), w.h, slots, padding, outs))
        return self._cts(outs, len(rows))

    def matmulRElarge(self, rows, weights, bias, mask_val=1.0):
        outs = self._outs(len(rows))
        self._ck(self.lib.fhelin_fc_matmulRElarge(self.h, self._harr(rows), len(rows), self._harr(weights), len(weights),
                                                  bias.h if bias else None, float(mask_val), outs))
        return self._cts(outs, len(rows))

    def matmulCRlarge(self, rows, weights, bias):
        flat = [c for r in rows for c in r]
        outs = self._outs(len(rows))
        self._ck(self.lib.fhelin_fc_matmulCRlarge(self.h, self._harr(flat), len(rows), self._harr(weights), bias.h if bias else None, outs))
        return self._cts(outs, len(rows))

    def matmulScores(self, queries, key):
        h = C.c_void_p()
        self._ck(self.lib.fhelin_fc_matmulScores(self.h, self._harr(queries), len(queries), key.h, C.byref(h)))
        return Ct(self, h)

    def wrapUpRepeated(self, v):
        h = C.c_void_p()
        self._ck(self.lib.fhelin_fc_wrapUpRepeated(self.h, self._harr(v), len(v), C.byref(h)))
        return Ct(self, h)

    def wrapUpExpanded(self, v):
        h = C.c_void_p()
        self._ck(self.lib.fhelin_fc_wrapUpExpanded(self.h, self._harr(v), len(v), C.byref(h)))
        return Ct(self, h)

    def unwrapExpanded(self, c, n):
        outs = self._outs(n)
        self._ck(self.lib.fhelin_fc_unwrapExpanded(self.h, c.h, n, outs))
        return self._cts(outs, n)

    def unwrapScoresExpanded(self, c, n):
        outs = self._outs(n)
        self._ck(self.lib.fhelin_fc_unwrapScoresExpanded(self.h, c.h, n, outs))
        return self._cts(outs, n)

    def unwrap_512_in_4_128(self, c, index):
        outs = self._outs(4)
        self._ck(self.lib.fhelin_fc_unwrap_512_in_4_128(self.h, c.h, index, outs))
        return self._cts(outs, 4)

    def unwrapRepeatedLarge(self, containers, input_number):
        outs = self._outs(4 * input_number)
        self._ck(self.lib.fhelin_fc_unwrapRepeatedLarge(self.h, self._harr(containers), len(containers), input_number, outs))
        flat = self._cts(outs, 4 * input_number)
        return [flat[4 * i: 4 * i + 4] for i in range(input_number)]

    def unwrapRepeatedLarge_range(self, containers, input_number, first, count):
        outs = self._outs(4 * count)
        self._ck(self.lib.fhelin_fc_unwrapRepeatedLarge_range(self.h, self._harr(containers), len(containers), input_number, first, count, outs))
        flat = self._cts(outs, 4 * count)
        return [flat[4 * i: 4 * i + 4] for i in range(count)]

    def ct_import_device(self, dptr, npoly, ell, deg, scale_hi, scale_lo, slots):
        h = C.c_void_p()
        self._ck(self.lib.fhelin_ct_import_device(self.h, C.c_void_p(dptr), npoly, ell, deg, scale_hi, scale_lo, slots, C.byref(h)))
        return Ct(self, h)

    # ---- device transport (include/fhelin.h "Device transport")
    FRAME_RAW, FRAME_PACKED = 0, 1
    STREAM_LEGACY = 1     # hipStreamLegacy: names the legacy default stream, whose own handle is 0 (0 / None mean "no stream")

    def frame_bytes(self, cts, format=1):
        """payload bytes of every ciphertext's frame (raw: the words of export(); packed: every limb vector at its modulus width):
        (list of sizes, the largest)"""
        cts = list(cts)
        n = len(cts)
        each = (C.c_size_t * max(n, 1))()
        most = C.c_size_t()
        self._ck(self.lib.fhelin_ct_frame_bytes(self.h, self._harr(cts) if n else None, n, int(format), each, C.byref(most)))
        return list(each[:n]), most.value

    def export_device_many(self, cts, dptr, stride, cap, format=1, stream=None):
        """cts -> the frames dptr + i * stride of one device buffer of `cap` bytes, in one step; returns meta [n, 8] (float64: npoly,
        ell, deg, slots, scale hi, scale lo, payload bytes, format).  stream: a HIP stream handle (torch: stream.cuda_stream) that is
        ordered behind the writes without a host synchronisation (torch's default stream has the handle 0: pass STREAM_LEGACY for
        it); None: one host synchronisation for the whole set"""
        cts = list(cts)
        n = len(cts)
        meta = np.zeros((n, 8), dtype=np.float64)
        self._ck(self.lib.fhelin_ct_export_device_many(self.h, self._harr(cts) if n else None, n, int(format), C.c_void_p(dptr), int(stride),
                                                       int(cap), meta.ctypes.data_as(C.POINTER(C.c_double)),
                                                       C.c_void_p(stream) if stream else None))
        return meta

    def import_device_many(self, dptr, stride, meta, check=False, stream=None):
        """the frames export_device_many wrote (meta [n, 8]) -> n handles, all or nothing; one allocation per (npoly, ell).  check: also
        the range check residue < modulus (one host synchronisation).  stream: the stream whose work produced the frames; the import is
        ordered behind it, and it behind the import, without a host synchronisation"""
        m = np.ascontiguousarray(meta, dtype=np.float64).reshape(-1, 8)
        n = m.shape[0]
        outs = self._outs(n)
        self._ck(self.lib.fhelin_ct_import_device_many(self.h, C.c_void_p(dptr), int(stride), m.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                       1 if check else 0, C.c_void_p(stream) if stream else None, outs))
        return self._cts(outs, n)

    def sync_count(self):
        """host synchronisations of this context so far (test hook)"""
        n = C.c_uint64()
        self._ck(self.lib.fhelin_debug_sync_count(self.h, C.byref(n)))
        return n.value

    def generate_containers(self, inputs, bias=None):
        cap = (len(inputs) + 31) // 32
        outs = self._outs(cap)
        n = C.c_int32()
        self._ck(self.lib.fhelin_fc_generate_containers(self.h, self._harr(inputs), len(inputs), bias.h if bias else None, outs, C.byref(n)))
        return self._cts(outs, n.value)

    def wrap_containers(self, v, inputs_number):
        h = C.c_void_p()
        self._ck(self.lib.fhelin_fc_wrap_containers(self.h, self._harr(v), len(v), inputs_number, C.byref(h)))
        return Ct(self, h)


    # ---- the composite calls on a batch of samples (include/fhelin.h fhelin_fcb_*): flat handle lists are sample-major
    def fcb_matmulScores(self, queries, n, keys):
        """queries: B*n handles (sample-major), keys: B handles -> B handles"""
        outs = self._outs(len(keys))
        self._ck(self.lib.fhelin_fcb_matmulScores(self.h, self._harr(queries), n, self._harr(keys), len(keys), outs))
        return self._cts(outs, len(keys))

    def fcb_matmul_ct(self, rows, ws, slots, padding):
        outs = self._outs(len(rows))
        self._ck(self.lib.fhelin_fcb_matmul_ct(self.h, self._harr(rows), self._harr(ws), len(rows), slots, padding, outs))
        return self._cts(outs, len(rows))

    def fcb_wrapUpRepeated(self, v, n, B):
        outs = self._outs(B)
        self._ck(self.lib.fhelin_fcb_wrapUpRepeated(self.h, self._harr(v), n, B, outs))
        return self._cts(outs, B)

    def fcb_wrapUpExpanded(self, v, n, B):
        outs = self._outs(B)
        self._ck(self.lib.fhelin_fcb_wrapUpExpanded(self.h, self._harr(v), n, B, outs))
        return self._cts(outs, B)

    def fcb_unwrapExpanded(self, cs, n):
        outs = self._outs(len(cs) * n)
        self._ck(self.lib.fhelin_fcb_unwrapExpanded(self.h, self._harr(cs), len(cs), n, outs))
        return self._cts(outs, len(cs) * n)

    def fcb_unwrapRepeatedLarge(self, containers, nc, B, input_number):
        outs = self._outs(B * input_number * 4)
        self._ck(self.lib.fhelin_fcb_unwrapRepeatedLarge(self.h, self._harr(containers), nc, B, input_number, outs))
        return self._cts(outs, B * input_number * 4)

    def fcb_generate_containers(self, inputs, n, B, bias=None):
        per = (n + 31) // 32
        outs = self._outs(B * per)
        k = C.c_int32()
        self._ck(self.lib.fhelin_fcb_generate_containers(self.h, self._harr(inputs), n, B, bias.h if bias else None, outs, C.byref(k)))
        return self._cts(outs, B * k.value), k.value

    def rotsum_batch(self, v, slots, padding, repeat=False):
        return self._rows(self.lib.fhelin_fc_rotsum_batch, v, len(v), slots, padding, 1 if repeat else 0)

    def add_plain_batch(self, v, pt):
        return self._rows(self.lib.fhelin_add_plain_batch, v, len(v), pt.h)

    def eval_poly_batch(self, xs, coeffs):
        cf = np.ascontiguousarray(coeffs, dtype=np.float64)
        return self._rows(self.lib.fhelin_eval_poly_batch, xs, len(xs), cf.ctypes.data_as(C.POINTER(C.c_double)), cf.size)

    def mult_many_batch(self, v, n, B):
        outs = self._outs(B)
        self._ck(self.lib.fhelin_mult_many_batch(self.h, self._harr(v), n, B, outs))
        return self._cts(outs, B)


class Pt:
    def __init__(self, eng, h):
        self.eng, self.h = eng, h

    def free(self):
        if self.h and self.eng.h:
            self.eng.lib.fhelin_pt_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
        self.h = None


class LinearTransform:
    """a linear-transform plan (fhelin_lt): host data, usable on the engine that made it"""

    def __init__(self, eng, h):
        self.eng, self.h = eng, h

    def info(self):
        i = [C.c_int32() for _ in range(4)]
        self.eng._ck(self.eng.lib.fhelin_lt_info(self.h, *[C.byref(x) for x in i]))
        return dict(n1=i[0].value, n2=i[1].value, n_terms=i[2].value, slots=i[3].value)

    def encoding_bytes(self):
        """device bytes of the limb-sliced encodings the plan's plaintexts hold: (ell + k) N 8 per (term, distinct (ell, scale) applied at)"""
        b = C.c_uint64()
        self.eng._ck(self.eng.lib.fhelin_lt_encoding_bytes(self.h, C.byref(b)))
        return b.value

    def rotations(self):
        """the rotation indices whose keys fhelin_lt_apply needs"""
        n = C.c_int32()
        self.eng._ck(self.eng.lib.fhelin_lt_rotations(self.h, None, 0, C.byref(n)))
        out = (C.c_int32 * max(n.value, 1))()
        self.eng._ck(self.eng.lib.fhelin_lt_rotations(self.h, out, n.value, C.byref(n)))
        return [out[i] for i in range(n.value)]

    def free(self):
        if self.h and self.eng.h:
            self.eng.lib.fhelin_lt_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
        self.h = None


class Ct:
    def __init__(self, eng, h):
        self.eng, self.h = eng, h

    def info(self):
        i = [C.c_int32() for _ in range(5)]
        sc = C.c_double()
        self.eng._ck(self.eng.lib.fhelin_ct_info(self.h, C.byref(i[0]), C.byref(i[1]), C.byref(i[2]), C.byref(i[3]), C.byref(sc), C.byref(i[4])))
        return dict(npoly=i[0].value, ell=i[1].value, level=i[2].value, deg=i[3].value, scale=sc.value, slots=i[4].value)

    @property
    def slots(self):
        return self.info()["slots"]

    @property
    def level(self):
        return self.info()["level"]

    def export(self):
        inf = self.info()
        out = np.empty((inf["npoly"], inf["ell"], self.eng.N), dtype=np.uint64)
        self.eng._ck(self.eng.lib.fhelin_ct_export(self.eng.h, self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def scale_parts(self):
        hi, lo = C.c_double(), C.c_double()
        self.eng._ck(self.eng.lib.fhelin_ct_scale(self.h, C.byref(hi), C.byref(lo)))
        return hi.value, lo.value

    def wrapped_info(self):
        """a wrapped input ciphertext: dict(count, total, ell = the inputs' limbs, positions)"""
        i = [C.c_int32() for _ in range(3)]
        pos = np.zeros(128, dtype=np.int32)
        self.eng._ck(self.eng.lib.fhelin_wrapped_info(self.h, C.byref(i[0]), C.byref(i[1]), C.byref(i[2]), pos.ctypes.data_as(C.c_void_p), 128))
        return dict(count=i[0].value, total=i[1].value, ell=i[2].value, positions=pos[:i[0].value].tolist())

    def compact_bytes(self):
        n = C.c_size_t()
        self.eng._ck(self.eng.lib.fhelin_ct_compact_bytes(self.h, C.byref(n)))
        return n.value

    def export_compact(self):
        """the compact form (c0, seed, nonce) of an unmodified seeded encryption, as bytes"""
        n = self.compact_bytes()
        out = C.create_string_buffer(n)
        self.eng._ck(self.eng.lib.fhelin_ct_export_compact(self.eng.h, self.h, out, n))
        return out.raw

    def packed_bytes(self, seeded=False):
        n = C.c_size_t()
        self.eng._ck(self.eng.lib.fhelin_ct_packed_bytes(self.eng.h, self.h, 1 if seeded else 0, C.byref(n)))
        return n.value

    def export_packed(self, seeded=False):
        """the packed blob (include/fhelin.h "Packed formats"): every component (seeded=False), or c0 with seed and nonce of an
        unmodified seeded encryption (seeded=True); bytes"""
        n = self.packed_bytes(seeded)
        out = C.create_string_buffer(n)
        self.eng._ck(self.eng.lib.fhelin_ct_export_packed(self.eng.h, self.h, 1 if seeded else 0, out, n))
        return out.raw

    def export_device(self, dptr, cap_words):
        self.eng._ck(self.eng.lib.fhelin_ct_export_device(self.eng.h, self.h, C.c_void_p(dptr), cap_words))

    def debug_addr(self):
        """test hook: (device address of the residues, of the batch allocation they are a view of or 0)"""
        d, b = C.c_uint64(), C.c_uint64()
        self.eng._ck(self.eng.lib.fhelin_debug_ct_addr(self.h, C.byref(d), C.byref(b)))
        return d.value, b.value

    def clone(self):
        return self.eng._un(self.eng.lib.fhelin_ct_clone, self)

    def free(self):
        if self.h and self.eng.h:
            self.eng.lib.fhelin_ct_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

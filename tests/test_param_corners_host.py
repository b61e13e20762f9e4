"""The parameter layer at every corner Context accepts (host-only contexts, no GPU): the kernels choose their code by the digit
size alpha, the digit count beta, the number of special primes k and the size of the primes, and their accumulation bounds assume
every modulus below 2^60 (Acc30's 30-bit halves, the Montgomery-finished sums of 16 products).  Every accepted corner must yield
distinct NTT-friendly primes below that bound and report the alpha / beta / k the kernels will be launched with; every parameter
set outside the documented limits (include/fhelin.h) must be refused with FHELIN_ERR_ARG before any prime reaches a kernel."""
import pytest

BOUND = 1 << 60

# (preset, overrides, alpha, beta, k): the corners of tests/test_param_corners_gpu.py and the limits themselves
ACCEPTED = [
    ("toy", dict(n_q=16, dnum=16), 1, 16, 2),                                   # alpha = 1, beta = 16
    ("toy", dict(n_q=16, dnum=1, n_p=16), 16, 1, 16),                           # alpha = 16, k = 16
    ("toy13", dict(n_q=17, dnum=2), 9, 2, 3),                                   # alpha = 9: digits of 9 and 8
    ("toy13", dict(n_q=10, dnum=2, n_p=5), 5, 2, 5),
    ("toy", dict(n_p=1), 2, 3, 1),
    ("toy", dict(n_p=9), 2, 3, 9),
    ("toy", dict(n_q=8, dnum=2, n_p=15), 4, 2, 15),
    ("toy13", dict(n_q=12, scale_bits=53), 4, 3, 3),                            # 53/54-bit primes
    ("toy13", dict(n_q=12, scale_bits=57), 4, 3, 3),                            # 57/58-bit primes
    ("toy", dict(n_q=8, first_bits=60, scale_bits=59), 3, 3, 2),                # 60-bit q0, 59/60-bit scaling primes
    ("toy", dict(n_q=4, dnum=4, first_bits=60, scale_bits=59), 1, 4, 2),        # ... at alpha = 1
    ("toy", dict(n_q=8, first_bits=40, scale_bits=50, special_bits=30, n_p=-1), 3, 3, 5),
    ("toy", dict(n_q=4, n_p=2, dnum=2, first_bits=24, scale_bits=24, special_bits=24), 2, 2, 2),
    ("toy", dict(n_q=16, dnum=16, first_bits=20, scale_bits=20, special_bits=20), 1, 16, 2),   # the smallest primes
    ("toy", dict(log_n=17, log_slots=16), 2, 3, 2),                             # the largest ring
    ("toy", dict(n_p=0), 2, 3, 0),                                              # no key switching
    ("toy", dict(n_q=64, dnum=4, n_p=16), 16, 4, 16),                           # the most limbs
    ("toy", dict(log_n=17, n_q=64, dnum=16, n_p=16, first_bits=60, scale_bits=59, log_slots=16), 4, 16, 16),
    ("reference", dict(n_q=6, n_p=2, dnum=3, first_bits=60, scale_bits=59), 2, 3, 2),
    ("toy", dict(n_q=2, scale_bits=60), 1, 2, 2),      # one scaling prime, the largest below 2^60: the limit is on the primes
    # the chains tests/test_kernel_corners_gpu.py adds
    ("toy", dict(n_q=16, dnum=16, first_bits=60, scale_bits=59), 1, 16, 2),     # 16 digits of 59/60-bit residues
    ("toy", dict(n_q=20, dnum=10), 2, 10, 2),                                   # more than 8 digits with alpha > 1
    ("toy", dict(n_q=8, dnum=8, first_bits=60, scale_bits=59), 1, 8, 2),        # eight digits of 59/60-bit residues
    ("toy", dict(n_p=8), 2, 3, 8),
]

REFUSED = [
    ("toy", dict(n_q=17, dnum=1)),                  # alpha = 17
    ("toy", dict(n_q=17, dnum=17)),                 # beta = 17
    ("toy", dict(n_q=65, dnum=8)),
    ("toy", dict(n_p=17)),
    ("toy", dict(scale_bits=60)),                   # 61-bit scaling primes
    ("toy13", dict(scale_bits=60)),
    ("toy", dict(first_bits=61)),
    ("toy", dict(special_bits=61)),
    ("toy", dict(scale_bits=19)),
    ("toy", dict(log_n=18, log_slots=16)),
    ("toy", dict(log_n=11, log_slots=10)),
]


def _ident(case):
    return "-".join([case[0]] + [f"{k}={v}" for k, v in case[1].items()])


@pytest.mark.parametrize("preset,over,alpha,beta,k", ACCEPTED, ids=[_ident(c) for c in ACCEPTED])
def test_accepted_corner_chain(fa, orc, preset, over, alpha, beta, k):
    """distinct primes = 1 mod 2N below 2^60, and the alpha / beta / k the kernels are launched with"""
    eng = fa.Engine(preset, device=-1, seed=1, **over)
    try:
        mods = [int(m) for m in eng.moduli]
        assert len(mods) == eng.n_q + eng.n_p
        assert len(set(mods)) == len(mods)
        two_n = 2 * eng.N
        for m in mods:
            assert m < BOUND, (m.bit_length(), over)
            assert m % two_n == 1 and orc.is_prime(m), m
        assert (eng.alpha, eng.dnum_digits, eng.n_p) == (alpha, beta, k)
        assert eng.alpha == -(-eng.n_q // eng.params.dnum)
        # the special primes are the largest below 2^special_bits, the first prime below 2^first_bits
        assert all(m < 1 << eng.params.special_bits for m in mods[eng.n_q:])
        assert mods[0] < 1 << eng.params.first_bits
    finally:
        eng.close()


def test_sixty_bit_chain_reaches_both_sides_of_two_to_59(fa):
    """the chain the GPU corner p60 runs: a 60-bit q0 and scaling primes above and below 2^59, all below 2^60"""
    eng = fa.Engine("toy", device=-1, seed=1, n_q=8, first_bits=60, scale_bits=59)
    try:
        q = [int(x) for x in eng.q]
        assert q[0].bit_length() == 60
        assert any(x >= 1 << 59 for x in q[1:]) and any(x < 1 << 59 for x in q[1:])
    finally:
        eng.close()


@pytest.mark.parametrize("preset,over", REFUSED, ids=[_ident(c) for c in REFUSED])
def test_refused_parameters(fa, preset, over):
    with pytest.raises(fa.FhelinError) as ei:
        fa.Engine(preset, device=-1, seed=1, **over)
    assert ei.value.code == 1, str(ei.value)

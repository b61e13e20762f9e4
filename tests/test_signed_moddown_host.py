"""The identity behind the gathered plain rotation (KsShape::gather), restated over the oracle's transforms in numpy and
Python integers.  A rotation applies its automorphism sigma_g LAST today: out = sigma_g(NTT_q(conv(INTT_p(accP)))).  The gathered form
applies it to the accumulator (pointwise in the evaluation domain), so the ModDown sees INTT_p(sigma_g(accP)) = sigma_g of the old
coefficient vector: the same values at permuted positions, NEGATED where the exponent wraps.  The fast basis conversion does not commute
with that negation (conv(p - x) = -conv(x) + k [P]_t), so moddown_conv_kernel<., SIGNED> un-negates its sources at the negated positions

    s(n) = ((g^-1 mod 2N) * n mod 2N) >= N,

converts, and negates the result.  Checked here: that form equals today's on every residue, for several Galois elements including
2N - 1 (conjugation), with zero coefficients planted at negated positions (x ? p - x : 0); and the conversion WITHOUT the sign
handling differs, so that the test cannot pass vacuously."""
import numpy as np
import pytest

LOG_N = 10
N = 1 << LOG_N
ROTATIONS = [1, 5, -3, 128, -1]


@pytest.fixture(scope="module")
def ring(orc):
    q, p = orc.prime_chain(LOG_N, 4, 55, 52, 3, 60)
    psi_q = [orc.min_root(int(m), 2 * N) for m in q]
    psi_p = [orc.min_root(int(m), 2 * N) for m in p]
    return [int(m) for m in q], [int(m) for m in p], psi_q, psi_p


def _conv(coef_p, q, p):
    """fast basis conversion P -> Q of coefficient vectors [k][N]: sum_p [x_p (P/p)^-1]_p (P/p) mod q_t, exact integers"""
    P = 1
    for m in p:
        P *= m
    y = [[int(x) * pow(P // m, -1, m) % m for x in row] for row, m in zip(coef_p, p)]
    out = np.zeros((len(q), N), dtype=np.uint64)
    for t, qt in enumerate(q):
        hat = [P // m % qt for m in p]
        out[t] = [sum(y[i][n] * hat[i] for i in range(len(p))) % qt for n in range(N)]
    return out


def _signs(g):
    gi = pow(g, -1, 2 * N)
    return np.array([(gi * n) % (2 * N) >= N for n in range(N)])


def _flip(rows, moduli, s):
    """x -> (x ? m - x : 0) where s, per limb"""
    out = np.array(rows, dtype=np.uint64).copy()
    for row, m in zip(out, moduli):
        neg = np.where(row == 0, np.uint64(0), np.uint64(m) - row)
        row[s] = neg[s]
    return out


def _case(orc, ring, g, plant_zeros):
    q, p, psi_q, psi_p = ring
    acc = np.stack([orc.uniform_residues(77 + 13 * i + g, [m], N)[0] for i, m in enumerate(p)])     # accP, NTT form
    s = _signs(g)
    if plant_zeros:
        # zero COEFFICIENTS at negated positions of the rotated vector: position n of sigma_g(x) holds -x[g^-1 n]
        coef = np.stack([orc.ntt_inverse(acc[i], p[i], psi_p[i]) for i in range(len(p))])
        gi = pow(g, -1, 2 * N)
        for n in np.flatnonzero(s)[::3]:
            coef[:, (gi * int(n)) % N] = 0
        acc = np.stack([orc.ntt_forward(coef[i], p[i], psi_p[i]) for i in range(len(p))])
    coef = np.stack([orc.ntt_inverse(acc[i], p[i], psi_p[i]) for i in range(len(p))])
    # today: the automorphism last
    conv = _conv(coef, q, p)
    A = np.stack([orc.automorph_ntt(orc.ntt_forward(conv[t], q[t], psi_q[t]), g) for t in range(len(q))])
    # gathered: the automorphism on the accumulator
    rot = np.stack([orc.automorph_ntt(acc[i], g) for i in range(len(p))])
    rcoef = np.stack([orc.ntt_inverse(rot[i], p[i], psi_p[i]) for i in range(len(p))])
    for i in range(len(p)):
        assert np.array_equal(rcoef[i], orc.automorph_coeff(coef[i], g, p[i]))
    assert np.array_equal(rcoef[:, s], _flip(coef, p, np.ones(N, bool))[:, [(pow(g, -1, 2 * N) * int(n)) % N for n in np.flatnonzero(s)]])
    if plant_zeros:
        assert (rcoef[:, s] == 0).any()
    signed = _flip(_conv(_flip(rcoef, p, s), q, p), q, s)
    B = np.stack([orc.ntt_forward(signed[t], q[t], psi_q[t]) for t in range(len(q))])
    plain = _conv(rcoef, q, p)
    C = np.stack([orc.ntt_forward(plain[t], q[t], psi_q[t]) for t in range(len(q))])
    return A, B, C, signed, plain, s


@pytest.mark.parametrize("plant_zeros", [False, True])
@pytest.mark.parametrize("rot", ROTATIONS + ["conj"])
def test_signed_conversion_commutes_with_the_automorphism(orc, ring, rot, plant_zeros):
    g = 2 * N - 1 if rot == "conj" else orc.galois(LOG_N, rot)
    A, B, C, signed, plain, s = _case(orc, ring, g, plant_zeros)
    assert A.dtype == B.dtype and A.shape == B.shape and A.tobytes() == B.tobytes()
    # without the sign handling the conversion is a different function: it differs at negated positions, and only there
    assert not np.array_equal(A, C)
    diff = (signed != plain).any(axis=0)
    assert diff.any() and not diff[~s].any()

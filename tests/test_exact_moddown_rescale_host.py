"""The identity behind the exact merged tail of a relinearised product that is rescaled right away (DESIGN.md 6g,
Evaluator::moddown_rescale_exact), restated over the oracle's transforms in numpy and Python integers.

The unmerged sequence computes, in NTT form, with conv = conv(INTT(accP)) the fast basis conversion P -> Q,

    y_t   = f ((accQ_t - NTT(conv_t)) P^-1 + d_t) + c_t - s_t             all ell limbs       (ModDown, affine step)
    out_t = (y_t - NTT(lift_t(INTT(y_top)))) q_top^-1                     t < ell - 1         (rescale, centred lift)

The merged tail forms X_t = f accQ_t + P (f d_t + c_t - s_t) and

    x_top = (INTT(X_top) - f conv_top) P^-1  mod q_top                    == INTT(y_top)
    out_t = (X_t - NTT(f conv_t + [P]_t lift_t(x_top))) (P q_top)^-1      == the rescale's out_t

with ONE inverse transform (special limbs + top limb) and ONE forward transform.  Checked here: both equalities on every residue, for
f in {1, 2}, with a constant, with a subtrahend, with both and with neither; and that converting f accP instead of scaling conv gives
DIFFERENT residues (the conversion does not commute with f), so that the test cannot pass vacuously."""
import numpy as np
import pytest

LOG_N = 10
N = 1 << LOG_N
ELL, K = 5, 3


@pytest.fixture(scope="module")
def ring(orc):
    q, p = orc.prime_chain(LOG_N, ELL, 55, 52, K, 60)
    psi_q = [orc.min_root(int(m), 2 * N) for m in q]
    psi_p = [orc.min_root(int(m), 2 * N) for m in p]
    return [int(m) for m in q], [int(m) for m in p], psi_q, psi_p


def _ints(row):
    return [int(v) for v in row]


def _u64(rows):
    return np.array(rows, dtype=np.uint64)


def _conv(coef_p, q, p):
    """fast basis conversion P -> Q of coefficient vectors [k][N]: sum_p [x_p (P/p)^-1]_p (P/p) mod q_t, exact integers"""
    P = 1
    for m in p:
        P *= m
    y = [[x * pow(P // m, -1, m) % m for x in row] for row, m in zip(coef_p, p)]
    return [[sum(y[i][n] * (P // p[i] % qt) for i in range(len(p))) % qt for n in range(N)] for qt in q]


def _fwd(orc, row, m, psi):
    return _ints(orc.ntt_forward(np.array(row, dtype=np.uint64), m, psi))


def _inv(orc, row, m, psi):
    return _ints(orc.ntt_inverse(np.array(row, dtype=np.uint64), m, psi))


def _lift(x_top, q_top, qt):
    """the rescale's centred lift of a coefficient modulo q_top into q_t"""
    return [(x - q_top if x > q_top // 2 else x) % qt for x in x_top]


def _inputs(orc, ring, seed):
    q, p, _, _ = ring
    accQ = [_ints(orc.uniform_residues(seed + 3 * t, [m], N)[0]) for t, m in enumerate(q)]
    accP = [_ints(orc.uniform_residues(seed + 100 + 3 * i, [m], N)[0]) for i, m in enumerate(p)]
    d = [_ints(orc.uniform_residues(seed + 200 + 3 * t, [m], N)[0]) for t, m in enumerate(q)]
    s = [_ints(orc.uniform_residues(seed + 300 + 3 * t, [m], N)[0]) for t, m in enumerate(q)]
    return accQ, accP, d, s


def _unmerged(orc, ring, accQ, conv, d, f, c, s):
    q, p, psi_q, _ = ring
    P = 1
    for m in p:
        P *= m
    y = []
    for t, qt in enumerate(q):
        nc = _fwd(orc, conv[t], qt, psi_q[t])
        pinv = pow(P, -1, qt)
        y.append([(f * ((accQ[t][n] - nc[n]) * pinv + d[t][n]) + c[t] - s[t][n]) % qt for n in range(N)])
    top = ELL - 1
    x_top = _inv(orc, y[top], q[top], psi_q[top])
    out = []
    for t in range(top):
        nl = _fwd(orc, _lift(x_top, q[top], q[t]), q[t], psi_q[t])
        qinv = pow(q[top], -1, q[t])
        out.append([(y[t][n] - nl[n]) * qinv % q[t] for n in range(N)])
    return x_top, out


def _merged(orc, ring, accQ, conv, d, f, c, s, scale_conv=True):
    """scale_conv: f * conv(accP) (the tail); else conv as given is already the conversion of f * accP (the WRONG order)"""
    q, p, psi_q, _ = ring
    P = 1
    for m in p:
        P *= m
    X = [[(f * accQ[t][n] + P * (f * d[t][n] + c[t] - s[t][n])) % qt for n in range(N)] for t, qt in enumerate(q)]
    g = f if scale_conv else 1
    top = ELL - 1
    xc = _inv(orc, X[top], q[top], psi_q[top])
    pinv = pow(P, -1, q[top])
    x_top = [(xc[n] - g * conv[top][n]) * pinv % q[top] for n in range(N)]
    out = []
    for t in range(top):
        qt = q[t]
        lift = _lift(x_top, q[top], qt)
        z = [(g * conv[t][n] + P % qt * lift[n]) % qt for n in range(N)]
        nz = _fwd(orc, z, qt, psi_q[t])
        minv = pow(P * q[top], -1, qt)
        out.append([(X[t][n] - nz[n]) * minv % qt for n in range(N)])
    return x_top, out


@pytest.mark.parametrize("with_sub", [False, True])
@pytest.mark.parametrize("with_const", [False, True])
@pytest.mark.parametrize("f", [1, 2])
def test_merged_tail_equals_moddown_affine_rescale(orc, ring, f, with_const, with_sub):
    q, p, psi_q, psi_p = ring
    accQ, accP, d, s = _inputs(orc, ring, 1000 * f + 10 * with_const + with_sub)
    if not with_sub:
        s = [[0] * N for _ in q]
    # the constant of add_real: one integer (here -1 at a 2^104 scale) modulo every limb
    c = [(-(1 << 104)) % qt if with_const else 0 for qt in q]
    coefP = [_inv(orc, accP[i], p[i], psi_p[i]) for i in range(K)]
    conv = _conv(coefP, q, p)
    x_a, out_a = _unmerged(orc, ring, accQ, conv, d, f, c, s)
    x_b, out_b = _merged(orc, ring, accQ, conv, d, f, c, s)
    assert x_a == x_b                                   # the same coefficients enter the same centred lift
    A, B = _u64(out_a), _u64(out_b)
    assert A.dtype == B.dtype and A.shape == B.shape == (ELL - 1, N) and A.tobytes() == B.tobytes()
    # the lift is centred on both sides: both halves of the range occur
    assert any(x > q[-1] // 2 for x in x_a) and any(x <= q[-1] // 2 for x in x_a)


def test_converting_the_scaled_accumulator_is_a_different_function(orc, ring):
    """conv(INTT(2 accP)) = 2 conv(INTT(accP)) - e P, e = the number of sources that wrap when doubled: with the factor applied to the
    conversion's SOURCES the conversion's residues and the top limb's coefficients (x_top + e) differ, and the outputs differ wherever
    x_top + e crosses q_top / 2 - the centred lift then wraps.  Such coefficients are planted (x_top = floor(q_top / 2) where e >= 1):
    the tail's order still equals the unmerged sequence there, the other order does not."""
    q, p, psi_q, psi_p = ring
    accQ, accP, d, s = _inputs(orc, ring, 4242)
    c = [(-(1 << 104)) % qt for qt in q]
    P = 1
    for m in p:
        P *= m
    top = ELL - 1
    coefP = [_inv(orc, accP[i], p[i], psi_p[i]) for i in range(K)]
    conv = _conv(coefP, q, p)
    conv2 = _conv([[2 * x % m for x in row] for row, m in zip(coefP, p)], q, p)
    assert conv2 != [[2 * x % qt for x in row] for row, qt in zip(conv, q)]
    wraps = [n for n in range(N) if conv2[top][n] != 2 * conv[top][n] % q[top]]
    assert len(wraps) > N // 2
    # plant: change accQ_top by NTT(delta) so that x_top[n] = floor(q_top / 2) at every third wrapping coefficient
    x_now, _ = _unmerged(orc, ring, accQ, conv, d, 2, c, s)
    planted = wraps[::3]
    half_inv = pow(2, -1, q[top])
    delta = [0] * N
    for n in planted:
        delta[n] = (q[top] // 2 - x_now[n]) * P * half_inv % q[top]     # x_top = (INTT(2 accQ_top + ...) - 2 conv_top) P^-1
    nd = _fwd(orc, delta, q[top], psi_q[top])
    accQ[top] = [(a + b) % q[top] for a, b in zip(accQ[top], nd)]
    x_a, out_a = _unmerged(orc, ring, accQ, conv, d, 2, c, s)
    assert all(x_a[n] == q[top] // 2 for n in planted)
    x_b, out_b = _merged(orc, ring, accQ, conv, d, 2, c, s)
    assert x_b == x_a and _u64(out_b).tobytes() == _u64(out_a).tobytes()
    x_w, out_w = _merged(orc, ring, accQ, conv2, d, 2, c, s, scale_conv=False)
    assert x_w != x_a
    assert _u64(out_w).tobytes() != _u64(out_a).tobytes()

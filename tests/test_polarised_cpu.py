"""The element-scaled metric on polarised states discriminates (tests/floors.py; no GPU).

tests/test_gpu_polarised.py bounds every density and gradient kernel by RATIO x the floor of the
reference's algorithm in `floors.elemrel` on near-product states.  Here, on the same states:
the floor itself stays inside the primitives' tolerance; a density that forms rho00 as
(power - rho11) in build precision — what k_dens1 did — lands at least 1e3 floors out in
elemrel, while normrel of the same result passes the usual bound (why the old metric was
blind); and the guard against denormal amplitudes fires."""
import numpy as np
import pytest

import floors as F
from oracle import oracle as O
from oracle.cref import CRefOps

TOL = {"f32": 1e-5, "f64": 1e-12}  # tests/test_gpu_primitives.py
REAL = {"f32": np.float32, "f64": np.float64}


def calls(n, which):
    """The q1 / q2 calls of tests/test_gpu_polarised.py: every position; the 27 pairs of
    test_gpu_primitives that exist at n, and the structured ones."""
    from test_gpu_primitives import q2_positions
    base = [p for p in q2_positions(np.random.default_rng(7)) if max(p) < n]
    return F.primitive_calls(range(n), base + F.structured_pairs(n, which))


def emulate_power_minus_rho11(psi, pos, real, block=4096):
    """get_q1_density with rho00 = power - rho11 per block of amplitudes, every sum and the
    subtraction in `real` (the blocks' partials summed in `real` too); rho01 and rho11 summed
    directly."""
    n = O.qubits_of(psi.size)
    s = psi.reshape(1 << (n - pos - 1), 2, 1 << pos)
    # blocks of whole (0, 1) pairs of the measured qubit
    x0, x1 = (s[:, b, :].reshape(-1) for b in (0, 1))
    nb = max(1, x0.size * 2 // block)
    p00 = p11 = real(0)
    c01 = np.complex128(0)
    for a0, a1 in zip(np.split(x0, nb), np.split(x1, nb)):
        sq = lambda v: (v.real.astype(real) ** 2 + v.imag.astype(real) ** 2)
        pw = np.sum(np.concatenate([sq(a0), sq(a1)]), dtype=real)
        r11 = np.sum(sq(a1), dtype=real)
        p11 = real(p11 + r11)
        p00 = real(p00 + real(pw - r11))
        c01 += np.vdot(a1.astype(np.complex128), a0.astype(np.complex128))
    return np.array([p00, c01, np.conj(c01), p11], np.complex128)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [12, 17])
@pytest.mark.parametrize("which", [0, 1])
def test_reference_floor_is_inside_the_primitives_tolerance(prec, n, which):
    fl = F.primitive_floors(prec, n, which, calls(n, which))
    assert set(fl) == set(F.KINDS)
    for kind, v in fl.items():
        print(f"[floor-elem] cref {prec} n={n} set {which} {kind}: floor {v:.3e}  tol {TOL[prec]:.0e}")
    assert all(v <= TOL[prec] for v in fl.values()), fl


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [12, 17])
@pytest.mark.parametrize("phases", F.PHASES)
def test_power_minus_rho11_is_caught_by_elemrel_and_missed_by_normrel(prec, n, phases):
    which = 0
    ops = CRefOps(prec)
    floor = F.primitive_floors(prec, n, which, calls(n, which))["q1dens"]
    f, _ = F.polarised_pair(prec, n, which, phases)
    f64 = f.astype(np.complex128)
    for pos in F.polarised_sets(n)[which]["near_one"]:  # rho00 = small there
        want = F.exact(O.get_q1_density, f64, pos)
        got = emulate_power_minus_rho11(f, pos, REAL[prec])
        err = F.elemrel(got, want, F.density_scale(f64, [pos]))
        nfloor = F.normrel(ops.get_q1_density(f, pos), want)
        nerr = F.normrel(got, want)
        print(f"[floor-elem] emulated power - rho11 {prec} n={n} {phases} pos={pos}: "
              f"elemrel {err:.3e} = {err / floor:.1e} floors ({floor:.3e}); "
              f"normrel {nerr:.3e} floor {nfloor:.3e}")
        assert want[0].real < 2 * F.SMALL[prec]
        assert err >= 1e3 * floor, (err, floor)
        assert nerr <= F.RATIO * nfloor + F.ATOL[prec], (nerr, nfloor)


def test_denormal_guard_fires_on_six_polarised_qubits():
    with pytest.raises(AssertionError, match="polarised state holds"):
        F.polarised_state(12, F.SMALL["f32"], (0, 1, 2, 3), (4, 5), "product", 0, "f32")
    # three are fine in both precisions
    for prec in ("f32", "f64"):
        psi = F.polarised_state(12, F.SMALL[prec], (0, 11), (5,), "random", 0, prec)
        assert abs(np.linalg.norm(psi) - 1) < 1e-12
        rho = O.get_q1_density(psi, 0)
        assert abs(rho[0].real / F.SMALL[prec] - 1) < 0.05, rho
        rho = O.get_q1_density(psi, 5)
        assert abs(rho[3].real / F.SMALL[prec] - 1) < 0.05, rho

"""Shared-footprint Pauli layers in a differentiable circuit (DenseCircuit.add_const_pauli_xlayer /
add_var_pauli_xlayer / add_const_pauli_xevolution / add_var_pauli_xevolution / add_const_excitation
/ add_var_excitation, quantum_differentiable_circuit/dense_circuit.py) over qdc_pauli_xlayer /
qdc_pauli_xlayer_reverse.

Tolerances.  An energy of a normalised state is bounded by A = sum_t |c_t| of its observable, so
two routes agree to TOL A.  The cotangent of weight 1 is bwd = 2 conj(H fwd), ||bwd|| <= 2 A, and a
rotation's gradient is held to TOL 1/2 ||bwd|| ||fwd|| = TOL A (the rotation tests' bound); an
excitation's gradient sum_k c_k dtheta_k to TOL A sum_k |c_k|; each side of a comparison of two
GPU routes gets that bound."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_dense_grad import DT, TOL
from test_gpu_pauli import random_sum

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def strings_of(g):
    """[(coeff, ops)] of a PauliSum, ops as (qubit, letter) pairs."""
    n = g.qubits_number
    out = []
    for c, x, z in g.terms():
        out.append((c, [(q, "Y" if z >> q & 1 else "X") if x >> q & 1 else (q, "Z")
                        for q in range(n) if (x | z) >> q & 1]))
    return out


def half_filled(n):
    """The basis state with the even qubits occupied (value 1)."""
    return sum(1 << q for q in range(0, n, 2))


def excitation_list(n):
    """Singles and doubles out of the half-filled state, footprints low, high and mixed."""
    return [([0], [1]), ([n - 2], [n - 1]), ([0, 2], [1, 3]), ([2], [n - 1]),
            ([0, n - 2], [n - 1, 3]), ([4], [1])]


def number_operator(n):
    from quantum_differentiable_circuit import PauliSum
    return PauliSum(n, [(0.5 * n, "")] + [(-0.5, f"Z{q}") for q in range(n)])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [6, 13])
def test_excitations_against_one_rotation_per_string(prec, n):
    """Singles and doubles as add_var_excitation, with rotations in between, against the same
    circuit with one add_var_pauli_rotation per string (theta_k = theta c_k): the energies, the
    excitations' gradients sum_k c_k dtheta_k, the other gradients."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    rng = np.random.default_rng(3000 + n)
    psi0 = O.random_state(rng, n).astype(DT[prec])
    obs = random_sum(rng, n, 12, top=True)
    a_norm = float(np.abs(obs.coeffs).sum())
    gens = [q.excitation(n, occ, virt) for occ, virt in excitation_list(n)]
    between = ["X0 Z1", f"Y{n - 1}", "Z2 Z3", "X1 Y4", "Y0 Y2", "X5"]
    ca, cb = DenseCircuit(n, prec), DenseCircuit(n, prec)
    ca.set_state_from_vector(psi0)
    cb.set_state_from_vector(psi0)
    var_a, var_b, spans = [], [], []
    for (occ, virt), g, ops in zip(excitation_list(n), gens, between):
        theta, phi = float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2))
        ca.add_var_excitation(occ, virt)
        var_a.append(theta)
        spans.append((len(var_b), g.coeffs))
        for c, s in strings_of(g):
            cb.add_var_pauli_rotation(s)
            var_b.append(theta * c)
        for circ, var in ((ca, var_a), (cb, var_b)):
            circ.add_var_pauli_rotation(ops)
            var.append(phi)
    ca.get_observable_op_with_grad(obs)
    cb.get_observable_op_with_grad(obs)
    assert len(ca.instructions) == 13 and len(cb.instructions) == 7 + sum(len(g) for g in gens)
    (ea,), (eb,) = ca.forward([], var_a), cb.forward([], var_b)
    print(f"{prec} n={n}: energies {ea:.12e} {eb:.12e}")
    assert abs(ea - eb) <= 2 * TOL[prec] * a_norm
    ga, gb = ca.backward([1.0], [], var_a), cb.backward([1.0], [], var_b)
    assert len(ga) == 12 and all(isinstance(g, float) for g in ga)
    for i, (k0, coeffs) in enumerate(spans):
        want = float(np.dot(coeffs, gb[k0:k0 + coeffs.size]))
        bound = 2 * TOL[prec] * a_norm * float(np.abs(coeffs).sum())
        print(f"  excitation {i}: {ga[2 * i]:.6e} against {want:.6e}")
        assert abs(ga[2 * i] - want) <= bound
        assert abs(ga[2 * i + 1] - gb[k0 + coeffs.size]) <= 2 * TOL[prec] * a_norm
    assert max(abs(g) for g in ga[::2]) > 1e-3 * a_norm
    # backward leaves the forward state at the initial state
    back = ca.state.get_cpu_state_copy()
    assert np.linalg.norm(back - psi0) <= 24 * TOL[prec]  # (12 gates each way, each to TOL)


def test_finite_difference_of_the_energy():
    """f64, n = 6: excitations, a variable xlayer and a variable xevolution from a random state;
    the directional derivative of the energy along a random direction in all angles by 8th-order
    central differences with eta = 1e-4 (truncation ~ eta^8, rounding ~ 1e-16 |E| / eta ~ 1e-11)
    against sum dE/dtheta dtheta at 1e-9 (absolute, the gradients are of order one)."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, eta = 6, 1e-4
    rng = np.random.default_rng(3100)
    c = DenseCircuit(n, "f64")
    psi0 = O.random_state(rng, n).astype(np.complex128)
    c.set_state_from_vector(psi0)
    var, pert = [], []
    for occ, virt in excitation_list(n):
        c.add_var_excitation(occ, virt)
        var.append(float(rng.uniform(-2, 2)))
        pert.append(float(rng.standard_normal()))
    lay = ["X0 Y3", "Y0 X3 Z5", "Y0 X3 Z1 Z2", "X0 Y3"]
    c.add_var_pauli_xlayer(lay)
    var.append(rng.uniform(-2, 2, len(lay)))
    pert.append(rng.standard_normal(len(lay)))
    hop = PauliSum(n, [(0.5, "X1 Z2 Z3 X4"), (0.5, "Y1 Z2 Z3 Y4")])
    c.add_var_pauli_xevolution(hop)
    var.append(float(rng.uniform(-2, 2)))
    pert.append(float(rng.standard_normal()))
    c.add_const_pauli_xlayer(["Y2", "Y2 Z0"])
    c.add_const_excitation([5], [3])
    const = [np.array([0.3, -0.8]), 0.6]
    c.get_observable_op_with_grad(random_sum(rng, n, 10, top=True))

    def energy(v):
        (e,) = c.forward(const, v)
        return e

    coeff = {-4: 1 / 280, -3: -4 / 105, -2: 1 / 5, -1: -4 / 5,
             1: 4 / 5, 2: -1 / 5, 3: 4 / 105, 4: -1 / 280}
    ds_fd = sum(w * energy([g + j * eta * p for g, p in zip(var, pert)])
                for j, w in coeff.items()) / eta
    energy(var)
    grads = c.backward([1.0], const, var)
    assert len(grads) == len(var)
    assert grads[6].shape == (4,) and grads[6].dtype == np.float64 and isinstance(grads[7], float)
    ds = sum(float(np.dot(g, p)) for g, p in zip(grads, pert))
    print(f"ds {ds:.12e} ds_fd {ds_fd:.12e} diff {abs(ds - ds_fd):.2e}")
    assert abs(ds - ds_fd) <= 1e-9 and abs(ds) > 1e-2
    assert np.abs(c.state.get_cpu_state_copy() - psi0).max() < 1e-12


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_xlayer_gradients_per_string_and_zeros_before_the_cotangent(prec):
    """A variable xlayer's gradient is the array of its strings' rotation gradients; layers after
    the last differentiable observable get zeros; constant kinds take the constant FIFO."""
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 13
    rng = np.random.default_rng(3200)
    psi0 = O.random_state(rng, n).astype(DT[prec])
    obs = random_sum(rng, n, 12, top=True)
    a_norm = float(np.abs(obs.coeffs).sum())
    lay = ["X0 Y12", "Y0 X12 Z5", "Y0 X12 Z1 Z11", "X0 Y12", "X0 Y12 Z3 Z4 Z5 Z6"]
    th = rng.uniform(-2, 2, len(lay))
    clay, cth = ["Y7 Y8", "X7 X8 Z0", "Y7 Y8 Z12"], np.array([0.4, -1.3, 0.2])
    hop = PauliSum(n, [(0.5, "X1 Z2 Z3 X4"), (0.5, "Y1 Z2 Z3 Y4")])
    ca, cb = DenseCircuit(n, prec), DenseCircuit(n, prec)
    for c in (ca, cb):
        c.set_state_from_vector(psi0)
    ca.add_var_pauli_xlayer(lay)
    ca.add_const_pauli_xlayer(clay)
    ca.add_const_pauli_xevolution(hop)
    ca.add_const_excitation([2], [9])
    ca.get_observable_op_with_grad(obs)
    ca.add_var_pauli_xlayer(lay[:2])
    ca.add_var_excitation([0], [1])
    ca.add_var_pauli_xevolution(hop)
    for s in lay:
        cb.add_var_pauli_rotation(s)
    import quantum_differentiable_circuit as q
    exc = q.excitation(n, [2], [9])
    cangles = list(cth) + [0.7 * c for c in hop.coeffs] + [-0.5 * c for c, _ in strings_of(exc)]
    for s in clay + [s for _, s in strings_of(hop)] + [s for _, s in strings_of(exc)]:
        cb.add_const_pauli_rotation(s)
    cb.get_observable_op_with_grad(obs)
    const_a = [cth, 0.7, -0.5]
    var_a = [th, np.array([0.1, 0.2]), 0.3, 0.4]
    (ea,) = ca.forward(const_a, var_a)
    (eb,) = cb.forward(cangles, list(th))
    assert abs(ea - eb) <= 2 * TOL[prec] * a_norm
    ga = ca.backward([1.0], const_a, var_a)
    gb = cb.backward([1.0], cangles, list(th))
    assert [type(g) for g in ga] == [np.ndarray, np.ndarray, float, float]
    assert ga[0].dtype == np.float64 and ga[0].shape == (len(lay),)
    print(f"{prec}: per-string gradients differ by {np.abs(ga[0] - np.array(gb)).max():.2e}")
    assert np.abs(ga[0] - np.array(gb)).max() <= 2 * TOL[prec] * a_norm
    assert np.abs(ga[0]).max() > 1e-3 * a_norm
    assert np.array_equal(ga[1], np.zeros(2)) and ga[2] == 0.0 and ga[3] == 0.0
    assert np.linalg.norm(ca.state.get_cpu_state_copy() - psi0) <= 14 * TOL[prec]  # 7 each way


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [6, 13])
def test_particle_number_is_conserved(prec, n):
    """From the half-filled basis state every excitation keeps <N> = n_occupied (an energy of
    A = sum |c| = n, held to TOL A per gate)."""
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    rng = np.random.default_rng(3300 + n)
    c = DenseCircuit(n, prec)
    psi = np.zeros(1 << n, DT[prec])
    psi[half_filled(n)] = 1
    c.set_state_from_vector(psi)
    for occ, virt in excitation_list(n):
        c.add_var_excitation(occ, virt)
    c.get_observable_op_with_grad(number_operator(n))
    var = [float(t) for t in rng.uniform(-2, 2, len(excitation_list(n)))]
    (particles,) = c.forward([], var)
    moved = 1.0 - abs(c.state.get_cpu_state_copy()[half_filled(n)]) ** 2
    print(f"{prec} n={n}: <N> = {particles:.12f}, weight moved {moved:.3f}")
    assert abs(particles - (n + 1) // 2) <= len(var) * TOL[prec] * n
    assert moved > 0.1
    grads = c.backward([1.0], [], var)
    assert max(abs(g) for g in grads) <= 2 * TOL[prec] * n  # d<N>/dtheta = 0
    assert np.linalg.norm(c.state.get_cpu_state_copy() - psi) <= 12 * TOL[prec]


def test_fifo_and_size_messages():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 5
    c = DenseCircuit(n, "f64")
    h = PauliSum(n, [(1.0, "X0 X1"), (0.5, "Y0 Y1 Z4")])
    c.add_var_pauli_xlayer(["X0 Y4", "Y0 X4 Z1"])
    c.add_const_pauli_xlayer([[(2, "Y")]])
    c.add_var_pauli_xevolution(h)
    c.add_const_excitation([0], [3])
    c.get_observable_op_with_grad(PauliSum(n, [(1.0, "Z0")]))
    a, b = np.array([0.1, 0.2]), np.array([0.3])
    with pytest.raises(q.PanicException, match="The number of variable gates is less than required."):
        c.forward([b, 0.5], [a])
    with pytest.raises(q.PanicException, match="The number of constant gates is less than required."):
        c.forward([b], [a, 0.4])
    with pytest.raises(q.PanicException, match="Number of variable gates is more than required."):
        c.forward([b, 0.5], [a, 0.4, 0.6])
    with pytest.raises(q.PanicException, match="Number of constant gates is more than required."):
        c.forward([b, 0.5, 0.7], [a, 0.4])
    with pytest.raises(q.PanicException, match="one angle per string"):
        c.forward([b, 0.5], [np.array([0.1]), 0.4])
    with pytest.raises(q.PanicException, match="must be real"):
        c.forward([b, 0.5], [a, 0.4 + 0.1j])
    (e,) = c.forward([b, 0.5], [a, 0.4])
    assert isinstance(e, float)
    with pytest.raises(q.PanicException, match="more than required"):
        c.backward([1.0], [b, 0.5], [0.9, a, 0.4])
    c.forward([b, 0.5], [a, 0.4])
    with pytest.raises(q.PanicException, match="less than required"):
        c.backward([1.0], [b, 0.5], [0.4])
    c.forward([b, 0.5], [a, 0.4])
    grads = c.backward([1.0], [b, 0.5], [a, 0.4])
    assert [type(x) for x in grads] == [np.ndarray, float] and grads[0].dtype == np.float64
    share = "The strings of a layer must share their X/Y positions."
    for add in (c.add_var_pauli_xlayer, c.add_const_pauli_xlayer):
        with pytest.raises(q.PanicException, match="pos is out of the bound."):
            add(["X0", "X0 Z5"])
        with pytest.raises(q.PanicException, match=share):
            add(["X0", "X1"])
        with pytest.raises(q.PanicException, match="The strings of a layer must commute."):
            add(["X0", "Y0"])
        with pytest.raises(q.PanicException, match="The layer has no terms."):
            add([])
    for add in (c.add_var_pauli_xevolution, c.add_const_pauli_xevolution):
        with pytest.raises(q.PanicException, match=share):
            add(PauliSum(n, [(1.0, "X0"), (1.0, "Y1")]))
        with pytest.raises(q.PanicException, match="The strings of a layer must commute."):
            add(PauliSum(n, [(1.0, "X0 X1"), (1.0, "X0 Y1")]))
        with pytest.raises(q.PanicException, match="different sizes"):
            add(PauliSum(n + 1, [(1.0, "X0")]))
        with pytest.raises(q.PanicException, match="The layer has no terms."):
            add(PauliSum(n, []))
        with pytest.raises(TypeError):
            add(["X0"])
    for add in (c.add_var_excitation, c.add_const_excitation):
        with pytest.raises(q.PanicException, match="pos is out of the bound."):
            add([0], [5])
        with pytest.raises(q.PanicException, match="positions must be different."):
            add([0, 1], [1, 2])
    # the diagonal kinds still take Z strings only
    with pytest.raises(q.PanicException, match="a Pauli layer takes Z strings only."):
        c.add_var_pauli_layer(["X0"])
    assert len(c.instructions) == 5
    from quantum_differentiable_circuit import dense_circuit as D
    assert (D.SAMPLE, D.CONST_XLAYER, D.VAR_XLAYER, D.CONST_XEVOL, D.VAR_XEVOL) == (12, 13, 14, 15, 16)


def test_ucc_example_layers_match_one_rotation_per_string():
    """examples/ucc_pauli.py at 8 qubits (4 sites), 1 layer, f64: the build with excitations as
    layers returns the energy, the particle number and the parameter gradient of the build with
    one rotation per string, each to 2 TOL A (A = sum |c| of the Hamiltonian; the generators have
    sum |c_k| = 1)."""
    sys.path.insert(0, str(ROOT / "examples"))
    try:
        ucc = importlib.import_module("ucc_pauli")
    finally:
        sys.path.remove(str(ROOT / "examples"))
    n = 8
    number = ucc.number_operator(n)
    a_norm = float(np.abs(ucc.hamiltonian(n).coeffs).sum())
    c1, gens = ucc.build(n, 1, "f64")
    c2, gens2 = ucc.build(n, 1, "f64", per_string=True)
    assert len(gens) == len(gens2) == 9 and all(abs(np.abs(g.coeffs).sum() - 1) < 1e-15 for g in gens)
    assert len(c1.instructions) == 10 and len(c2.instructions) == 1 + 6 * 2 + 3 * 8
    params = np.random.default_rng(42).normal(size=len(gens))
    e1, g1, p1 = ucc.loss_and_grad(c1, gens, params, number=number)
    e2, g2, p2 = ucc.loss_and_grad(c2, gens, params, per_string=True, number=number)
    print(f"energy {e1:.15e} {e2:.15e}; particles {p1:.12f}; gradient diff {np.abs(g1 - g2).max():.2e}")
    assert abs(e1 - e2) <= 2 * TOL["f64"] * a_norm
    assert np.abs(g1 - g2).max() <= 2 * TOL["f64"] * a_norm
    assert abs(p1 - 4) <= 9 * TOL["f64"] * n and abs(p2 - 4) <= 33 * TOL["f64"] * n
    assert np.abs(g1).max() > 1e-3

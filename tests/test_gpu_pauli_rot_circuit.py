"""Pauli rotations in a differentiable circuit (DenseCircuit.add_const_pauli_rotation /
add_var_pauli_rotation, quantum_differentiable_circuit/dense_circuit.py) over qdc_pauli_rot /
qdc_pauli_rot_reverse."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_pauli import random_sum

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_finite_difference_identity_with_rotations():
    """tests/test_gpu_pauli_circuit.py::test_finite_difference_identity_with_observables with
    rotations: f64, n = 9, seed 42, two layers; each layer holds variable Haar gates with
    k = 1..5, after each of them a variable rotation (a diagonal string, a weight-9 string, one on
    the top qubit, one with three Y's, one more), then a constant rotation and a differentiable
    observable; the first layer also a differentiable 2-qubit density; one more variable rotation
    after the last observable.  Loss = 0.7 E1 - 1.3 E2 + tsallis(densities).  8th-order central
    differences with eta = 1e-6, jointly in the gate perturbations p and the angle perturbations
    dtheta, against sum Re(g . p) + sum dL/dtheta dtheta at relative 1e-9; the trailing rotation's
    gradient is exactly 0.0; backward leaves fwd at the initial state (1e-12)."""
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, eta = 9, 1e-6
    rng = np.random.default_rng(42)
    c = DenseCircuit(n, "f64")
    psi0 = np.zeros(1 << n, np.complex128)
    psi0[0] = 1
    c.set_state_from_vector(psi0)
    place = lambda k: [int(p) for p in rng.permutation(n)[:k]]
    rots = [["Z1 Z6", " ".join("XYZ"[q % 3] + str(q) for q in range(n)), "X8 Z2", "Y0 Y4 Y7", "X3 Y5"],
            ["Z0 Z3 Z8", " ".join("YZX"[q % 3] + str(q) for q in range(n)), "Y8", "Y1 Y2 Z5 Y6", "X0"]]
    var, pert, const = [], [], [0.4, -1.1]
    obs = [random_sum(rng, n, 12, top=True) for _ in range(2)]
    for layer in range(2):
        for k, ops in zip(rng.permutation([1, 2, 3, 4, 5]), rots[layer]):
            c.add_var_gate(place(k))
            var.append(O.haar_unitary(rng, 1 << k))
            pert.append(rng.standard_normal(1 << (2 * k)) + 1j * rng.standard_normal(1 << (2 * k)))
            c.add_var_pauli_rotation(ops)
            var.append(float(rng.uniform(-3, 3)))
            pert.append(float(rng.standard_normal()))
        c.add_const_pauli_rotation(["Y2 X7", [(8, "Z"), (0, "Y")]][layer])
        c.get_observable_op_with_grad(obs[layer])
        if layer == 0:
            c.get_dens_op_with_grad(place(2))
    c.add_var_pauli_rotation("X4 Y8")
    var.append(0.77)
    pert.append(-0.6)
    is_angle = [isinstance(v, float) for v in var]
    assert sum(is_angle) == 11

    def loss(v):
        e1, rho, e2 = c.forward(const, v)
        assert isinstance(e1, float) and isinstance(e2, float) and rho.shape == (4, 4)
        return 0.7 * e1 - 1.3 * e2 + O.tsallis_loss_and_cotangents([rho])[0]

    coeff = {-4: 1 / 280, -3: -4 / 105, -2: 1 / 5, -1: -4 / 5,
             1: 4 / 5, 2: -1 / 5, 3: 4 / 105, 4: -1 / 280}
    ds_fd = sum(w * loss([g + j * eta * p for g, p in zip(var, pert)])
                for j, w in coeff.items()) / eta
    e1, rho, e2 = c.forward(const, var)
    _, cots = O.tsallis_loss_and_cotangents([rho])
    grads = c.backward([0.7, np.ascontiguousarray(cots[0].conj()), -1.3], const, var)
    assert len(grads) == len(var)
    assert [isinstance(g, float) for g in grads] == is_angle
    assert [g.shape for g, a in zip(grads, is_angle) if not a] == \
        [v.shape for v, a in zip(var, is_angle) if not a]
    assert grads[-1] == 0.0
    assert all(g != 0.0 for g, a in zip(grads[:-1], is_angle[:-1]) if a)
    ds = sum(g * p if a else np.tensordot(g, p, axes=1).real
             for g, p, a in zip(grads, pert, is_angle))
    print(f"ds {ds:.12e} ds_fd {ds_fd:.12e} rel {abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)):.2e}")
    assert abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)) < 1e-9
    assert np.abs(c.state.get_cpu_state_copy() - psi0).max() < 1e-12


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_circuit_of_rotations_is_the_calls_by_hand(prec):
    """A circuit of rotations only returns, bit for bit, the energies and dtheta of the same
    sequence issued through apply_pauli_rotation / pauli_energy / pauli_inject /
    pauli_rot_reverse."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 12
    h1 = PauliSum(n, [(1.0, "Z0 Z1"), (-0.5, "X11"), (0.25, "Y3 Y10")])
    h2 = PauliSum(n, [(-1.0, "X0"), (0.7, "Z5 Z11"), (0.2, "")])
    # (kind, ops, angle): v variable, c constant
    seq = [("v", "X0", 0.3), ("v", "Y11", -1.2), ("c", "X3 X10", 0.9), ("v", "Z0 Z1", 2.1),
           ("obs", h1, 0.6), ("v", "Y0 Z4 X11", -0.4), ("c", "Z7", 1.3), ("v", "Y0 X5", 0.8),
           ("obs", h2, -1.7), ("v", "X5", 0.5)]
    c = DenseCircuit(n, prec)
    for kind, ops, _ in seq:
        if kind == "obs":
            c.get_observable_op_with_grad(ops)
        else:
            (c.add_var_pauli_rotation if kind == "v" else c.add_const_pauli_rotation)(ops)
    var = [a for k, _, a in seq if k == "v"]
    const = [np.array([a]) for k, _, a in seq if k == "c"]  # a 1-element array is an angle too
    energies = c.forward(const, var)
    grads = c.backward([a for k, _, a in seq if k == "obs"], const, var)

    fwd = q.QuantizedTensor.new_standard(n, precision=prec)
    want_e = []
    for kind, ops, a in seq:
        if kind == "obs":
            want_e.append(fwd.pauli_energy(ops))
        else:
            fwd.apply_pauli_rotation(ops, a)
    bwd, want_g = None, []
    for kind, ops, a in reversed(seq):
        if kind == "obs":
            if bwd is None:
                bwd = q.QuantizedTensor(n, prec)
                q.pauli_inject(fwd, bwd, ops, a, accumulate=False)
            else:
                q.pauli_inject(fwd, bwd, ops, a, accumulate=True)
        else:
            d = q.pauli_rot_reverse(fwd, bwd, ops, a, want_grad=kind == "v")
            if kind == "v":
                want_g.insert(0, d)
    assert energies == want_e and len(energies) == 2
    assert grads == want_g and len(grads) == 6 and grads[-1] == 0.0
    assert all(isinstance(g, float) for g in grads) and all(abs(g) > 1e-3 for g in grads[:2])
    assert np.array_equal(c.state.get_cpu_state_copy(), fwd.get_cpu_state_copy())
    assert np.array_equal(c.bwd.get_cpu_state_copy(), bwd.get_cpu_state_copy())
    # run() applies the rotations too
    assert c.run(const, var) == want_e


def test_fifo_messages():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 5
    c = DenseCircuit(n, "f64")
    c.add_var_pauli_rotation("X0 Z4")
    c.add_const_pauli_rotation([(2, "Y")])
    c.add_var_gate([1])
    c.add_var_pauli_rotation("Z3")
    c.get_observable_op_with_grad(PauliSum(n, [(1.0, "Z0")]))
    g = O.haar_unitary(np.random.default_rng(1), 2)
    with pytest.raises(q.PanicException, match="The number of variable gates is less than required."):
        c.forward([0.1], [0.2, g])
    with pytest.raises(q.PanicException, match="The number of constant gates is less than required."):
        c.forward([], [0.2, g, 0.3])
    with pytest.raises(q.PanicException, match="Number of variable gates is more than required."):
        c.forward([0.1], [0.2, g, 0.3, 0.4])
    with pytest.raises(q.PanicException, match="Number of constant gates is more than required."):
        c.forward([0.1, 0.5], [0.2, g, 0.3])
    with pytest.raises(q.PanicException, match="must be real"):
        c.forward([0.1], [0.2 + 0.1j, g, 0.3])
    with pytest.raises(q.PanicException, match="must be real"):
        c.forward([np.array([0.1 + 1j])], [0.2, g, 0.3])
    (e,) = c.forward([0.1], [np.float64(0.2), g, np.array(0.3)])
    assert isinstance(e, float)
    with pytest.raises(q.PanicException, match="more than required"):
        c.backward([1.0], [0.1], [0.9, 0.2, g, 0.3])
    c.forward([0.1], [0.2, g, 0.3])
    with pytest.raises(q.PanicException, match="less than required"):
        c.backward([1.0], [0.1], [g, 0.3])
    c.forward([0.1], [0.2, g, 0.3])
    grads = c.backward([1.0], [0.1], [0.2, g, 0.3])
    assert [type(x) for x in grads] == [float, np.ndarray, float]
    for bad in ("X5", [(9, "Z")]):
        with pytest.raises(q.PanicException, match="pos is out of the bound."):
            c.add_var_pauli_rotation(bad)
        with pytest.raises(q.PanicException, match="pos is out of the bound."):
            c.add_const_pauli_rotation(bad)
    with pytest.raises(q.PanicException, match="a qubit appears twice in a Pauli term."):
        c.add_var_pauli_rotation("X1 Z1")
    assert len(c.instructions) == 5


def test_qaoa_example_matches_vqe_example():
    """examples/qaoa_pauli.py against examples/vqe_pauli.py at n = 8, 2 layers, f64, the same
    parameters (theta = 2 g on the bonds, 2 b on the sites): energy within 1e-12, gradient within
    1e-10."""
    sys.path.insert(0, str(ROOT / "examples"))
    try:
        vqe, qaoa = importlib.import_module("vqe_pauli"), importlib.import_module("qaoa_pauli")
    finally:
        sys.path.remove(str(ROOT / "examples"))
    n, layers = 8, 2
    params = np.random.default_rng(42).normal(size=2 * layers)
    e1, g1 = vqe.loss_and_grad(vqe.build(n, layers, "f64"), params, n)
    e2, g2 = qaoa.loss_and_grad(qaoa.build(n, layers, "f64"), params, n)
    print(f"energy {e1:.15e} {e2:.15e}; gradient diff {np.abs(g1 - g2).max():.2e}")
    assert abs(e1 - e2) <= 1e-12
    assert np.abs(g1 - g2).max() <= 1e-10
    assert np.abs(g1).max() > 1e-3

"""Diagonal Pauli layers in a differentiable circuit (DenseCircuit.add_const_pauli_layer /
add_var_pauli_layer / add_const_pauli_evolution / add_var_pauli_evolution,
quantum_differentiable_circuit/dense_circuit.py) over qdc_pauli_layer / qdc_pauli_layer_reverse."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_pauli import random_sum

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_finite_difference_identity_with_layers():
    """tests/test_gpu_pauli_rot_circuit.py's finite-difference test with layers: f64, n = 6, two
    layers of variable Haar gates (k = 1, 2, 3), variable rotations, a variable per-term layer
    and a variable evolution exp(-i theta/2 H), a constant layer and a constant evolution, then a
    differentiable observable; one more variable layer after the last observable.  Loss =
    0.7 E1 - 1.3 E2.  8th-order central differences with eta = 1e-6, jointly in the gate
    perturbations, the rotations' angles, the layers' angles and the evolutions' theta, against
    sum Re(g . p) + sum dL/dtheta dtheta at relative 1e-9; the trailing layer's gradient is
    zeros; backward leaves fwd at the initial state (1e-12)."""
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, eta = 6, 1e-6
    rng = np.random.default_rng(43)
    c = DenseCircuit(n, "f64")
    psi0 = O.random_state(rng, n).astype(np.complex128)
    c.set_state_from_vector(psi0)
    place = lambda k: [int(p) for p in rng.permutation(n)[:k]]
    per_term = [["Z0 Z1", "Z2", "Z1 Z3 Z5", "", "Z0 Z1"], ["Z4 Z5", "Z0 Z1 Z2 Z3 Z4 Z5", "Z3"]]
    ham = [PauliSum(n, [(0.7, "Z0 Z5"), (-1.2, "Z1 Z2"), (0.4, "Z3"), (0.9, "")]),
           PauliSum(n, [(1.0, f"Z{i} Z{(i + 1) % n}") for i in range(n)])]
    rots = [["X0 Y3", "Z2 Z4"], ["Y5", "X1 Z2 Y4"]]
    var, pert, const = [], [], []
    obs = [random_sum(rng, n, 10, top=True) for _ in range(2)]
    for layer in range(2):
        for k, ops in zip((1, 2), rots[layer]):
            c.add_var_gate(place(k + layer))
            var.append(O.haar_unitary(rng, 1 << (k + layer)))
            m = 1 << (2 * (k + layer))
            pert.append(rng.standard_normal(m) + 1j * rng.standard_normal(m))
            c.add_var_pauli_rotation(ops)
            var.append(float(rng.uniform(-3, 3)))
            pert.append(float(rng.standard_normal()))
        c.add_var_pauli_layer(per_term[layer])
        var.append(rng.uniform(-3, 3, len(per_term[layer])))
        pert.append(rng.standard_normal(len(per_term[layer])))
        c.add_const_pauli_layer(["Z1 Z4", "Z0"])
        const.append(np.array([0.4, -1.1]))
        c.add_var_gate(place(2))
        var.append(O.haar_unitary(rng, 4))
        pert.append(rng.standard_normal(16) + 1j * rng.standard_normal(16))
        c.add_var_pauli_evolution(ham[layer])
        var.append(float(rng.uniform(-2, 2)))
        pert.append(float(rng.standard_normal()))
        c.add_const_pauli_evolution(ham[1 - layer])
        const.append(0.3 - layer)
        c.add_var_gate(place(1))
        var.append(O.haar_unitary(rng, 2))
        pert.append(rng.standard_normal(4) + 1j * rng.standard_normal(4))
        c.get_observable_op_with_grad(obs[layer])
    c.add_var_pauli_layer(["Z2 Z3", "Z5"])
    var.append(np.array([0.77, -0.2]))
    pert.append(np.array([-0.6, 0.3]))

    def loss(v):
        e1, e2 = c.forward(const, v)
        return 0.7 * e1 - 1.3 * e2

    coeff = {-4: 1 / 280, -3: -4 / 105, -2: 1 / 5, -1: -4 / 5,
             1: 4 / 5, 2: -1 / 5, 3: 4 / 105, 4: -1 / 280}
    ds_fd = sum(w * loss([g + j * eta * p for g, p in zip(var, pert)])
                for j, w in coeff.items()) / eta
    c.forward(const, var)
    grads = c.backward([0.7, -1.3], const, var)
    assert len(grads) == len(var)
    for g, v in zip(grads, var):
        if isinstance(v, float):
            assert isinstance(g, float) and g != 0.0
        elif v.dtype == np.float64:
            assert g.dtype == np.float64 and g.shape == v.shape
        else:
            assert g.shape == (v.size,)
    assert np.array_equal(grads[-1], np.zeros(2))
    assert all(np.all(g != 0.0) for g, v in zip(grads[:-1], var) if getattr(v, "dtype", None) == np.float64)
    ds = sum(float(np.dot(g, p)) if np.isrealobj(p) else np.tensordot(g, p, axes=1).real
             for g, p in zip(grads, pert))
    print(f"ds {ds:.12e} ds_fd {ds_fd:.12e} rel {abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)):.2e}")
    assert abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)) < 1e-9
    assert np.abs(c.state.get_cpu_state_copy() - psi0).max() < 1e-12


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_circuit_of_layers_is_the_calls_by_hand(prec):
    """A circuit of layers, evolutions and rotations returns, bit for bit, the energies and the
    gradients of the same sequence issued through apply_pauli_layer / pauli_layer_reverse; an
    evolution is the layer with theta_k = theta c_k and the gradient sum_k c_k dtheta_k."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 12
    h1 = PauliSum(n, [(1.0, "Z0 Z1"), (-0.5, "X11"), (0.25, "Y3 Y10")])
    cost = PauliSum(n, [(0.5, f"Z{i} Z{j}") for i in range(n) for j in range(i)] + [(0.2, "")])
    lay = ["Z0 Z11", "Z3", "Z1 Z2 Z10", "Z3"]
    seq = [("rot", "X0", 0.3), ("rot", "Y11", -1.2), ("vlayer", lay, np.array([0.3, -0.7, 1.9, 0.1])),
           ("vevol", cost, 0.45), ("rot", "X5 X6", 0.9), ("clayer", lay[:2], np.array([1.0, 2.0])),
           ("cevol", cost, -0.8), ("obs", h1, 0.6), ("vlayer", lay[1:], np.array([0.5, 0.6, 0.7]))]
    c = DenseCircuit(n, prec)
    add = {"rot": c.add_var_pauli_rotation, "vlayer": c.add_var_pauli_layer,
           "vevol": c.add_var_pauli_evolution, "clayer": c.add_const_pauli_layer,
           "cevol": c.add_const_pauli_evolution, "obs": c.get_observable_op_with_grad}
    for kind, ops, _ in seq:
        add[kind](ops)
    var = [a for k, _, a in seq if k in ("rot", "vlayer", "vevol")]
    const = [a for k, _, a in seq if k in ("clayer", "cevol")]
    energies = c.forward(const, var)
    grads = c.backward([0.6], const, var)

    def layer_of(kind, ops, a):
        if kind.endswith("evol"):
            return ops.zmasks, a * ops.coeffs
        return ops, a

    fwd = q.QuantizedTensor.new_standard(n, precision=prec)
    want_e = []
    for kind, ops, a in seq:
        if kind == "obs":
            want_e.append(fwd.pauli_energy(ops))
        elif kind == "rot":
            fwd.apply_pauli_rotation(ops, a)
        else:
            fwd.apply_pauli_layer(*layer_of(kind, ops, a))
    bwd, want_g = None, []
    for kind, ops, a in reversed(seq):
        if kind == "obs":
            bwd = q.QuantizedTensor(n, prec)
            q.pauli_inject(fwd, bwd, ops, a, accumulate=False)
        elif kind == "rot":
            want_g.insert(0, q.pauli_rot_reverse(fwd, bwd, ops, a))
        else:
            d = q.pauli_layer_reverse(fwd, bwd, *layer_of(kind, ops, a), want_grad=kind[0] == "v")
            if kind == "vlayer":
                want_g.insert(0, d)
            elif kind == "vevol":
                want_g.insert(0, float(np.dot(ops.coeffs, d)))
    assert energies == want_e and len(energies) == 1
    assert len(grads) == len(want_g) == 6
    for g, w in zip(grads, want_g):
        assert type(g) is type(w) and np.array_equal(g, w)
    assert isinstance(grads[3], float) and abs(grads[3]) > 1e-4
    assert grads[2].shape == (4,) and np.all(grads[2] != 0.0) and not grads[-1].any()
    assert np.array_equal(c.state.get_cpu_state_copy(), fwd.get_cpu_state_copy())
    assert np.array_equal(c.bwd.get_cpu_state_copy(), bwd.get_cpu_state_copy())
    assert c.run(const, var) == want_e


def test_fifo_messages():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 5
    c = DenseCircuit(n, "f64")
    h = PauliSum(n, [(1.0, "Z0 Z1"), (0.5, "Z4")])
    c.add_var_pauli_layer(["Z0 Z4", "Z1"])
    c.add_const_pauli_layer([[(2, "Z")]])
    c.add_var_pauli_evolution(h)
    c.add_const_pauli_evolution(h)
    c.get_observable_op_with_grad(PauliSum(n, [(1.0, "X0")]))
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
    for add in (c.add_var_pauli_layer, c.add_const_pauli_layer):
        with pytest.raises(q.PanicException, match="pos is out of the bound."):
            add(["Z0", "Z5"])
        with pytest.raises(q.PanicException, match="a Pauli layer takes Z strings only."):
            add(["Z0", "X1"])
        with pytest.raises(q.PanicException, match="The layer has no terms."):
            add([])
    for add in (c.add_var_pauli_evolution, c.add_const_pauli_evolution):
        with pytest.raises(q.PanicException, match="a Pauli layer takes Z strings only."):
            add(PauliSum(n, [(1.0, "Z0"), (1.0, "Y1")]))
        with pytest.raises(q.PanicException, match="different sizes"):
            add(PauliSum(n + 1, [(1.0, "Z0")]))
        with pytest.raises(q.PanicException, match="The layer has no terms."):
            add(PauliSum(n, []))
        with pytest.raises(TypeError):
            add(["Z0"])
    assert len(c.instructions) == 5


def test_qaoa_example_cost_layer_matches_the_default_build():
    """examples/qaoa_pauli.py at n = 8, 2 layers, f64: build(..., cost_layer=True) returns the
    energy and the parameter gradient of the default build for the same parameters, to 1e-10."""
    sys.path.insert(0, str(ROOT / "examples"))
    try:
        qaoa = importlib.import_module("qaoa_pauli")
    finally:
        sys.path.remove(str(ROOT / "examples"))
    n, layers = 8, 2
    params = np.random.default_rng(42).normal(size=2 * layers)
    e1, g1 = qaoa.loss_and_grad(qaoa.build(n, layers, "f64"), params, n)
    c = qaoa.build(n, layers, "f64", cost_layer=True)
    assert len(c.instructions) == layers * (1 + n) + 1
    e2, g2 = qaoa.loss_and_grad(c, params, n, cost_layer=True)
    print(f"energy {e1:.15e} {e2:.15e}; gradient diff {np.abs(g1 - g2).max():.2e}")
    assert abs(e1 - e2) <= 1e-10
    assert np.abs(g1 - g2).max() <= 1e-10
    assert np.abs(g1).max() > 1e-3

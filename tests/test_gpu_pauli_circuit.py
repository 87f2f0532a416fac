"""Pauli-sum observables in a differentiable circuit (DenseCircuit.get_observable_op[_with_grad],
quantum_differentiable_circuit/dense_circuit.py) over qdc_pauli_energy / qdc_pauli_inject."""
import numpy as np
import pytest

import floors as F
from oracle import oracle as O
from test_gpu_pauli import random_sum

pytestmark = pytest.mark.gpu
DT = F.DT

X = np.array([[0, 1], [1, 0]], np.complex128)
Y = np.array([[0, -1j], [1j, 0]], np.complex128)
Z = np.array([[1, 0], [0, -1]], np.complex128)


def test_finite_difference_identity_with_observables():
    """tests/test_gpu_dense_grad.py::test_dense_circuit_finite_difference_identity with
    observables: f64, n = 9, two layers of variable Haar gates with k = 1..5; after the first
    layer a differentiable observable E1 (12 random strings of weight up to 9, every third on the
    top qubit) and a differentiable 2-qubit density, after the second layer a second observable
    E2.  Loss = 0.7 E1 - 1.3 E2 + tsallis(densities).  The reverse walk meets E2 first (the first
    cotangent: a storing injection into a new bwd), then the density, then E1 (an accumulating
    injection into the existing bwd).  8th-order central differences with eta = 1e-6 against
    sum Re(g . p) at relative 1e-9; backward leaves fwd at the initial state (1e-12)."""
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, eta = 9, 1e-6
    rng = np.random.default_rng(42)
    c = DenseCircuit(n, "f64")
    psi0 = np.zeros(1 << n, np.complex128)
    psi0[0] = 1
    c.set_state_from_vector(psi0)
    place = lambda k: [int(p) for p in rng.permutation(n)[:k]]
    var, pert = [], []
    obs = [random_sum(rng, n, 12, top=True) for _ in range(2)]
    assert all(any((x >> (n - 1)) & 1 for _, x, _ in o.terms()) for o in obs)
    assert max(bin(x | z).count("1") for o in obs for _, x, z in o.terms()) >= 8
    for layer in range(2):
        for k in rng.permutation([1, 2, 3, 4, 5]):
            c.add_var_gate(place(k))
            var.append(O.haar_unitary(rng, 1 << k))
            pert.append(rng.standard_normal(1 << (2 * k)) + 1j * rng.standard_normal(1 << (2 * k)))
        c.get_observable_op_with_grad(obs[layer])
        if layer == 0:
            c.get_dens_op_with_grad(place(2))

    def loss(v):
        e1, rho, e2 = c.forward([], v)
        assert isinstance(e1, float) and isinstance(e2, float) and rho.shape == (4, 4)
        return 0.7 * e1 - 1.3 * e2 + O.tsallis_loss_and_cotangents([rho])[0]

    coeff = {-4: 1 / 280, -3: -4 / 105, -2: 1 / 5, -1: -4 / 5,
             1: 4 / 5, 2: -1 / 5, 3: 4 / 105, 4: -1 / 280}
    ds_fd = sum(w * loss([g + j * eta * p for g, p in zip(var, pert)])
                for j, w in coeff.items()) / eta
    e1, rho, e2 = c.forward([], var)
    _, cots = O.tsallis_loss_and_cotangents([rho])
    grads = c.backward([0.7, np.ascontiguousarray(cots[0].conj()), -1.3], [], var)
    assert [g.shape for g in grads] == [v.shape for v in var]
    ds = sum(np.tensordot(g, p, axes=1).real for g, p in zip(grads, pert))
    print(f"ds {ds:.12e} ds_fd {ds_fd:.12e} rel {abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)):.2e}")
    assert abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)) < 1e-9
    assert np.abs(c.state.get_cpu_state_copy() - psi0).max() < 1e-12


def _density_route_circuit(n, layers, seed):
    """Three layers of 1- and 2-qubit gates, then one DIFF_Q2_DENSITY per bond and one
    DIFF_Q1_DENSITY per site: (ins, const, var, bond/site list in density order)."""
    rng = np.random.default_rng(seed)
    ins, const, var = [], [], []
    for layer in range(layers):
        for p in range(n):
            variable = (p + layer) % 3 != 0
            ins.append((O.VAR_Q1 if variable else O.CONST_Q1, (p,)))
            (var if variable else const).append(O.haar_unitary(rng, 2))
        for p in range(layer % 2, n - 1, 2):
            variable = p % 4 != 1
            ins.append((O.VAR_Q2 if variable else O.CONST_Q2, (p + 1, p)))
            (var if variable else const).append(O.haar_unitary(rng, 4))
    dens = [(k + 1, k) for k in range(n - 1)] + [(k,) for k in range(n)]
    ins += [(O.DIFF_Q2_DENSITY if len(d) == 2 else O.DIFF_Q1_DENSITY, d) for d in dens]
    return ins, const, var, dens


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_same_answer_as_the_density_route(prec):
    """H = sum_k (Z_k Z_{k+1} + 0.5 Y_k Y_{k+1}) + sum_k (X_k + 0.3 Z_k) at n = 10 as one
    observable, against the density route's exact result (one density per bond and per site,
    cotangents the matching h) within RATIO x the measured floor of the reference's own algorithm
    in the build's precision (tests/floors.py)."""
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 10
    ins, const, var, dens = _density_route_circuit(n, 3, seed=31)
    h2, h1 = np.kron(Z, Z) + 0.5 * np.kron(Y, Y), X + 0.3 * Z
    hs = [h2 if len(d) == 2 else h1 for d in dens]
    cots = lambda rho, dtype: [np.ascontiguousarray(h, dtype=dtype) for h in hs]
    fl = F.Floor(prec, n, ins, const, var, cots=cots, run=False)
    e_exact = sum(np.trace(rho @ h).real for rho, h in zip(fl.exact["forward"], hs))
    terms = []
    for k in range(n - 1):
        terms += [(1.0, f"Z{k} Z{k + 1}"), (0.5, f"Y{k} Y{k + 1}")]
    for k in range(n):
        terms += [(1.0, f"X{k}"), (0.3, f"Z{k}")]
    obs = PauliSum(n, terms)

    def dense(with_observable):
        c = DenseCircuit(n, prec)
        for kind, pos in ins:
            if kind in (O.VAR_Q1, O.VAR_Q2):
                c.add_var_gate(pos)
            elif kind in (O.CONST_Q1, O.CONST_Q2):
                c.add_const_gate(pos)
            elif not with_observable:
                c.get_dens_op_with_grad(pos)
        if with_observable:
            c.get_observable_op_with_grad(obs)
        return c

    c = dense(True)
    (energy,) = c.forward(fl.const, fl.var)
    csum = np.abs(obs.coeffs).sum()
    bound = (F.RATIO * fl.floor["forward"] + F.ATOL[prec]) * csum
    print(f"energy {prec}: got {energy:.15e} exact {e_exact:.15e} err {abs(energy - e_exact):.3e} "
          f"bound {bound:.3e} (floor {fl.floor['forward']:.3e}, sum |c| {csum})")
    assert abs(energy - e_exact) <= bound
    grads = c.backward([1.0], fl.const, fl.var)
    fl.check("grads", grads, what=f"observable {prec} ")
    if prec == "f64":
        d = dense(False)
        rho = d.forward(fl.const, fl.var)
        assert abs(sum(np.trace(r @ h).real for r, h in zip(rho, hs)) - energy) <= 1e-12 * csum
        route = d.backward(fl.cots, fl.const, fl.var)
        err = F.normrel(grads, route)
        print(f"observable vs density route f64: normrel {err:.2e}")
        assert err <= 1e-12


def test_plain_observable_op():
    """get_observable_op is in run and not in forward; outputs come in instruction order; wrong
    counts of cotangents raise the density messages."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 6
    rng = np.random.default_rng(2)
    c = DenseCircuit(n, "f64")
    h_plain = PauliSum(n, [(1.0, "Z0 Z1"), (0.5, "X5")])
    h_diff = PauliSum(n, [(-0.7, "Y0 Y5"), (0.2, "")])
    c.add_var_gate([0, 3, 5])
    c.get_observable_op(h_plain)
    c.get_dens_op_with_grad([1, 2])
    c.add_var_gate([4, 1])
    c.get_observable_op_with_grad(h_diff)
    c.get_dens_op([3])
    var = [O.haar_unitary(rng, 8), O.haar_unitary(rng, 4)]
    psi = np.zeros(1 << n, np.complex128)
    psi[0] = 1
    mid = O.apply_qk_gate(psi, var[0], [0, 3, 5])
    end = O.apply_qk_gate(mid, var[1], [4, 1])
    e_plain = np.vdot(mid, h_plain.to_matrix() @ mid).real
    e_diff = np.vdot(end, h_diff.to_matrix() @ end).real
    out = c.run([], var)
    assert [type(o) for o in out] == [float, np.ndarray, float, np.ndarray]
    assert out[1].shape == (4, 4) and out[3].shape == (2, 2)
    assert abs(out[0] - e_plain) < 1e-12 and abs(out[2] - e_diff) < 1e-12
    fwd = c.forward([], var)
    assert [type(o) for o in fwd] == [np.ndarray, float]
    assert np.array_equal(fwd[0], out[1]) and fwd[1] == out[2]
    cot = np.ascontiguousarray(np.kron(Z, Z))
    with pytest.raises(q.PanicException, match="The number of gradients wrt density matrices is "
                                               "less than required."):
        c.backward([1.0], [], var)
    c.forward([], var)
    with pytest.raises(q.PanicException, match="Number of gradients wrt density matrices is more "
                                               "than required."):
        c.backward([cot, cot, 1.0], [], var)
    c.forward([], var)
    grads = c.backward([cot, 1.0], [], var)
    assert [g.shape for g in grads] == [(64,), (16,)]
    with pytest.raises(TypeError):
        c.get_observable_op("Z0")
    with pytest.raises(q.PanicException, match="different sizes"):
        c.get_observable_op_with_grad(PauliSum(n + 1, [(1.0, "Z0")]))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_full_size(prec):
    """n = 28 (f32) / 27 (f64), |0..0> spread by Hadamards on 0, 7, 20 and n - 1, as
    test_qk_density_full_size does: H = X_0 + X_7 + Z_3 + X_20 X_{n-1} + Y_0 Y_7 within 1e-5.
    The qubits 0, 7, 20, n - 1 are in |+>, qubit 3 stays in |0>, so the five terms give
    1 + 1 + 1 + 1 + 0 = 4.  (The request for this test listed <Z_3> as 0, i.e. E = 3; <0|Z|0> is
    +1.  Each term is also checked alone, so the value of every one is pinned.)"""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    n = 28 if prec == "f32" else 27
    t = q.QuantizedTensor.new_standard(n, precision=prec)
    h = (np.array([[1, 1], [1, -1]]) / np.sqrt(2)).astype(DT[prec])
    for p in (0, 7, 20, n - 1):
        t.apply_q1_gate(h.reshape(-1), p)
    terms = {"X0": 1.0, "X7": 1.0, "Z3": 1.0, f"X20 X{n - 1}": 1.0, "Y0 Y7": 0.0}
    e = t.pauli_energy(PauliSum(n, [(1.0, ops) for ops in terms]))
    print(f"full size {prec}: E = {e:.9f}")
    assert abs(e - sum(terms.values())) < 1e-5
    for ops, want in terms.items():
        assert abs(t.pauli_energy(PauliSum(n, [(1.0, ops)])) - want) < 1e-5, ops

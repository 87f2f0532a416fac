"""Overlap, transition-element and fidelity ops in a differentiable circuit
(DenseCircuit.get_overlap_op[_with_grad], get_fidelity_op[_with_grad],
quantum_differentiable_circuit/dense_circuit.py) over qdc_overlap / qdc_pauli_overlap and their
injections (include/qdc/overlap.h), and examples/vqd_pauli.py."""
import importlib
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_dense_grad import DT, tensor
from test_gpu_pauli import random_sum

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_finite_difference_identity_with_overlaps():
    """tests/test_gpu_pauli_rot_circuit.py::test_finite_difference_identity_with_rotations with
    two-state outputs: f64, n = 9, seed 42, two layers; each layer holds variable Haar gates with
    k = 1..5, after each of them a variable rotation, then a constant rotation and an output:
    layer 0 a differentiable observable E, layer 1 the fidelity F with a random UNNORMALISED
    target given as a host vector and the transition element o2 = <target2|H2|psi> with a second
    target given as a QuantizedTensor; one more variable rotation after the last output.
    Loss = 0.7 E + 1.9 F + Re(o2) - 0.4 Im(o2)^2, so the cotangents are 0.7, 1.9 and
    g2 = 1 - 0.8 Im(o2) i.  8th-order central differences with eta = 1e-6, jointly in the gate
    perturbations p and the angle perturbations dtheta, against sum Re(g . p) + sum dL/dtheta
    dtheta at relative 1e-9; the trailing rotation's gradient is exactly 0.0; backward leaves fwd
    at the initial state (1e-12)."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, eta = 9, 1e-6
    rng = np.random.default_rng(42)
    c = DenseCircuit(n, "f64")
    psi0 = np.zeros(1 << n, np.complex128)
    psi0[0] = 1
    c.set_state_from_vector(psi0)
    place = lambda k: [int(p) for p in rng.permutation(n)[:k]]
    rots = [["Z1 Z6", " ".join("XYZ"[i % 3] + str(i) for i in range(n)), "X8 Z2", "Y0 Y4 Y7", "X3 Y5"],
            ["Z0 Z3 Z8", " ".join("YZX"[i % 3] + str(i) for i in range(n)), "Y8", "Y1 Y2 Z5 Y6", "X0"]]
    var, pert, const = [], [], [0.4, -1.1]
    h1, h2 = (random_sum(rng, n, 12, top=True) for _ in range(2))
    target = O.random_state(rng, n, normalise=False)
    assert abs(np.vdot(target, target).real - 1) > 0.5
    target2 = q.QuantizedTensor.new_from_host(O.random_state(rng, n), precision="f64")
    for layer in range(2):
        for k, ops in zip(rng.permutation([1, 2, 3, 4, 5]), rots[layer]):
            c.add_var_gate(place(k))
            var.append(O.haar_unitary(rng, 1 << k))
            pert.append(rng.standard_normal(1 << (2 * k)) + 1j * rng.standard_normal(1 << (2 * k)))
            c.add_var_pauli_rotation(ops)
            var.append(float(rng.uniform(-3, 3)))
            pert.append(float(rng.standard_normal()))
        c.add_const_pauli_rotation(["Y2 X7", [(8, "Z"), (0, "Y")]][layer])
        if layer == 0:
            c.get_observable_op_with_grad(h1)
        else:
            c.get_fidelity_op_with_grad(target)
            c.get_overlap_op_with_grad(target2, h2)
    c.add_var_pauli_rotation("X4 Y8")
    var.append(0.77)
    pert.append(-0.6)
    is_angle = [isinstance(v, float) for v in var]
    assert sum(is_angle) == 11

    def loss(v):
        e, f, o2 = c.forward(const, v)
        assert isinstance(e, float) and isinstance(f, float) and isinstance(o2, complex)
        return 0.7 * e + 1.9 * f + o2.real - 0.4 * o2.imag ** 2

    coeff = {-4: 1 / 280, -3: -4 / 105, -2: 1 / 5, -1: -4 / 5,
             1: 4 / 5, 2: -1 / 5, 3: 4 / 105, 4: -1 / 280}
    ds_fd = sum(w * loss([g + j * eta * p for g, p in zip(var, pert)])
                for j, w in coeff.items()) / eta
    e, f, o2 = c.forward(const, var)
    assert f > 1e-5 and abs(o2.imag) > 1e-5 and abs(o2.real) > 1e-5  # every term of the loss acts
    grads = c.backward([0.7, 1.9, 1.0 - 0.8j * o2.imag], const, var)
    assert len(grads) == len(var)
    assert [isinstance(g, float) for g in grads] == is_angle
    assert grads[-1] == 0.0
    assert all(g != 0.0 for g, a in zip(grads[:-1], is_angle[:-1]) if a)
    ds = sum(g * p if a else np.tensordot(g, p, axes=1).real
             for g, p, a in zip(grads, pert, is_angle))
    print(f"ds {ds:.12e} ds_fd {ds_fd:.12e} rel {abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)):.2e}")
    assert abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)) < 1e-9
    assert np.abs(c.state.get_cpu_state_copy() - psi0).max() < 1e-12


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_circuit_with_overlaps_is_the_calls_by_hand(prec):
    """A circuit of rotations with fidelity and overlap ops returns, bit for bit, the values and
    dtheta of the same sequence issued through apply_pauli_rotation / overlap / pauli_overlap /
    overlap_inject / pauli_rot_reverse."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 12
    rng = np.random.default_rng(12)
    h = PauliSum(n, [(1.0, "Z0 Z1"), (-0.5, "X11"), (0.25, "Y3 Y10"), (0.2, "")])
    t1, t2, t3 = (tensor(prec, O.random_state(rng, n, normalise=False)) for _ in range(3))
    # (kind, what, value): v / c a variable / constant rotation and its angle; fid, ov, hov an
    # output on a target and its cotangent
    seq = [("v", "X0", 0.3), ("v", "Y11", -1.2), ("c", "X3 X10", 0.9), ("v", "Z0 Z1", 2.1),
           ("fid", t1, 0.6), ("v", "Y0 Z4 X11", -0.4), ("c", "Z7", 1.3), ("ov", t2, 0.4 + 0.9j),
           ("v", "Y0 X5", 0.8), ("hov", t3, -1.7 + 0.2j), ("v", "X5", 0.5)]
    outs = ("fid", "ov", "hov")
    c = DenseCircuit(n, prec)
    for kind, what, _ in seq:
        if kind == "fid":
            c.get_fidelity_op_with_grad(what)
        elif kind == "ov":
            c.get_overlap_op_with_grad(what)
        elif kind == "hov":
            c.get_overlap_op_with_grad(what, h)
        else:
            (c.add_var_pauli_rotation if kind == "v" else c.add_const_pauli_rotation)(what)
    var = [a for k, _, a in seq if k == "v"]
    const = [a for k, _, a in seq if k == "c"]
    values = c.forward(const, var)
    grads = c.backward([a for k, _, a in seq if k in outs], const, var)

    fwd = q.QuantizedTensor.new_standard(n, precision=prec)
    want_v = []
    for kind, what, a in seq:
        if kind == "fid":
            want_v.append(abs(what.overlap(fwd)) ** 2)
        elif kind == "ov":
            want_v.append(what.overlap(fwd))
        elif kind == "hov":
            want_v.append(what.pauli_overlap(fwd, h))
        else:
            fwd.apply_pauli_rotation(what, a)
    bwd, want_g = None, []
    for kind, what, a in reversed(seq):
        if kind in outs:
            g = 2.0 * a * what.overlap(fwd) if kind == "fid" else a
            first = bwd is None
            if first:
                bwd = q.QuantizedTensor(n, prec)
            q.overlap_inject(what, bwd, g, h if kind == "hov" else None, accumulate=not first)
        else:
            d = q.pauli_rot_reverse(fwd, bwd, what, a, want_grad=kind == "v")
            if kind == "v":
                want_g.insert(0, d)
    assert values == want_v and len(values) == 3
    assert isinstance(values[0], float) and all(isinstance(v, complex) for v in values[1:])
    assert grads == want_g and len(grads) == 6 and grads[-1] == 0.0
    assert all(isinstance(g, float) for g in grads) and all(g != 0.0 for g in grads[:5])
    assert np.array_equal(c.state.get_cpu_state_copy(), fwd.get_cpu_state_copy())
    assert np.array_equal(c.bwd.get_cpu_state_copy(), bwd.get_cpu_state_copy())


def test_run_forward_and_targets():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, prec = 7, "f64"
    rng = np.random.default_rng(3)
    h = PauliSum(n, [(0.7, "X0 Z6"), (-0.3, "Y2")])
    vec = O.random_state(rng, n, normalise=False)
    tt = tensor(prec, vec)

    def build(target):
        c = DenseCircuit(n, prec)
        c.add_var_pauli_rotation("X0 Y3")
        c.get_overlap_op(target)              # run only
        c.get_fidelity_op_with_grad(target)
        c.add_var_pauli_rotation("Z1 X6")
        c.get_fidelity_op(target)             # run only
        c.get_overlap_op_with_grad(target, h)
        c.get_overlap_op(target, h)           # run only
        return c

    var = [0.8, -1.9]
    c = build(tt)
    r, f = c.run([], var), c.forward([], var)
    assert len(r) == 5 and len(f) == 2 and f == [r[1], r[3]]
    assert [type(x) for x in r] == [complex, float, float, complex, complex]
    assert r[1] == abs(r[0]) ** 2 and r[3] == r[4]
    g = c.backward([0.5, 1.0 - 2.0j], [], var)
    # a host-vector target is the same target
    cv = build(vec)
    assert cv.run([], var) == r and cv.backward([0.5, 1.0 - 2.0j], [], var) == g
    # a tensor target is held by reference: refilling it changes the next forward
    tt.set_from_host(O.random_state(rng, n))
    f2 = c.forward([], var)
    assert f2[0] != f[0] and f2[1] != f[1]
    assert cv.forward([], var) == f  # (the uploaded copy did not change)
    # the fidelity's cotangent is a real weight
    with pytest.raises(q.PanicException, match="Pauli coefficients must be real."):
        c.backward([0.5j, 1.0], [], var)


def test_builder_panics():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n = 5
    c = DenseCircuit(n, "f32")
    ok, big = q.QuantizedTensor.new_standard(n, "f32"), q.QuantizedTensor.new_standard(n + 1, "f32")
    dbl = q.QuantizedTensor.new_standard(n, "f64")
    builders = (c.get_overlap_op, c.get_overlap_op_with_grad, c.get_fidelity_op,
                c.get_fidelity_op_with_grad)
    for add in builders:
        with pytest.raises(q.PanicException, match="different sizes"):
            add(big)
        with pytest.raises(q.PanicException, match="different sizes"):
            add(np.zeros(1 << (n - 1), np.complex64))
        with pytest.raises(q.PanicException, match="different precisions"):
            add(dbl)
    for add in builders[:2]:
        with pytest.raises(q.PanicException, match="The observable and the tensor have different sizes."):
            add(ok, PauliSum(n + 1, [(1.0, "X0")]))
        with pytest.raises(q.PanicException, match="The observable has no terms."):
            add(ok, PauliSum(n, []))
        with pytest.raises(TypeError):
            add(ok, "X0")
    assert c.instructions == []


def test_vqd_example_finds_both_energies():
    """examples/vqd_pauli.py at 8 qubits, 4 layers, f64, 500 L-BFGS-B iterations per stage: the
    ground and the first excited energy within 1e-3 of numpy.linalg.eigvalsh (an optimiser
    target, not a kernel tolerance: a host emulation of the same loss reaches 1e-6 for both), and
    the penalty leaves |<psi_0|psi_1>|^2 below 1e-2."""
    sys.path.insert(0, str(ROOT / "examples"))
    try:
        vqd = importlib.import_module("vqd_pauli")
    finally:
        sys.path.remove(str(ROOT / "examples"))
    n = 8
    (e0, e1, f1), (t0, t1) = vqd.run(n, 4, 500, 4.0, "f64", 42)
    ev = np.linalg.eigvalsh(vqd.hamiltonian(n).to_matrix())
    print(f"E0 {e0:.9f} exact {ev[0]:.9f}; E1 {e1:.9f} exact {ev[1]:.9f}; F {f1:.2e}; "
          f"{t0 * 1e3:.2f} / {t1 * 1e3:.2f} ms per call")
    assert ev[1] - ev[0] > 0.1
    assert abs(e0 - ev[0]) <= 1e-3 and abs(e1 - ev[1]) <= 1e-3
    assert f1 <= 1e-2

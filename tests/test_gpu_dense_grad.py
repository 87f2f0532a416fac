"""Gradient and reduced density matrix of dense k-qubit gates (include/qdc/dense.h: qdc_qkgrad,
qdc_qkdensity; csrc/qdc_qkgrad.hpp) and the differentiable circuit over them (DenseCircuit).

The reference for k >= 3 is the einsum below (pinned to the oracle's q1 / q2 functions by
tests/test_dense_grad_cpu.py), on the complex128 image of the build-precision inputs, compared
with the reference's per-element metric (O.cmp_complex_slices) at the primitives' tolerances of
tests/test_gpu_primitives.py: 1e-5 (f32), 1e-12 (f64)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
DT = {"f32": np.complex64, "f64": np.complex128}
TOL = {"f32": 1e-5, "f64": 1e-12}

# tests/test_gpu_dense.py's table: in-chunk qubit 0, lane bits, far bits, unsorted order
POSITIONS = {
    1: [[0], [5], [16]],
    2: [[1, 0], [3, 14], [16, 2]],
    3: [[2, 1, 0], [0, 9, 4], [16, 15, 3], [7, 12, 5]],
    4: [[3, 2, 1, 0], [16, 0, 8, 4], [10, 11, 12, 13], [5, 1, 15, 6]],
    5: [[4, 3, 2, 1, 0], [0, 16, 2, 14, 4], [12, 13, 14, 15, 16], [9, 3, 11, 0, 7]],
}


def _groups(state, positions):
    n, k = O.qubits_of(state.size), len(positions)
    axes = [n - 1 - p for p in positions]
    return np.moveaxis(np.asarray(state).reshape([2] * n), axes, range(k)).reshape(1 << k, -1)


def qk_grad_ref(fwd, bwd, positions):
    return np.einsum("rg,cg->rc", _groups(bwd, positions), _groups(fwd, positions)).reshape(-1)


def qk_density_ref(state, positions):
    s = _groups(state, positions)
    return np.einsum("rg,cg->rc", s, s.conj()).reshape(-1)


def trace_out(rho, k, keep):
    """Reduced matrix of a 2^k x 2^k density on its local qubits keep[0..) (most significant
    first), as a flat array."""
    t = np.asarray(rho).reshape([2] * (2 * k))
    rest = [a for a in range(k) if a not in keep]
    t = t.transpose(list(keep) + rest + [k + a for a in keep] + [k + a for a in rest])
    m, r = 1 << len(keep), 1 << len(rest)
    return np.einsum("aibi->ab", t.reshape(m, r, m, r)).reshape(-1)


def tensor(prec, psi):
    import quantum_differentiable_circuit as q
    return q.QuantizedTensor.new_from_host(np.asarray(psi).astype(DT[prec]), precision=prec)


_STATES = {}


def states(prec, n=17, seed=77):
    """(fwd tensor, bwd tensor, fwd, bwd as complex128 of the build-precision values), shared
    and never modified."""
    key = (prec, n, seed)
    if key not in _STATES:
        rng = np.random.default_rng(seed)
        f, b = (O.random_state(rng, n).astype(DT[prec]) for _ in range(2))
        _STATES[key] = (tensor(prec, f), tensor(prec, b), f.astype(np.complex128),
                        b.astype(np.complex128))
    return _STATES[key]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_qk_grad_and_density_every_layout_class(prec, k):
    import quantum_differentiable_circuit as q
    tf, tb, f, b = states(prec)
    for pos in POSITIONS[k]:
        e = O.cmp_complex_slices(q.get_qk_grad(tf, tb, pos), qk_grad_ref(f, b, pos), TOL[prec])
        print(f"grad {prec} k={k} {pos}: rel {e:.2e}")
        e = O.cmp_complex_slices(tf.get_qk_density(pos), qk_density_ref(f, pos), TOL[prec])
        print(f"density {prec} k={k} {pos}: rel {e:.2e}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_k1_k2_are_the_q1_q2_primitives_bit_for_bit(prec):
    import quantum_differentiable_circuit as q
    tf, tb, _, _ = states(prec)
    for (p,) in POSITIONS[1]:
        assert np.array_equal(q.get_qk_grad(tf, tb, [p]), q.get_q1_grad(tf, tb, p))
        assert np.array_equal(tf.get_qk_density([p]), tf.get_q1_density(p))
    for p2, p1 in POSITIONS[2] + [p[::-1] for p in POSITIONS[2]]:
        assert np.array_equal(q.get_qk_grad(tf, tb, [p2, p1]), q.get_q2_grad(tf, tb, p2, p1))
        assert np.array_equal(tf.get_qk_density([p2, p1]), tf.get_q2_density(p2, p1))


@pytest.mark.parametrize("k", [3, 5])
def test_small_states(k):
    """Fewer groups than one tile (n - k < 4, n = k: one group), the density of a state that is
    not normalised."""
    import quantum_differentiable_circuit as q
    rng = np.random.default_rng(3)
    for n in (k, k + 1, k + 3):
        f, b = O.random_state(rng, n, normalise=False), O.random_state(rng, n)
        pos = [int(p) for p in rng.permutation(n)[:k]]
        tf, tb = tensor("f64", f), tensor("f64", b)
        O.cmp_complex_slices(q.get_qk_grad(tf, tb, pos), qk_grad_ref(f, b, pos), TOL["f64"])
        O.cmp_complex_slices(tf.get_qk_density(pos), qk_density_ref(f, pos), TOL["f64"])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_grid_stride_loop_and_tail(monkeypatch, prec, k):
    """Three blocks: every wave walks many tiles, and 2^(13-k) tiles do not divide evenly."""
    import quantum_differentiable_circuit as q
    monkeypatch.setenv("QDC_QKG_GRID", "3")
    tf, tb, f, b = states(prec)
    for pos in POSITIONS[k][1:3]:
        e = O.cmp_complex_slices(q.get_qk_grad(tf, tb, pos), qk_grad_ref(f, b, pos), TOL[prec])
        print(f"grad {prec} k={k} {pos} grid 3: rel {e:.2e}")
        e = O.cmp_complex_slices(tf.get_qk_density(pos), qk_density_ref(f, pos), TOL[prec])
        print(f"density {prec} k={k} {pos} grid 3: rel {e:.2e}")


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_deterministic_and_accumulating(prec, k):
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit._native import ptr
    tf, tb, _, _ = states(prec)
    pos = POSITIONS[k][3]
    arr = (C.c_size_t * k)(*pos)
    once = q.get_qk_grad(tf, tb, pos)
    assert np.array_equal(q.get_qk_grad(tf, tb, pos), once)
    buf = once.copy()
    assert tf._lib.qdc_qkgrad(tf._p, tb._p, ptr(buf), arr, k, 17) is None
    O.cmp_complex_slices(buf, 2 * once, TOL[prec] * 10)
    rho = tf.get_qk_density(pos)
    assert np.array_equal(tf.get_qk_density(pos), rho)
    buf = rho.copy()
    assert tf._lib.qdc_qkdensity(tf._p, ptr(buf), arr, k, 17) is None
    O.cmp_complex_slices(buf, 2 * rho, TOL[prec] * 10)
    # a pre-filled buffer is added to, not overwritten
    fill = (np.arange(once.size) * (1 - 2j)).astype(DT[prec])
    buf = fill.copy()
    assert tf._lib.qdc_qkdensity(tf._p, ptr(buf), arr, k, 17) is None
    # (fill + rho is rounded once, at the magnitude of fill)
    assert np.abs(buf - fill - rho).max() <= 2 * np.finfo(DT[prec]).eps * np.abs(fill).max()
    assert np.abs(buf - rho).max() > 1


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_density_properties(prec, k):
    tf, _, f, _ = states(prec)
    c = 1 << k
    for pos in POSITIONS[k]:
        rho = tf.get_qk_density(pos).reshape(c, c)
        assert np.abs(rho - rho.conj().T).max() < TOL[prec]
        assert abs(np.trace(rho) - np.vdot(f, f)) < TOL[prec]
        if k == 3:
            O.cmp_complex_slices(trace_out(rho, 3, [0, 1]), tf.get_q2_density(pos[0], pos[1]),
                                 TOL[prec])


def test_panics():
    import quantum_differentiable_circuit as q
    t = q.QuantizedTensor.new_standard(6, precision="f32")
    u = q.QuantizedTensor.new_standard(6, precision="f32")
    with pytest.raises(q.PanicException, match="positions must be different"):
        t.get_qk_density([1, 2, 1])
    with pytest.raises(q.PanicException, match="positions must be different"):
        q.get_qk_grad(t, u, [1, 2, 1])
    with pytest.raises(q.PanicException, match="out of the bound"):
        t.get_qk_density([1, 2, 6])
    with pytest.raises(q.PanicException, match="out of the bound"):
        q.get_qk_grad(t, u, [1, 2, 6])
    with pytest.raises(q.PanicException, match="k must be"):
        t.get_qk_density(list(range(6)))
    with pytest.raises(q.PanicException, match="k must be"):
        q.get_qk_grad(t, u, list(range(6)))
    with pytest.raises(q.PanicException, match="fwd and bwd have different lengths"):
        q.get_qk_grad(t, q.QuantizedTensor.new_standard(7, precision="f32"), [0, 1, 2])
    # the C ABI validates too (no Python-side checks on this path)
    lib = q._native.load("f32")
    out = np.zeros(64, np.complex64)
    pos = (C.c_size_t * 3)(0, 0, 1)
    msg = lib.qdc_qkgrad(t._p, u._p, out.ctypes.data, pos, 3, 6)
    assert msg is not None and b"different" in msg
    msg = lib.qdc_qkdensity(t._p, out.ctypes.data, pos, 3, 6)
    assert msg is not None and b"different" in msg
    six = (C.c_size_t * 6)(*range(6))
    msg = lib.qdc_qkdensity(t._p, out.ctypes.data, six, 6, 6)
    assert msg is not None and b"supported range" in msg


def test_dense_circuit_is_abi_circuit_at_k1_k2():
    """Only 1- and 2-qubit instructions: DenseCircuit makes AbiCircuit's kernel calls, so the
    forward densities and the gradients are the same bits."""
    from quantum_differentiable_circuit import (CONST_Q1, CONST_Q2, DIFF_Q1_DENSITY,
                                                DIFF_Q2_DENSITY, Q2_DENSITY, VAR_Q1, VAR_Q2)
    from quantum_differentiable_circuit.abi_circuit import AbiCircuit
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, layers = 10, 3
    rng = np.random.default_rng(12)
    a, d = AbiCircuit(n, "f64"), DenseCircuit(n, "f64")
    const, var = [], []

    def gate(variable, pos):
        (var if variable else const).append(O.haar_unitary(rng, 1 << len(pos)))
        a.add({(1, 0): CONST_Q1, (1, 1): VAR_Q1, (2, 0): CONST_Q2, (2, 1): VAR_Q2}[
            (len(pos), variable)], *pos)
        (d.add_var_gate if variable else d.add_const_gate)(pos)

    def dens(pos, diff=True):
        a.add((DIFF_Q1_DENSITY if len(pos) == 1 else DIFF_Q2_DENSITY) if diff else Q2_DENSITY, *pos)
        (d.get_dens_op_with_grad if diff else d.get_dens_op)(pos)

    for layer in range(layers):
        for p in range(n):
            gate(p % 3 != 0, [p])
        for p in range(layer % 2, n - 1, 2):
            gate(p % 4 != 1, [p + 1, p] if layer % 2 else [p, p + 1])
        dens([int(rng.integers(n))])
        p2, p1 = (int(x) for x in rng.permutation(n)[:2])
        dens([p2, p1])
        dens([p1, p2], diff=False)
    for got, want in zip(d.run(const, var), a.run(const, var)):
        assert np.array_equal(got, want)
    fa, fd = a.forward(const, var), d.forward(const, var)
    assert len(fd) == len(fa) == 2 * layers
    for got, want in zip(fd, fa):
        assert got.shape == want.shape and np.array_equal(got, want)
    cots = [np.ascontiguousarray(c.conj()) for c in O.tsallis_loss_and_cotangents(fa)[1]]
    ga, gd = a.backward(cots, const, var), d.backward(cots, const, var)
    assert len(gd) == len(ga) == len(var)
    for got, want in zip(gd, ga):
        assert got.shape == want.shape and np.array_equal(got, want)


def test_dense_circuit_finite_difference_identity():
    """tests/test_gpu_circuit.py::test_finite_difference_identity for dense gates: f64, n = 9,
    two layers with a variable Haar gate of every k = 1..5 at random placements, constant gates of
    3 and 2 qubits, differentiable densities of 2 and 3 qubits after each layer; 8th-order
    central differences with eta = 1e-6 along random complex directions against
    sum Re(g . p) at relative 1e-9; backward leaves fwd at the initial state (1e-12)."""
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    n, eta = 9, 1e-6
    rng = np.random.default_rng(42)
    c = DenseCircuit(n, "f64")
    psi0 = np.zeros(1 << n, np.complex128)
    psi0[0] = 1
    c.set_state_from_vector(psi0)
    place = lambda k: [int(p) for p in rng.permutation(n)[:k]]
    const, var, pert = [], [], []
    for layer in range(2):
        for k in rng.permutation([1, 2, 3, 4, 5]):
            c.add_var_gate(place(k))
            var.append(O.haar_unitary(rng, 1 << k))
            pert.append(rng.standard_normal(1 << (2 * k)) + 1j * rng.standard_normal(1 << (2 * k)))
        kc = 3 if layer == 0 else 2
        c.add_const_gate(place(kc))
        const.append(O.haar_unitary(rng, 1 << kc))
        c.get_dens_op_with_grad(place(2))
        c.get_dens_op_with_grad(place(3))

    def tsallis(v):
        return O.tsallis_loss_and_cotangents(c.forward(const, v))[0]

    coeff = {-4: 1 / 280, -3: -4 / 105, -2: 1 / 5, -1: -4 / 5,
             1: 4 / 5, 2: -1 / 5, 3: 4 / 105, 4: -1 / 280}
    ds_fd = sum(w * tsallis([g + j * eta * p for g, p in zip(var, pert)])
                for j, w in coeff.items()) / eta
    dens = c.forward(const, var)
    assert [d.shape for d in dens] == [(4, 4), (8, 8)] * 2
    _, cots = O.tsallis_loss_and_cotangents(dens)
    grads = c.backward([np.ascontiguousarray(x.conj()) for x in cots], const, var)
    assert [g.shape for g in grads] == [v.shape for v in var]
    ds = sum(np.tensordot(g, p, axes=1).real for g, p in zip(grads, pert))
    print(f"ds {ds:.12e} ds_fd {ds_fd:.12e} rel {abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)):.2e}")
    assert abs(ds - ds_fd) / min(abs(ds), abs(ds_fd)) < 1e-9
    assert np.abs(c.state.get_cpu_state_copy() - psi0).max() < 1e-12


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_qk_density_full_size(prec):
    """n = 28 (f32) / 27 (f64), |0..0> spread by four Hadamards: unit trace, and the pair
    (positions[0], positions[1]) traced out of it is get_q2_density."""
    import quantum_differentiable_circuit as q
    n = 28 if prec == "f32" else 27
    t = q.QuantizedTensor.new_standard(n, precision=prec)
    h = (np.array([[1, 1], [1, -1]]) / np.sqrt(2)).astype(DT[prec])
    for p in (0, 7, 20, n - 1):
        t.apply_q1_gate(h.reshape(-1), p)
    for k, pos in ((3, [n - 1, 3, 0]), (4, [7, 21, 0, 14]), (5, [0, 1, 20, n - 2, 7])):
        rho = t.get_qk_density(pos).reshape(1 << k, 1 << k)
        assert abs(np.trace(rho) - 1) < 1e-5
        O.cmp_complex_slices(trace_out(rho, k, [0, 1]), t.get_q2_density(pos[0], pos[1]), 1e-5)

"""Gradient and density of dense k-qubit gates (include/qdc/dense.h: qdc_qkgrad, qdc_qkdensity),
the parts that need no GPU: the symbols and their ctypes prototypes, the k-qubit einsum reference
of tests/test_gpu_dense_grad.py pinned to the oracle's q1 / q2 functions (the reference's
convention), and the import of the circuit built on them."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O


def qk_grad_ref(fwd, bwd, positions):
    """G[r*C + c] = sum over groups of bwd[r] * fwd[c]; local index bit (k-1-b) = qubit
    positions[b] (apply_qk_gate's convention)."""
    n, k = O.qubits_of(fwd.size), len(positions)
    axes = [n - 1 - p for p in positions]
    f = np.moveaxis(np.asarray(fwd).reshape([2] * n), axes, range(k)).reshape(1 << k, -1)
    b = np.moveaxis(np.asarray(bwd).reshape([2] * n), axes, range(k)).reshape(1 << k, -1)
    return np.einsum("rg,cg->rc", b, f).reshape(-1)


def qk_density_ref(state, positions):
    """rho[r*C + c] = sum over groups of state[r] * conj(state[c])."""
    n, k = O.qubits_of(state.size), len(positions)
    axes = [n - 1 - p for p in positions]
    s = np.moveaxis(np.asarray(state).reshape([2] * n), axes, range(k)).reshape(1 << k, -1)
    return np.einsum("rg,cg->rc", s, s.conj()).reshape(-1)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_libraries_export_and_type_the_dense_reductions(prec):
    from quantum_differentiable_circuit import _native
    raw = ctypes.CDLL(str(_native.lib_path(prec)))
    assert hasattr(raw, "qdc_qkgrad") and hasattr(raw, "qdc_qkdensity")
    assert "qdc_qkgrad" in _native.RUNTIME and "qdc_qkdensity" in _native.RUNTIME
    lib = _native.load(prec)
    sz = ctypes.POINTER(ctypes.c_size_t)
    assert lib.qdc_qkgrad.restype == ctypes.c_char_p
    assert list(lib.qdc_qkgrad.argtypes) == [ctypes.c_void_p] * 3 + [sz, ctypes.c_size_t,
                                                                     ctypes.c_size_t]
    assert lib.qdc_qkdensity.restype == ctypes.c_char_p
    assert list(lib.qdc_qkdensity.argtypes) == [ctypes.c_void_p] * 2 + [sz, ctypes.c_size_t,
                                                                        ctypes.c_size_t]


def test_qk_reference_extends_q1_q2_conventions():
    n = 7
    rng = np.random.default_rng(5)
    fwd, bwd = O.random_state(rng, n), O.random_state(rng, n)
    for pos in range(n):
        assert np.allclose(qk_grad_ref(fwd, bwd, [pos]), O.get_q1_grad(fwd, bwd, pos),
                           rtol=0, atol=1e-14)
        assert np.allclose(qk_density_ref(fwd, [pos]), O.get_q1_density(fwd, pos),
                           rtol=0, atol=1e-14)
    for pos2 in range(n):
        for pos1 in range(n):  # both orders of every pair
            if pos1 == pos2:
                continue
            assert np.allclose(qk_grad_ref(fwd, bwd, [pos2, pos1]),
                               O.get_q2_grad(fwd, bwd, pos2, pos1), rtol=0, atol=1e-14)
            assert np.allclose(qk_density_ref(fwd, [pos2, pos1]),
                               O.get_q2_density(fwd, pos2, pos1), rtol=0, atol=1e-14)


def test_dense_circuit_imports_without_a_gpu():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import dense_circuit
    assert callable(dense_circuit.DenseCircuit)
    assert "get_qk_grad" in q.__all__ and callable(q.get_qk_grad)
    for name in ("apply_qk_gate_tr", "apply_qk_gate_conj_tr", "get_qk_density"):
        assert callable(getattr(q.QuantizedTensor, name))

"""Pauli rotations exp(-i theta/2 P) on the host: the mask parser (observable.pauli_masks), the
identities the kernels of csrc/qdc_paulirot.hpp rest on (include/qdc/pauli.h), in numpy at n = 5,
and the presence of the two entry points."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
N = 5
# nY = 0, 1, 2, 3 (and a fourth Y for the period of the phase)
STRINGS = ["X0 Z2 X4", "Y1 Z3", "Y0 X2 Y4", "Y0 Y1 Z2 Y3", "Y0 Y1 Y2 Y4", "Z1 Z4", ""]


def rot_matrix(n, ops, theta):
    from quantum_differentiable_circuit import PauliSum
    p = PauliSum(n, [(1.0, ops)]).to_matrix()
    return np.cos(theta / 2) * np.eye(1 << n) - 1j * np.sin(theta / 2) * p, p


def test_pauli_masks():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.observable import pauli_masks
    assert pauli_masks(13, "X0 Y3 Z12") == (0b1001, (1 << 12) | 0b1000)
    assert pauli_masks(13, [(0, "X"), (3, "y"), (12, "Z")]) == pauli_masks(13, "x0 y3 z12")
    assert pauli_masks(4, "") == (0, 0) and pauli_masks(4, []) == (0, 0)
    assert pauli_masks(40, "Y39") == (1 << 39, 1 << 39)
    for ops in STRINGS:
        x, z = pauli_masks(N, ops)
        assert [(1.0, x, z)] == PauliSum(N, [(1.0, ops)]).terms()
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        pauli_masks(5, "X5")
    with pytest.raises(q.PanicException, match="a qubit appears twice in a Pauli term."):
        pauli_masks(5, "X1 Z1")
    with pytest.raises(ValueError):
        pauli_masks(5, "X1 W2")
    with pytest.raises(ValueError):
        pauli_masks(5, [(1, "Q")])
    assert "pauli_rot_reverse" in q.__all__ and callable(q.pauli_rot_reverse)
    assert callable(q.QuantizedTensor.apply_pauli_rotation)


@pytest.mark.parametrize("ops", STRINGS)
def test_identities(ops):
    """P^T = (-1)^nY P, dR/dtheta = -(i/2) P R, and the two forms of dL/dtheta:
    Re sum_i bwd[i] (dR/dtheta fwd_in)[i] = 1/2 Im sum_i bwd[i] (P fwd_out)[i]."""
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.observable import pauli_masks
    theta, h = 0.83, 1e-4
    x, z = pauli_masks(N, ops)
    ny = bin(x & z).count("1")
    r, p = rot_matrix(N, ops, theta)
    dim = 1 << N
    assert np.allclose(p, p.conj().T, atol=0) and np.allclose(p @ p, np.eye(dim), atol=1e-15)
    assert np.array_equal(p.T, (-1) ** ny * p)
    rt = np.cos(theta / 2) * np.eye(dim) - 1j * np.sin(theta / 2) * (-1) ** ny * p
    assert np.abs(r.T - rt).max() < 1e-15
    assert np.abs(r @ rot_matrix(N, ops, -theta)[0] - np.eye(dim)).max() < 1e-15
    dr = -0.5j * p @ r
    fd = (rot_matrix(N, ops, theta + h)[0] - rot_matrix(N, ops, theta - h)[0]) / (2 * h)
    assert np.abs(dr - fd).max() < 1e-8
    rng = np.random.default_rng(ny + 10)
    fwd_in, bwd = (rng.standard_normal(dim) + 1j * rng.standard_normal(dim) for _ in range(2))
    fwd_out = r @ fwd_in
    first = np.sum(bwd * (dr @ fwd_in)).real
    second = 0.5 * np.sum(bwd * (p @ fwd_out)).imag
    scale = 0.5 * np.linalg.norm(bwd) * np.linalg.norm(fwd_in)
    assert abs(first - second) <= 1e-14 * scale
    # and the host definition the GPU tests use: PauliSum.apply is the matrix
    assert np.abs(PauliSum(N, [(1.0, ops)]).apply(fwd_in) - p @ fwd_in).max() < 1e-14


def test_symbols_present():
    from quantum_differentiable_circuit import _native
    header = (ROOT / "include" / "qdc" / "pauli.h").read_text()
    for name in ("qdc_pauli_rot", "qdc_pauli_rot_reverse"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.RUNTIME
        for prec in ("f32", "f64"):
            assert hasattr(ctypes.CDLL(str(_native.lib_path(prec))), name), (name, prec)

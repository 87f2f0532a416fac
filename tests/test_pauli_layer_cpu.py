"""Diagonal Pauli layers exp(-i/2 sum_k theta_k Z^{z_k}) on the host (include/qdc/pauli.h:
qdc_pauli_layer, qdc_pauli_layer_reverse, qdc_pauli_layer_plan; csrc/qdc_paulilayer.hpp): the
entry points, the host plan, the identities the kernels rest on in numpy at n = 5, and the
parser's and the validation's panics."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
N = 5
ZS = [0b00011, 0b10100, 0, 0b11111, 0b00011, 0b01000]  # a duplicate, the identity, weight n
L_OF = {"f32": 11, "f64": 10}
GCAP = 32  # terms of a reducing launch: two real gradients per complex value of a partial


def signs(n, z):
    idx = np.arange(1 << n)
    return np.array([1.0 - 2.0 * (bin(i & z).count("1") & 1) for i in idx])


def plan(n, zs, prec):
    from quantum_differentiable_circuit import pauli_layer_plan
    return pauli_layer_plan(n, np.asarray(zs, dtype=np.uint64), prec)


def test_symbols_present():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import _native
    header = (ROOT / "include" / "qdc" / "pauli.h").read_text()
    for name in ("qdc_pauli_layer", "qdc_pauli_layer_reverse", "qdc_pauli_layer_plan"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.RUNTIME
        for prec in ("f32", "f64"):
            assert hasattr(ctypes.CDLL(str(_native.lib_path(prec))), name), (name, prec)
    for name in ("pauli_layer_reverse", "pauli_layer_plan"):
        assert name in q.__all__ and callable(getattr(q, name))
    assert callable(q.QuantizedTensor.apply_pauli_layer)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_groups(prec):
    lw = L_OF[prec]
    n = 28 if prec == "f32" else 27
    chain = [(1 << i) | (1 << (i + 1)) for i in range(n - 1)]
    p = plan(n, chain, prec)
    # bonds inside the span, the bond across its edge (one low bit), the rest (low mask 0)
    assert p["L"] == lw and p["groups"] == lw + 1 and p["high_terms"] == n - lw
    assert (p["forward_launches"], p["reverse_launches"], p["reverse_grad_launches"]) == (1, 1, 1)
    m = lw + 2
    pairs = [(1 << i) | (1 << j) for i in range(m) for j in range(i)]
    p = plan(m, pairs, prec)
    assert p["groups"] == lw * (lw - 1) // 2 + lw + 1 and p["high_terms"] == 2 * lw + 1
    small = [(1 << i) | (1 << j) for i in range(8) for j in range(i)]
    assert plan(8, small, prec)["groups"] == 28 and plan(8, small, prec)["high_terms"] == 0
    assert plan(m, [1 << (lw + 1)], prec) == dict(p, groups=1, high_terms=1,
                                                   reverse_grad_launches=1)
    assert plan(m, [0], prec)["groups"] == 1 and plan(m, [0], prec)["high_terms"] == 0
    # a wholly high term shares the group of z = 0; duplicates stay separate terms of one group
    assert plan(m, [0, 1 << lw, 3 << lw], prec)["groups"] == 1
    dup = plan(m, [5, 5, 5 | (1 << lw)], prec)
    assert dup["groups"] == 1 and dup["high_terms"] == 1


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_launches_and_invalid_masks(prec):
    rng = np.random.default_rng(3)
    for k, fwd, grad in ((1, 1, 1), (GCAP, 1, 1), (GCAP + 1, 1, 2), (128, 1, 4), (129, 2, 5),
                         (300, 3, 10)):
        p = plan(12, rng.integers(0, 1 << 12, size=k), prec)
        assert (p["forward_launches"], p["reverse_launches"], p["reverse_grad_launches"]) == \
            (fwd, fwd, grad), k
    assert plan(12, [1 << 12], prec) is None
    assert plan(12, [1, 1 << 40], prec) is None
    assert plan(12, [], prec) is None
    assert plan(41, [1], prec) is None
    assert plan(0, [0], prec)["groups"] == 1
    from quantum_differentiable_circuit import _native
    lib = _native.load(prec)
    z = (ctypes.c_ulonglong * 1)(1)
    assert lib.qdc_pauli_layer_plan(z, 1, 12, None) == ctypes.c_size_t(-1).value
    assert lib.qdc_pauli_layer_plan(None, 1, 12, (ctypes.c_uint * 6)()) == ctypes.c_size_t(-1).value


def test_identities():
    """The layer is the product of the rotations in any order and diagonal; U^T = U; the gradient
    1/2 Im sum_i s_k(i) bwd[i] fwd[i] is Re sum_i bwd[i] (dU/dtheta_k fwd_in)[i], is the same before
    and after the multiply, and a split layer is exact."""
    from quantum_differentiable_circuit import PauliSum
    rng = np.random.default_rng(11)
    dim = 1 << N
    th = rng.uniform(-np.pi, np.pi, len(ZS))
    phi = 0.5 * sum(t * signs(N, z) for t, z in zip(th, ZS))
    u = np.diag(np.exp(-1j * phi))
    for order in (range(len(ZS)), reversed(range(len(ZS)))):
        prod = np.eye(dim, dtype=complex)
        for k in order:
            p = PauliSum.from_masks(N, [1.0], [0], [ZS[k]]).to_matrix()
            prod = (np.cos(th[k] / 2) * np.eye(dim) - 1j * np.sin(th[k] / 2) * p) @ prod
        assert np.abs(prod - u).max() < 1e-14
    assert np.array_equal(u.T, u)
    half = len(ZS) // 2
    phi_a = 0.5 * sum(t * signs(N, z) for t, z in zip(th[:half], ZS[:half]))
    phi_b = 0.5 * sum(t * signs(N, z) for t, z in zip(th[half:], ZS[half:]))
    assert np.abs(np.exp(-1j * phi_a) * np.exp(-1j * phi_b) - np.exp(-1j * phi)).max() < 1e-14
    f_in, b = (rng.standard_normal(dim) + 1j * rng.standard_normal(dim) for _ in range(2))
    f_out = u @ f_in
    scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f_in)
    h = 1e-5
    for k, z in enumerate(ZS):
        d = 0.5 * np.sum(signs(N, z) * b * f_out).imag
        du = -0.5j * np.diag(signs(N, z)) @ u
        assert abs(d - np.sum(b * (du @ f_in)).real) <= 1e-14 * scale
        # before and after the multiply: (e^{-i phi} b) (e^{+i phi} f) = b f
        after = 0.5 * np.sum(signs(N, z) * (np.exp(-1j * phi) * b) * (np.exp(1j * phi) * f_out)).imag
        assert abs(d - after) <= 1e-14 * scale
        tp, tm = th.copy(), th.copy()
        tp[k] += h
        tm[k] -= h
        loss = lambda t: np.sum(b * (np.exp(-0.5j * sum(a * signs(N, y) for a, y in zip(t, ZS)))
                                     * f_in)).real
        assert abs(d - (loss(tp) - loss(tm)) / (2 * h)) <= 1e-8 * scale


@pytest.mark.parametrize("bits", [32, 64])
def test_fixed_point_phase(bits):
    """t_k = round(theta_k / 4 pi 2^B) mod 2^B, summed with signs mod 2^B and read as a signed
    number of 2^-B turns, is phi mod 2 pi to K 2^-B turns: wrap-around is the range reduction."""
    rng = np.random.default_rng(bits)
    th = rng.uniform(-40, 40, len(ZS))
    mod = 1 << bits
    t = [round(x / (4 * np.pi) % 1 * 2.0 ** 32) * (1 << (bits - 32)) % mod for x in th]
    for i in range(1 << N):
        s = [1 - 2 * (bin(i & z).count("1") & 1) for z in ZS]
        acc = sum(a * b for a, b in zip(s, t)) % mod
        turns = (acc - mod if acc >= mod // 2 else acc) / mod
        phi = 0.5 * sum(a * b for a, b in zip(s, th))
        # (the emulation rounds at 2^-32 turns in both cases)
        assert abs(np.angle(np.exp(1j * (2 * np.pi * turns - phi)))) <= 2 * np.pi * len(ZS) * 2.0 ** -32


def test_parser_and_validation_panics():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit.observable import layer_angles, layer_masks
    assert list(layer_masks(6, ["Z0 Z5", "", [(2, "z")], "Z0 Z5"])) == [33, 0, 4, 33]
    assert layer_masks(6, []).size == 0 and layer_masks(6, []).dtype == np.uint64
    for bad in (["X0"], ["Z0", "Y1 Z2"], [[(3, "X")]]):
        with pytest.raises(q.PanicException, match="a Pauli layer takes Z strings only."):
            layer_masks(6, bad)
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        layer_masks(6, ["Z6"])
    with pytest.raises(q.PanicException, match="a qubit appears twice in a Pauli term."):
        layer_masks(6, ["Z1 Z1"])
    with pytest.raises(q.PanicException):
        layer_masks(6, "Z0 Z1")  # one string is not a layer
    with pytest.raises(ValueError):
        layer_masks(6, ["Z0 W1"])
    assert layer_angles([0.5, 1], 2).dtype == np.float64
    assert np.array_equal(layer_angles(np.array([1 + 0j, 2]), 2), [1.0, 2.0])
    for bad, count in (([0.1], 2), ([[0.1, 0.2]], 2), (0.3, 1), ([], 1)):
        with pytest.raises(q.PanicException, match="one angle per string"):
            layer_angles(bad, count)
    with pytest.raises(q.PanicException, match="must be real"):
        layer_angles([0.1 + 1j], 1)
    with pytest.raises(q.PanicException, match="a Pauli layer takes Z strings only."):
        q.pauli_layer_plan(6, ["X1"])
    assert q.pauli_layer_plan(6, ["Z1", "Z1 Z2"], "f64")["groups"] == 2

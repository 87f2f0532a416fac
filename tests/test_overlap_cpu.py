"""Overlaps and transition elements on the host (include/qdc/overlap.h: qdc_overlap,
qdc_pauli_overlap, qdc_overlap_inject, qdc_pauli_overlap_inject; csrc/qdc_overlap.hpp): the entry
points, and the conventions of the header pinned in numpy at n <= 6 — o = <a|H|b> against
PauliSum.to_matrix(), the injection bwd += conj(g H t) against a central difference of a loss of
o, and the identity that makes pauli_inject an instance of it.  tests/test_gpu_overlap*.py import
the reference formulas from here."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_pauli import apply_ref, random_sum

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("qdc_overlap", "qdc_pauli_overlap", "qdc_overlap_inject", "qdc_pauli_overlap_inject")


def h_apply(obs, psi):
    """H psi in complex128 (obs None: H = I)."""
    psi = np.asarray(psi, np.complex128)
    return psi.copy() if obs is None else apply_ref(obs, psi)


def overlap_ref(a, b, obs=None):
    """o = <a|H|b> = sum_i conj(a[i]) (H b)[i]."""
    return complex(np.vdot(np.asarray(a, np.complex128), h_apply(obs, b)))


def inject_ref(src, g, obs=None):
    """The injection conj(g * H src) of a loss of o = <src|H|psi>, g = dL/dRe o + i dL/dIm o."""
    return np.conj(complex(g) * h_apply(obs, src))


def scale_of(a, b, obs=None):
    """sum |c_t| * ||a|| * ||b||: the size of the terms that add up to o."""
    c = 1.0 if obs is None else float(np.abs(obs.coeffs).sum())
    return c * float(np.linalg.norm(a)) * float(np.linalg.norm(b))


def loss_and_g(o):
    """L = |o|^2 + 0.3 Re o - 0.7 Im o and g = dL/dRe o + i dL/dIm o."""
    return abs(o) ** 2 + 0.3 * o.real - 0.7 * o.imag, 2 * o + 0.3 - 0.7j


def test_symbols_present():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import _native
    header = (ROOT / "include" / "qdc" / "overlap.h").read_text()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.RUNTIME and name not in _native.PRIMITIVES
    assert len(_native.PRIMITIVES) == 18
    dbl, ull = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_ulonglong)
    vp, sz, d, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_double, ctypes.c_int
    protos = {"qdc_overlap": [vp, vp, sz, dbl],
              "qdc_pauli_overlap": [vp, vp, ull, ull, dbl, sz, sz, dbl],
              "qdc_overlap_inject": [vp, vp, sz, d, d, i],
              "qdc_pauli_overlap_inject": [vp, vp, ull, ull, dbl, sz, sz, d, d, i]}
    for prec in ("f32", "f64"):
        lib = _native.load(prec)
        for name in SYMBOLS:
            fn = getattr(lib, name)  # AttributeError: the library does not export it
            assert fn.restype is ctypes.c_char_p and list(fn.argtypes) == protos[name], name
    assert "overlap_inject" in q.__all__ and callable(q.overlap_inject)
    assert callable(q.QuantizedTensor.overlap) and callable(q.QuantizedTensor.pauli_overlap)


@pytest.mark.parametrize("n", [1, 3, 6])
def test_transition_element_is_the_matrix_element(n):
    rng = np.random.default_rng(20 + n)
    obs = random_sum(rng, n, 10, top=True)
    a, b = (O.random_state(rng, n, normalise=False) for _ in range(2))
    m = obs.to_matrix()
    assert np.abs(apply_ref(obs, b) - m @ b).max() <= 1e-13 * scale_of(1.0, b, obs)
    assert abs(overlap_ref(a, b, obs) - a.conj() @ m @ b) <= 1e-13 * scale_of(a, b, obs)
    assert abs(overlap_ref(a, b) - a.conj() @ b) <= 1e-13 * scale_of(a, b)
    # H is Hermitian: <a|H|b> = conj <b|H|a>
    assert abs(overlap_ref(a, b, obs) - np.conj(overlap_ref(b, a, obs))) <= 1e-13 * scale_of(a, b, obs)


@pytest.mark.parametrize("with_obs", [False, True])
def test_injection_is_the_cotangent_of_a_loss_of_o(with_obs):
    """dL = Re sum_i conj(g (H t))[i] dpsi[i] against a central difference of L(o(psi))."""
    n, eta = 5, 1e-6
    rng = np.random.default_rng(31)
    obs = random_sum(rng, n, 9, top=True) if with_obs else None
    t, psi, dpsi = (O.random_state(rng, n, normalise=False) for _ in range(3))
    loss = lambda p: loss_and_g(overlap_ref(t, p, obs))[0]
    _, g = loss_and_g(overlap_ref(t, psi, obs))
    assert abs(g.imag) > 0.1 and abs(g.real) > 0.1
    want = (loss(psi + eta * dpsi) - loss(psi - eta * dpsi)) / (2 * eta)
    got = float(np.sum(inject_ref(t, g, obs) * dpsi).real)
    # (L is quadratic in psi: the central difference has no truncation error, only rounding)
    assert abs(got - want) <= 1e-8 * max(1.0, abs(want)), (got, want)


def test_fidelity_and_energy_are_instances():
    n = 4
    rng = np.random.default_rng(32)
    obs = random_sum(rng, n, 7, top=True)
    t, psi = (O.random_state(rng, n, normalise=False) for _ in range(2))
    # check 1: F = |o|^2 has g = 2 o
    o = overlap_ref(t, psi)
    eta, dpsi = 1e-6, O.random_state(rng, n)
    fd = (abs(overlap_ref(t, psi + eta * dpsi)) ** 2 - abs(overlap_ref(t, psi - eta * dpsi)) ** 2) / (2 * eta)
    assert abs(float(np.sum(inject_ref(t, 2 * o) * dpsi).real) - fd) <= 1e-8 * max(1.0, abs(fd))
    # check 2: the bra frozen at psi, g = 2 w: pauli_inject's 2 w conj(H psi), exactly
    w = -0.65
    assert np.array_equal(inject_ref(psi, 2 * w, obs), 2 * w * np.conj(apply_ref(obs, psi)))
    # and that injection is the gradient of w <psi|H|psi> in psi
    e = lambda p: w * overlap_ref(p, p, obs).real
    fd = (e(psi + eta * dpsi) - e(psi - eta * dpsi)) / (2 * eta)
    assert abs(float(np.sum(inject_ref(psi, 2 * w, obs) * dpsi).real) - fd) <= 1e-8 * max(1.0, abs(fd))

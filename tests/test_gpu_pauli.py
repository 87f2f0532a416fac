"""Pauli-sum observables on the GPU (include/qdc/pauli.h: qdc_pauli_energy, qdc_pauli_inject;
csrc/qdc_pauli.hpp).

The reference is numpy in complex128 on the build-precision inputs: P applied by index arithmetic
as the header defines it, (P psi)[i] = i^nY (-1)^popcount(j & z) psi[j] with j = i ^ x; for
n <= 12 also PauliSum.to_matrix() (pinned to Kronecker products by tests/test_pauli_cpu.py).  The
states are those of tests/test_gpu_dense_grad.py (n = 17, seed 77), the tolerances the
primitives' own (tests/test_gpu_primitives.py): 1e-5 (f32), 1e-12 (f64), on |E - E_ref| /
(sum |c_t| ||psi||^2) and on the norm-relative error of an injected state."""
import ctypes as C

import numpy as np
import pytest

from floors import normrel
from oracle import oracle as O
from test_gpu_dense_grad import DT, TOL, states, tensor
from test_pauli_cpu import ising, table_cap

pytestmark = pytest.mark.gpu
N = 17


def parity(v):
    v = v.copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return (v & np.uint64(1)).astype(np.int64)


def apply_ref(obs, psi):
    """H psi by the index rule of the definition, complex128."""
    psi = np.asarray(psi, np.complex128)
    idx = np.arange(psi.size, dtype=np.uint64)
    out = np.zeros_like(psi)
    for c, x, z in obs.terms():
        j = idx ^ np.uint64(x)
        sign = 1.0 - 2.0 * parity(j & np.uint64(z))
        out += c * (1j ** (bin(x & z).count("1") % 4)) * sign * psi[j]
    return out


def energy_ref(obs, psi):
    e = np.vdot(np.asarray(psi, np.complex128), apply_ref(obs, psi))
    assert abs(e.imag) <= 1e-9 * max(1.0, abs(e.real))
    return float(e.real)


def tile_width(prec):
    from quantum_differentiable_circuit import PauliSum, observable
    return observable.plan(PauliSum(1, [(1.0, "Z0")]), prec)["W"]


def check_energy(prec, t, psi, obs, what):
    got, want = t.pauli_energy(obs), energy_ref(obs, psi)
    scale = np.abs(obs.coeffs).sum() * np.vdot(psi, psi).real
    print(f"energy {prec} {what}: got {got:.15e} want {want:.15e} err/scale "
          f"{abs(got - want) / scale:.2e}")
    assert abs(got - want) <= TOL[prec] * scale, what
    return got


def check_inject(prec, tf, psi, obs, what, weight=1.0, onto=None):
    """accumulate=False into a bwd full of NaN (a kernel that read it, or skipped an amplitude,
    would leave one), or accumulate=True onto the known state `onto`."""
    import quantum_differentiable_circuit as q
    want = 2.0 * weight * apply_ref(obs, psi).conj()
    if onto is None:
        tb = tensor(prec, np.full(psi.size, np.nan + 1j * np.nan))
        q.pauli_inject(tf, tb, obs, weight, accumulate=False)
    else:
        tb = tensor(prec, onto)
        want = want + onto.astype(DT[prec]).astype(np.complex128)
        q.pauli_inject(tf, tb, obs, weight)
    got = tb.get_cpu_state_copy()
    assert np.isfinite(got.view(got.real.dtype)).all(), what
    err = normrel(got, want)
    print(f"inject {prec} {what}: normrel {err:.2e}")
    assert err <= TOL[prec], what
    return got


def single_terms(w):
    terms = [""]
    for p in (0, w - 1, w, N - 1):
        terms += [f"Z{p}", f"X{p}", f"Y{p}"]
    # 1, 2, 3 and 4 Y's (the four phases), inside a tile and reaching past it
    terms += ["Y2", "Y1 Y5", "Y0 Y3 Y9", f"Y1 Y4 Y8 Y{w - 1}"]
    terms += [f"Y{N - 1}", f"Y3 Y{N - 1}", f"Y0 Y{w} Y{N - 1}", f"Y1 Y{w - 1} Y{w} Y{N - 1}"]
    terms += [f"Y2 Z6 X{w - 2}", f"Z0 Y{w + 1} Z{N - 1}"]
    terms.append(" ".join("XYZ"[q % 3] + str(q) for q in range(N)))  # weight 17
    terms += [f"X0 X{N - 1}", f"Z1 X{w} Y{N - 1}"]  # far, lowest x bit 0 and W
    return terms


def random_sum(rng, n, count, top=False):
    from quantum_differentiable_circuit import PauliSum
    terms = []
    for t in range(count):
        qs = [int(p) for p in rng.permutation(n)[:int(rng.integers(1, min(n, 9) + 1))]]
        if top and t % 3 == 0 and n - 1 not in qs:
            qs[0] = n - 1
        terms.append((float(rng.standard_normal()), [(p, "XYZ"[int(rng.integers(3))]) for p in qs]))
    return PauliSum(n, terms)


def sums(prec):
    from quantum_differentiable_circuit import PauliSum
    return {"ising": PauliSum(N, ising(N, 0.8)),
            "random40": random_sum(np.random.default_rng(5), N, 40, top=True)}


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_single_terms(prec):
    from quantum_differentiable_circuit import PauliSum
    tf, _, f, _ = states(prec)
    for ops in single_terms(tile_width(prec)):
        check_energy(prec, tf, f, PauliSum(N, [(1.0, ops)]), repr(ops))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_state_that_is_not_normalised(prec):
    from quantum_differentiable_circuit import PauliSum
    w = tile_width(prec)
    psi = O.random_state(np.random.default_rng(9), N, normalise=False).astype(DT[prec])
    t, psi = tensor(prec, psi), psi.astype(np.complex128)
    assert abs(np.vdot(psi, psi).real - 1) > 0.5
    e = check_energy(prec, t, psi, PauliSum(N, [(1.0, "")]), "identity")
    assert abs(e - np.vdot(psi, psi).real) <= TOL[prec] * np.vdot(psi, psi).real
    for ops in (f"Z{w}", "X3 Y4", f"Y0 X{N - 1}"):
        check_energy(prec, t, psi, PauliSum(N, [(-1.5, ops)]), repr(ops))
    check_inject(prec, t, psi, PauliSum(N, [(-1.5, f"Y0 X{N - 1}"), (0.5, "Z2")]), "unnormalised")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sums(prec):
    tf, _, f, _ = states(prec)
    for name, obs in sums(prec).items():
        check_energy(prec, tf, f, obs, name)
    # more launches than one batch of reduction slots
    from quantum_differentiable_circuit import observable
    many = random_sum(np.random.default_rng(6), N, 64, top=True)
    assert observable.plan(many, prec)["energy_launches"] > 32
    check_energy(prec, tf, f, many, "random64")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_injection(prec):
    from quantum_differentiable_circuit import PauliSum, observable
    tf, _, f, b = states(prec)
    w = tile_width(prec)
    for name, obs in sums(prec).items():
        check_inject(prec, tf, f, obs, name)
        check_inject(prec, tf, f, obs, name + " accumulate", weight=0.75, onto=b)
        check_inject(prec, tf, f, obs, name + " w < 0", weight=-1.25)
    far_only = PauliSum(N, [(0.9, f"X{N - 1}"), (-0.4, f"Y{w} Z3"), (0.6, f"X{w + 1} X0"),
                            (1.1, f"X{N - 1} Z{w}")])
    p = observable.plan(far_only, prec)
    assert p["window_groups"] == 0 and p["far_groups"] == 3
    check_inject(prec, tf, f, far_only, "no window group")
    check_inject(prec, tf, f, far_only, "no window group accumulate", weight=-2.0, onto=b)
    check_energy(prec, tf, f, far_only, "no window group")


@pytest.mark.parametrize("n", ["1", "2", "3", "W-1", "W", "W+1"])
def test_small_states(n):
    """f64; random strings, every third on the top qubit; energy, injection, and to_matrix()."""
    w = tile_width("f64")
    n = {"W-1": w - 1, "W": w, "W+1": w + 1}.get(n) or int(n)
    rng = np.random.default_rng(100 + n)
    obs = random_sum(rng, n, 12, top=True)
    psi = O.random_state(rng, n, normalise=False)
    onto = O.random_state(rng, n)
    t = tensor("f64", psi)
    e = check_energy("f64", t, psi, obs, f"n={n}")
    got = check_inject("f64", t, psi, obs, f"n={n}", weight=0.6)
    check_inject("f64", t, psi, obs, f"n={n} accumulate", weight=-0.3, onto=onto)
    if n <= 12:
        m = obs.to_matrix()
        scale = np.abs(obs.coeffs).sum() * np.vdot(psi, psi).real
        assert abs(e - np.vdot(psi, m @ psi).real) <= TOL["f64"] * scale
        assert normrel(got, 1.2 * (m @ psi).conj()) <= TOL["f64"]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_grid_stride_loops_and_tails(monkeypatch, prec):
    """Three blocks: 2^(17-W) tiles and 2^16 / 1024 spans of pairs do not divide evenly."""
    monkeypatch.setenv("QDC_PAULI_GRID", "3")
    tf, _, f, b = states(prec)
    for name, obs in sums(prec).items():
        check_energy(prec, tf, f, obs, name + " grid 3")
        check_inject(prec, tf, f, obs, name + " grid 3")
        check_inject(prec, tf, f, obs, name + " grid 3 accumulate", weight=0.5, onto=b)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_groups_larger_than_the_table(prec):
    """A diagonal group of cap + 5 terms and a far group of cap + 1 (n = 13: several tiles)."""
    from quantum_differentiable_circuit import PauliSum, observable
    n, cap = 13, table_cap(prec)
    rng = np.random.default_rng(8)
    coeff = lambda: float(rng.standard_normal())
    # cap + 5 distinct Z strings; cap + 1 strings on the footprint X/Y12 X0 (both phase classes)
    diag = [(coeff(), [(p, "Z") for p in range(12) if (m >> p) & 1]) for m in range(cap + 5)]
    far = [(coeff(), [(12, "XY"[m % 2]), (0, "X")] + [(p + 1, "Z") for p in range(11) if (m >> p) & 1])
           for m in range(cap + 1)]
    obs = PauliSum(n, diag + far)
    assert len(obs) == 2 * cap + 6
    p = observable.plan(obs, prec)
    assert (p["window_groups"], p["far_groups"], p["energy_launches"]) == (1, 1, 4)
    psi = O.random_state(rng, n).astype(DT[prec])
    t, psi = tensor(prec, psi), psi.astype(np.complex128)
    check_energy(prec, t, psi, obs, "chunked")
    check_inject(prec, t, psi, obs, "chunked")
    check_inject(prec, t, psi, obs, "chunked accumulate", weight=-0.5,
                 onto=O.random_state(rng, n))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_deterministic_and_accumulating(prec):
    import quantum_differentiable_circuit as q
    tf, tb, f, _ = states(prec)
    obs = sums(prec)["random40"]
    once = tf.pauli_energy(obs)
    assert tf.pauli_energy(obs) == once
    a, b = (q.QuantizedTensor(N, prec) for _ in range(2))
    q.pauli_inject(tf, a, obs, 0.5, accumulate=False)
    q.pauli_inject(tf, b, obs, 0.5, accumulate=False)
    assert np.array_equal(a.get_cpu_state_copy(), b.get_cpu_state_copy())
    e = C.c_double(5.0)
    assert tf._lib.qdc_pauli_energy(tf._p, *obs._args(), N, C.byref(e)) is None
    assert e.value == 5.0 + once and abs(e.value - once) > 1


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_launch_counts(prec):
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import observable
    tf, _, _, _ = states(prec)
    obs = sums(prec)["ising"]
    p = observable.plan(obs, prec)
    assert p["far_groups"] == N - p["W"] and p["energy_launches"] == 1 + p["far_groups"]
    out = q.QuantizedTensor(N, prec)
    q.primitives_profile(True, prec)
    try:
        tf.pauli_energy(obs)
        q.pauli_inject(tf, out, obs, 1.0, accumulate=False)
        q.pauli_inject(tf, out, obs, 1.0)
        stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    count = lambda name: stats.get(name, {"launches": 0})["launches"]
    s = float(16 << N if prec == "f64" else 8 << N)
    assert count("pauli_window") == 1 and count("pauli_far") == p["far_groups"]
    assert count("pauli_window") + count("pauli_far") == p["energy_launches"]
    assert count("pauli_window_inj") + count("pauli_far_inj") == 2 * p["inject_launches"]
    assert count("pauli_window_inj") == 2
    # algorithmic bytes: S per energy pass; 2 S storing, 3 S accumulating
    assert stats["pauli_window"]["algo_bytes"] == s
    assert stats["pauli_far"]["algo_bytes"] == s * p["far_groups"]
    assert stats["pauli_window_inj"]["algo_bytes"] == 5 * s
    assert stats["pauli_far_inj"]["algo_bytes"] == 6 * s * p["far_groups"]


def test_panics():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    t = q.QuantizedTensor.new_standard(6, precision="f32")
    u = q.QuantizedTensor.new_standard(6, precision="f32")
    obs = PauliSum(6, [(1.0, "X0 Z5")])
    with pytest.raises(q.PanicException, match="different sizes"):
        t.pauli_energy(PauliSum(7, [(1.0, "X0")]))
    with pytest.raises(q.PanicException, match="different sizes"):
        q.pauli_inject(t, u, PauliSum(5, [(1.0, "X0")]))
    with pytest.raises(q.PanicException, match="fwd and bwd have different lengths"):
        q.pauli_inject(t, q.QuantizedTensor.new_standard(7, precision="f32"), obs)
    with pytest.raises(q.PanicException, match="The observable has no terms."):
        t.pauli_energy(PauliSum(6, []))
    with pytest.raises(q.PanicException, match="The observable has no terms."):
        q.pauli_inject(t, u, PauliSum(6, []))
    with pytest.raises(q.PanicException, match="fwd and bwd must be different states."):
        q.pauli_inject(t, t, obs)
    with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
        q.pauli_inject(t, u, obs, weight=float("inf"))
    with pytest.raises(q.PanicException, match="Pauli coefficients must be real."):
        q.pauli_inject(t, u, obs, weight=1j)
    # the C ABI validates too (no Python-side checks on this path)
    lib = q._native.load("f32")
    ull, dbl = C.c_ulonglong * 2, C.c_double * 2
    e = C.c_double(0.0)
    x, z, c = ull(1, 64), ull(0, 0), dbl(1.0, 1.0)
    msg = lib.qdc_pauli_energy(t._p, x, z, c, 2, 6, C.byref(e))
    assert msg == b"pos is out of the bound."
    msg = lib.qdc_pauli_inject(t._p, u._p, z, x, c, 2, 6, 1.0, 1)
    assert msg == b"pos is out of the bound."
    x = ull(1, 32)
    assert lib.qdc_pauli_energy(t._p, x, z, c, 0, 6, C.byref(e)) == b"The observable has no terms."
    assert lib.qdc_pauli_inject(t._p, u._p, x, z, c, 0, 6, 1.0, 0) == b"The observable has no terms."
    msg = lib.qdc_pauli_energy(t._p, x, z, dbl(1.0, float("inf")), 2, 6, C.byref(e))
    assert msg == b"Pauli coefficients must be finite."
    msg = lib.qdc_pauli_inject(t._p, u._p, x, z, c, 2, 6, float("nan"), 1)
    assert msg == b"Pauli coefficients must be finite."
    msg = lib.qdc_pauli_inject(t._p, t._p, x, z, c, 2, 6, 1.0, 1)
    assert msg is not None and b"different states" in msg
    msg = lib.qdc_pauli_energy(t._p, x, z, c, 2, 41, C.byref(e))
    assert msg is not None and b"supported range" in msg
    assert e.value == 0.0
    # and a valid call through the raw symbol: |0..0> has <Z5 X0> = 0, <Z5> = 1
    assert lib.qdc_pauli_energy(t._p, ull(0, 1), ull(32, 32), c, 2, 6, C.byref(e)) is None
    assert e.value == 1.0

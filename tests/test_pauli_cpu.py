"""Pauli-sum observables on the host (no GPU): PauliSum's parsing, merging and panics, its dense
matrix against Kronecker products (the bit order and the Y sign of include/qdc/pauli.h), and the
launch plan of the energy / injection kernels (qdc_pauli_plan, csrc/qdc_pauli.hpp)."""
import ctypes as C

import numpy as np
import pytest

PAULI = {"I": np.eye(2, dtype=np.complex128),
         "X": np.array([[0, 1], [1, 0]], np.complex128),
         "Y": np.array([[0, -1j], [1j, 0]], np.complex128),
         "Z": np.array([[1, 0], [0, -1]], np.complex128)}


def kron_string(n, ops):
    """The matrix of a Pauli string {qubit: letter}: qubit 0 is the least significant index bit,
    so it is the LAST Kronecker factor."""
    m = np.ones((1, 1), np.complex128)
    for q in range(n - 1, -1, -1):
        m = np.kron(m, PAULI[ops.get(q, "I")])
    return m


def ising(n, field=1.0):
    return ([(1.0, f"Z{k} Z{k + 1}") for k in range(n - 1)] + [(field, f"X{k}") for k in range(n)])


def test_parsing_and_masks():
    from quantum_differentiable_circuit import PauliSum
    obs = PauliSum(13, [(0.5, "X0 Y3 Z12"), (-2, ""), (1.5, [(1, "z"), (2, "Y")])])
    assert obs.qubits_number == 13 and len(obs) == 3
    assert obs.terms() == [(-2.0, 0, 0), (1.5, 0b100, 0b110),
                           (0.5, 0b1001, (1 << 12) | 0b1000)]
    assert obs.xmasks.dtype == np.uint64 and obs.coeffs.dtype == np.float64
    same = PauliSum.from_masks(13, [1.5, 0.5, -2], [4, 9, 0], [6, 4104, 0])
    assert same.terms() == obs.terms()
    # numpy scalars and complex coefficients with zero imaginary part are real coefficients
    assert PauliSum(2, [(np.float32(2), "X1"), (1 + 0j, "X1")]).terms() == [(3.0, 2, 0)]


def test_merging():
    from quantum_differentiable_circuit import PauliSum
    obs = PauliSum(4, [(1.0, "X0 Z1"), (0.25, "Z1 X0"), (2.0, "Y2"), (-1.0, [(2, "Y")])])
    assert obs.terms() == [(1.25, 1, 2), (1.0, 4, 4)]
    np.testing.assert_allclose(obs.to_matrix(), 1.25 * kron_string(4, {0: "X", 1: "Z"})
                               + kron_string(4, {2: "Y"}), atol=0)


def test_panics():
    from quantum_differentiable_circuit import PanicException, PauliSum
    with pytest.raises(PanicException, match="a qubit appears twice in a Pauli term."):
        PauliSum(4, [(1.0, "X1 Z1")])
    with pytest.raises(PanicException, match="a qubit appears twice in a Pauli term."):
        PauliSum(4, [(1.0, [(2, "Y"), (2, "Y")])])
    with pytest.raises(PanicException, match="pos is out of the bound."):
        PauliSum(4, [(1.0, "X4")])
    with pytest.raises(PanicException, match="pos is out of the bound."):
        PauliSum.from_masks(4, [1.0], [16], [0])
    with pytest.raises(PanicException, match="pos is out of the bound."):
        PauliSum.from_masks(4, [1.0], [0], [1 << 40])
    with pytest.raises(PanicException, match="Pauli coefficients must be real."):
        PauliSum(4, [(1.0 + 0.5j, "X1")])
    with pytest.raises(PanicException, match="Pauli coefficients must be real."):
        PauliSum.from_masks(4, [1j], [1], [0])
    with pytest.raises(PanicException, match="Pauli coefficients must be finite."):
        PauliSum(4, [(float("nan"), "X1")])
    with pytest.raises(PanicException, match="at most 12 qubits"):
        PauliSum(13, [(1.0, "X1")]).to_matrix()
    with pytest.raises(ValueError):
        PauliSum(4, [(1.0, "W1")])


@pytest.mark.parametrize("ops", ["X0", "Y1", "Z2", "Y0 Y2", "X0 Y1 Z2"])
def test_to_matrix_against_kronecker_products(ops):
    """n = 3: qubit 0 is the least significant index bit, Y = [[0, -i], [i, 0]]."""
    from quantum_differentiable_circuit import PauliSum
    obs = PauliSum(3, [(1.0, ops)])
    want = kron_string(3, {int(t[1:]): t[0] for t in ops.split()})
    m = obs.to_matrix()
    assert m.shape == (8, 8) and m.dtype == np.complex128
    assert np.array_equal(m, want)
    assert np.array_equal(m, m.conj().T)
    # the index rule of the definition, applied to a vector, is the same operator
    v = np.random.default_rng(1).standard_normal(8) + 1j * np.arange(8)
    np.testing.assert_allclose(obs.apply(v), want @ v, atol=1e-15)


def test_to_matrix_of_a_sum():
    from quantum_differentiable_circuit import PauliSum
    terms = [(0.7, "X0 X4"), (-1.1, "Y0 Z2 Y3"), (0.3, ""), (2.0, "Z1 Y4")]
    want = (0.7 * kron_string(5, {0: "X", 4: "X"}) - 1.1 * kron_string(5, {0: "Y", 2: "Z", 3: "Y"})
            + 0.3 * np.eye(32) + 2.0 * kron_string(5, {1: "Z", 4: "Y"}))
    np.testing.assert_allclose(PauliSum(5, terms).to_matrix(), want, atol=1e-15)


# ---- the launch plan ------------------------------------------------------------------------
def plan_of(n, terms, prec):
    from quantum_differentiable_circuit import PauliSum, observable
    return observable.plan(PauliSum(n, terms), prec)


def tile_width(prec):
    return plan_of(1, [(1.0, "Z0")], prec)["W"]


def table_cap(prec):
    """The table entries of one launch: the largest diagonal group that is one launch."""
    k = 1
    while k < 4096:
        p = plan_of(13, [(1.0, [(q, "Z") for q in range(13) if (m >> q) & 1])
                         for m in range(k + 1)], prec)
        if p["energy_launches"] > 1:
            return k
        k += 1
    raise AssertionError("no cap found")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_tile_width(prec):
    """A tile of 2^W amplitudes is 16 KiB in either precision."""
    w = tile_width(prec)
    assert (1 << w) * (8 if prec == "f32" else 16) == 16384


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_ising_chain(prec):
    """n = W + 3: the ZZ group and X_0 .. X_{W-1} share one pass; X_W, X_{W+1}, X_{W+2} are far."""
    w = tile_width(prec)
    n = w + 3
    p = plan_of(n, ising(n), prec)
    assert p["merged"] == 2 * n - 1
    assert p["window_groups"] == w + 1 and p["far_groups"] == 3
    assert p["energy_launches"] == 4 and p["inject_launches"] == 4
    assert p["group_x"] == [0] + [1 << q for q in range(w)] + [1 << q for q in range(w, n)]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_window_boundary(prec):
    w = tile_width(prec)
    n = w + 2
    p = plan_of(n, [(1.0, f"X{w - 1}")], prec)
    assert (p["window_groups"], p["far_groups"], p["group_x"]) == (1, 0, [1 << (w - 1)])
    p = plan_of(n, [(1.0, f"X{w}")], prec)
    assert (p["window_groups"], p["far_groups"], p["group_x"]) == (0, 1, [1 << w])
    assert p["energy_launches"] == 1 and p["inject_launches"] == 1
    # Y counts by its x bit, Z never makes a group far; each class ascending, window first
    p = plan_of(n, [(1.0, f"Y{w} Z0"), (1.0, f"Z{n - 1}"), (1.0, f"X1 Z{n - 1}"),
                    (1.0, f"X0 X{w + 1}"), (1.0, "Y0")], prec)
    assert p["group_x"] == [0, 1, 2, 1 << w, (1 << (w + 1)) | 1]
    assert (p["window_groups"], p["far_groups"], p["energy_launches"]) == (3, 2, 3)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_small_state_is_all_window(prec):
    w = tile_width(prec)
    for n in (1, 3, w - 1):
        p = plan_of(n, ising(n) + [(0.5, f"Y0 Y{n - 1}" if n > 1 else "Y0")], prec)
        assert p["far_groups"] == 0 and p["energy_launches"] == 1
        assert p["window_groups"] == len(p["group_x"]) and p["group_x"] == sorted(p["group_x"])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_merges_duplicates(prec):
    from quantum_differentiable_circuit import observable
    p = observable.plan_masks(6, [1, 1, 0, 1, 0], [2, 2, 5, 3, 5], prec)
    assert p["merged"] == 3 and p["window_groups"] == 2 and p["group_x"] == [0, 1]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_chunks_groups_larger_than_the_table(prec):
    w, cap = tile_width(prec), table_cap(prec)
    assert cap >= 16
    n = w + 2
    zs = lambda count: [[(q, "Z") for q in range(12) if (m >> q) & 1] for m in range(count)]
    diag = [(1.0, ops) for ops in zs(cap + 5)]
    p = plan_of(n, diag, prec)
    assert (p["window_groups"], p["energy_launches"], p["inject_launches"]) == (1, 2, 2)
    p = plan_of(n, diag + [(1.0, "X3")], prec)  # the tail of the group and X3 share a launch
    assert (p["window_groups"], p["energy_launches"]) == (2, 2)
    p = plan_of(n, [(1.0, ops) for ops in zs(2 * cap)] + [(1.0, "X3")], prec)
    assert p["energy_launches"] == 3
    far = [(1.0, [(w + 1, "X")] + ops) for ops in zs(cap + 1)]
    p = plan_of(n, far, prec)
    assert (p["window_groups"], p["far_groups"], p["energy_launches"]) == (0, 1, 2)
    p = plan_of(n, diag + far, prec)
    assert (p["window_groups"], p["far_groups"], p["energy_launches"]) == (1, 1, 4)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan_rejects_invalid_arguments(prec):
    from quantum_differentiable_circuit import _native, observable
    assert observable.plan_masks(4, [16], [0], prec) is None       # x bit at n
    assert observable.plan_masks(4, [0], [1 << 63], prec) is None  # z bit far above n
    assert observable.plan_masks(4, [], [], prec) is None          # no terms
    assert observable.plan_masks(41, [1], [0], prec) is None       # n out of range
    lib = _native.load(prec)
    x = (C.c_ulonglong * 3)(0, 1, 2)
    z = (C.c_ulonglong * 3)(1, 0, 0)
    out = (C.c_uint * 6)()
    gx = (C.c_ulonglong * 3)()
    bad = C.c_size_t(-1).value
    assert lib.qdc_pauli_plan(x, z, 3, 4, out, gx, 2) == bad  # cap below the three groups
    assert lib.qdc_pauli_plan(x, z, 3, 4, out, gx, 3) == 3
    assert list(gx) == [0, 1, 2] and list(out)[1:] == [3, 3, 0, 1, 1]

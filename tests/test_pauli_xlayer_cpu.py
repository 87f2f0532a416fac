"""Pauli layers with a shared X/Y footprint on the host (include/qdc/pauli.h: qdc_pauli_xlayer,
qdc_pauli_xlayer_reverse, qdc_pauli_xlayer_plan; csrc/qdc_paulixlayer.hpp): the pair formula the
kernels rest on against the product of the rotations in numpy, the gradient formula against finite
differences, the mask helpers, the excitation generators against dense Jordan-Wigner matrices, the
host plan, and an emulation of the fixed-point phase in f32."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
L_OF = {"f32": 11, "f64": 10}


def popcount(a):
    return bin(int(a)).count("1")


def signs(n, z):
    """s(i) = (-1)^popcount(i & z) for every index, float64."""
    x = np.arange(1 << n, dtype=np.uint64) & np.uint64(z)
    for sh in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(sh)
    return 1.0 - 2.0 * (x & np.uint64(1)).astype(np.float64)


def string_apply(n, x, z, psi):
    """P psi by the index rule of include/qdc/pauli.h, complex128 (or wider)."""
    j = np.arange(1 << n, dtype=np.uint64) ^ np.uint64(x)
    ph = (1, 1j, -1, -1j)[popcount(x & z) % 4]
    return ph * signs(n, z)[j] * psi[j]


def rotations(n, x, zs, th, psi):
    """The reference of every xlayer test: psi <- cos(theta_k/2) psi - i sin(theta_k/2) P_k psi
    for each k in turn."""
    psi = np.asarray(psi, dtype=np.complex128).copy()
    for z, t in zip(zs, th):
        psi = np.cos(t / 2) * psi - 1j * np.sin(t / 2) * string_apply(n, x, z, psi)
    return psi


def pair_terms(x, zs):
    """(par, ph0, eps, hb): the parity of every nY, i^par, the host signs and the deleted bit."""
    ny = [popcount(x & z) for z in zs]
    par = ny[0] & 1
    assert all(k & 1 == par for k in ny)
    eps = np.array([(-1.0) ** ((k - par) // 2 + k) for k in ny])
    return par, (1, 1j)[par], eps, int(x).bit_length() - 1


def delete_bit(v, hb):
    return (v & ((1 << hb) - 1)) | ((v >> (hb + 1)) << hb)


def pair_layer(n, x, zs, th, psi):
    """The layer by the pair formula: phi = r(i)/2 on the owner i (bit hb clear), taken from the
    reduced masks on the pair index."""
    par, ph0, eps, hb = pair_terms(x, zs)
    p = np.arange(1 << (n - 1), dtype=np.uint64)
    low = np.uint64((1 << hb) - 1)
    i = (p & low) | ((p & ~low) << np.uint64(1))
    j = i ^ np.uint64(x)
    phi = 0.5 * sum(e * t * signs(n - 1, delete_bit(z, hb)) for e, t, z in zip(eps, th, zs))
    out = np.asarray(psi, dtype=np.complex128).copy()
    out[i] = np.cos(phi) * psi[i] - 1j * ph0 * np.sin(phi) * psi[j]
    out[j] = np.cos(phi) * psi[j] - 1j * np.conj(ph0) * np.sin(phi) * psi[i]
    return out


def pair_gradients(n, x, zs, fwd, bwd):
    """dL/dtheta_k = 1/2 eps_k sum_pairs s_k(p) q, q = Im(ph0 b_i f_j + conj(ph0) b_j f_i)."""
    par, ph0, eps, hb = pair_terms(x, zs)
    p = np.arange(1 << (n - 1), dtype=np.uint64)
    low = np.uint64((1 << hb) - 1)
    i = (p & low) | ((p & ~low) << np.uint64(1))
    j = i ^ np.uint64(x)
    q = (ph0 * bwd[i] * fwd[j] + np.conj(ph0) * bwd[j] * fwd[i]).imag
    return np.array([0.5 * e * np.sum(signs(n - 1, delete_bit(z, hb)) * q)
                     for e, z in zip(eps, zs)])


def xplan(n, x, zs, prec):
    from quantum_differentiable_circuit import pauli_xlayer_plan
    return pauli_xlayer_plan(n, (x, np.asarray(zs, dtype=np.uint64)), prec)


# (n, x, zs): both parities, nY mod 4 taking all four values over the two groups of each x
CASES = [
    (6, 0b001111, [0, 0b000011, 0b001111, 0b110000, 0b110011, 0b000011, 0b111111 & ~0b1100]),  # nY 0 2 4 0 2 2 2
    (6, 0b001111, [0b000001, 0b000111, 0b110010, 0b101110]),                # nY 1 3 1 3
    (8, 0b10010110, [0, 0b00000110, 0b10010110, 0b01101001, 0b11111111, 0b10000010]),  # nY 0 2 4 0 4 2
    (8, 0b10010110, [0b00000010, 0b00010110, 0b11101111, 0b10000000, 0b10000000]),     # nY 1 3 3 1 1
    (3, 0b001, [0, 0b110, 0b010]),
    (3, 0b001, [0b001, 0b111, 0b011]),
    (1, 1, [0]),
    (1, 1, [1, 1]),
]


def test_cases_cover_every_residue():
    seen = set()
    for _, x, zs in CASES:
        seen |= {popcount(x & z) % 4 for z in zs}
        assert len({popcount(x & z) & 1 for z in zs}) == 1
    assert seen == {0, 1, 2, 3}


def test_symbols_present():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import _native
    header = (ROOT / "include" / "qdc" / "pauli.h").read_text()
    for name in ("qdc_pauli_xlayer", "qdc_pauli_xlayer_reverse", "qdc_pauli_xlayer_plan"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.RUNTIME
        for prec in ("f32", "f64"):
            assert hasattr(ctypes.CDLL(str(_native.lib_path(prec))), name), (name, prec)
    for name in ("pauli_xlayer_reverse", "pauli_xlayer_plan", "xlayer_masks", "excitation"):
        assert name in q.__all__ and callable(getattr(q, name))
    assert callable(q.QuantizedTensor.apply_pauli_xlayer)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_pair_formula_is_the_product_of_the_rotations(case):
    n, x, zs = CASES[case]
    rng = np.random.default_rng(100 + case)
    dim = 1 << n
    psi = rng.standard_normal(dim) + 1j * rng.standard_normal(dim)
    th = rng.uniform(-np.pi, np.pi, len(zs))
    want = rotations(n, x, zs, th, psi)
    assert np.abs(pair_layer(n, x, zs, th, psi) - want).max() < 1e-13
    back = rotations(n, x, zs[::-1], th[::-1], psi)  # any order
    assert np.abs(back - want).max() < 1e-13
    # the strings commute, as the parity rule says
    from quantum_differentiable_circuit import PauliSum
    mats = [PauliSum.from_masks(n, [1.0], [x], [z]).to_matrix() for z in zs]
    for a in mats:
        for b in mats:
            assert np.abs(a @ b - b @ a).max() == 0


@pytest.mark.parametrize("case", range(len(CASES)))
def test_r_on_the_partner_and_the_deleted_bit(case):
    """r(j) = (-1)^par r(i), and on owners (bit hb clear) deleting bit hb from i and z leaves the
    sign s_k(i)."""
    n, x, zs = CASES[case]
    par, _, eps, hb = pair_terms(x, zs)
    th = np.random.default_rng(case).uniform(-3, 3, len(zs))
    r = sum(e * t * signs(n, z) for e, t, z in zip(eps, th, zs))
    idx = np.arange(1 << n)
    assert np.allclose(r[idx ^ x], (-1) ** par * r, atol=1e-14)
    owners = idx[(idx >> hb) & 1 == 0]
    for z in zs:
        red = signs(n - 1, delete_bit(z, hb)) if n > 1 else np.ones(1)
        assert np.array_equal(signs(n, z)[owners], red[[delete_bit(int(i), hb) for i in owners]])


@pytest.mark.parametrize("case", range(len(CASES)))
def test_gradient_formula_against_finite_differences(case):
    n, x, zs = CASES[case]
    rng = np.random.default_rng(200 + case)
    dim = 1 << n
    f_in, b = (rng.standard_normal(dim) + 1j * rng.standard_normal(dim) for _ in range(2))
    th = rng.uniform(-np.pi, np.pi, len(zs))
    f_out = rotations(n, x, zs, th, f_in)
    d = pair_gradients(n, x, zs, f_out, b)
    scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f_in)
    loss = lambda t: np.sum(b * rotations(n, x, zs, t, f_in)).real
    h = 1e-5
    for k, z in enumerate(zs):
        assert abs(d[k] - 0.5 * np.sum(b * string_apply(n, x, z, f_out)).imag) <= 1e-13 * scale
        tp, tm = th.copy(), th.copy()
        tp[k] += h
        tm[k] -= h
        assert abs(d[k] - (loss(tp) - loss(tm)) / (2 * h)) <= 1e-8 * scale
    # the reverse step: U(-theta) uncomputes, U^T pulls back (U(theta) at par 0, U(-theta) at 1),
    # and the q-weighted sums do not change under the layer (a split layer is exact)
    par = pair_terms(x, zs)[0]
    from quantum_differentiable_circuit import PauliSum
    u = np.eye(dim, dtype=complex)
    for z, t in zip(zs, th):
        p = PauliSum.from_masks(n, [1.0], [x], [z]).to_matrix()
        u = (np.cos(t / 2) * np.eye(dim) - 1j * np.sin(t / 2) * p) @ u
    assert np.abs(pair_layer(n, x, zs, -th, f_out) - f_in).max() < 1e-13
    pulled = pair_layer(n, x, zs, -th if par else th, b)
    assert np.abs(pulled - u.T @ b).max() < 1e-13
    assert np.abs(pair_gradients(n, x, zs, f_in, pulled) - d).max() <= 1e-13 * scale


def test_xlayer_masks_and_panics():
    import quantum_differentiable_circuit as q
    x, zs = q.xlayer_masks(6, ["X0 Y3", "Y0 X3 Z5", [(0, "x"), (3, "Y"), (1, "Z")]])
    assert x == 0b1001 and list(zs) == [0b1000, 0b100001, 0b1010] and zs.dtype == np.uint64
    assert q.xlayer_masks(6, ["Z1", ""])[0] == 0
    x0, z0 = q.xlayer_masks(6, [])
    assert x0 == 0 and z0.size == 0
    passed = q.xlayer_masks(6, (9, np.array([8, 33], dtype=np.uint64)))
    assert passed[0] == 9 and list(passed[1]) == [8, 33]
    for bad in (["X0", "X1"], ["X0 X1", "X0"], ["Z0", "X0"], ["Y0 Y1", "X0 X1 X2"]):
        with pytest.raises(q.PanicException,
                           match="The strings of a layer must share their X/Y positions."):
            q.xlayer_masks(6, bad)
    for bad in (["X0", "Y0"], ["X0 X1", "X0 Y1"], ["Y0 Y1 Y2", "X0 X1 X2", "X0 Y1 Y2"]):
        with pytest.raises(q.PanicException, match="The strings of a layer must commute."):
            q.xlayer_masks(6, bad)
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        q.xlayer_masks(6, ["X6"])
    with pytest.raises(q.PanicException):
        q.xlayer_masks(6, "X0 X1")  # one string is not a layer
    with pytest.raises(q.PanicException, match="The strings of a layer must commute."):
        q.pauli_xlayer_plan(6, ["X0", "Y0"])
    # the library checks raw masks
    assert xplan(6, 1, [0, 1], "f32") is None
    assert xplan(6, 64, [0], "f32") is None
    assert xplan(6, 1, [64], "f32") is None
    assert xplan(6, 1, [], "f32") is None
    assert xplan(41, 1, [0], "f32") is None


def jw_matrices(n):
    """Dense a_q, q < n: (prod_{r<q} Z_r) |0><1|_q, qubit 0 the least significant index bit."""
    lower = np.array([[0, 1], [0, 0]], dtype=complex)
    zed = np.diag([1.0, -1.0]).astype(complex)
    out = []
    for q in range(n):
        m = np.eye(1, dtype=complex)
        for r in range(n):  # kron from qubit 0 upwards: later factors are more significant
            m = np.kron(lower if r == q else zed if r < q else np.eye(2), m)
        out.append(m)
    return out


@pytest.mark.parametrize("n,occ,virt", [(3, [0], [2]), (4, [2], [1]), (5, [0, 1], [3, 4]),
                                        (5, [3, 0], [1, 4]), (6, [0, 1, 2], [3, 4, 5]),
                                        (6, [4, 0, 3], [5, 1, 2])])
def test_excitation_against_dense_jordan_wigner(n, occ, virt):
    import quantum_differentiable_circuit as q
    a = jw_matrices(n)
    tau = np.eye(1 << n, dtype=complex)
    for p in virt:
        tau = tau @ a[p].conj().T
    for o in occ:
        tau = tau @ a[o]
    g = q.excitation(n, occ, virt)
    assert len(g) == 2 ** (2 * len(occ) - 1)
    assert np.abs(g.to_matrix() - 1j * (tau - tau.conj().T)).max() < 1e-15
    foot = sum(1 << k for k in occ + virt)
    assert np.all(g.xmasks == foot)
    x, zs = q.xlayer_masks(n, (foot, g.zmasks))
    assert len({popcount(x & int(z)) & 1 for z in zs}) == 1
    from quantum_differentiable_circuit.observable import xevolution_masks
    assert xevolution_masks(g)[0] == foot
    number = sum(m.conj().T @ m for m in a)
    assert np.abs(g.to_matrix() @ number - number @ g.to_matrix()).max() < 1e-14
    # qubit value 1 = occupied: the number operator counts the set bits
    assert np.allclose(np.diag(number).real, [popcount(i) for i in range(1 << n)])


def test_excitation_panics():
    import quantum_differentiable_circuit as q
    for occ, virt in (([0], [0]), ([0, 1], [1, 2]), ([0, 0], [1, 2])):
        with pytest.raises(q.PanicException, match="positions must be different."):
            q.excitation(6, occ, virt)
    for occ, virt in (([], []), ([0], [1, 2]), ([0, 1, 2, 3], [4, 5, 6, 7])):
        with pytest.raises(q.PanicException, match="an excitation takes"):
            q.excitation(8, occ, virt)
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        q.excitation(4, [0], [4])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plan(prec):
    lw = L_OF[prec]
    n = lw + 6
    # hb below the span's width, inside it (a slot bit) and above it: the deleted bit is hb, the
    # groups are those of the reduced masks modulo 2^L
    zs = [0, 1 << 2, 1 << 3, 1 << (lw - 1), 1 << lw, 1 << (lw + 1), (1 << 3) | (1 << (lw + 2))]
    for hb in (2, lw - 1, lw + 3):
        x = (1 << hb) | 1
        zx = [z | 1 if z & x else z for z in zs]  # (a Y on qubit hb comes with one on qubit 0)
        p = xplan(n, x, zx, prec)
        red = {delete_bit(z, hb) % (1 << lw) for z in zx}
        assert p["L"] == lw and p["deleted_bit"] == hb and p["groups"] == len(red), hb
        assert (p["forward_launches"], p["reverse_launches"], p["reverse_grad_launches"]) == (1, 1, 1)
    # hand-checked at x = 0b101: Y0 Y2 becomes the low mask 1, Z3 moves to bit 2 (twice), bit L
    # moves into the span, bit L + 1 to bit L (high only: the identity's group)
    assert xplan(n, 0b101, [z | 1 if z & 4 else z for z in zs], prec)["groups"] == 5
    # x = 1: self-paired chunks in f32 (bit 0 dropped, a span of L - 1 bits), neighbour chunks in f64
    # (reduced masks 0, 1, 2, 1, 2^(lw-1): the last is wholly high in the f32 span of lw - 1 bits)
    p = xplan(n, 1, [0, 2, 4, 2, 1 << lw], prec)
    if prec == "f32":
        assert p["L"] == lw - 1 and p["deleted_bit"] is None and p["groups"] == 3
    else:
        assert p["L"] == lw and p["deleted_bit"] == 0 and p["groups"] == 4
    assert xplan(n, 1, [1, 3, 1 | (1 << lw)], prec)["groups"] == (2 if prec == "f32" else 3)
    # x = 0: the diagonal layer's plan
    from quantum_differentiable_circuit import pauli_layer_plan
    d = pauli_layer_plan(n, np.array(zs, dtype=np.uint64), prec)
    p = xplan(n, 0, zs, prec)
    assert p["deleted_bit"] is None and p["L"] == lw and p["groups"] == d["groups"]
    # launches: 128 terms per streaming launch, 32 per reducing launch
    rng = np.random.default_rng(5)
    for k, fwd, grad in ((32, 1, 1), (33, 1, 2), (128, 1, 4), (129, 2, 5), (130, 2, 5), (70, 1, 3)):
        z = [int(v) & ~0b11 for v in rng.integers(0, 1 << n, size=k)]  # nY = 0
        for x in (0b11, 0):
            p = xplan(n, x, z, prec)
            assert (p["forward_launches"], p["reverse_launches"], p["reverse_grad_launches"]) == \
                (fwd, fwd, grad), (k, x)
    from quantum_differentiable_circuit import _native
    lib = _native.load(prec)
    z1 = (ctypes.c_ulonglong * 1)(0)
    assert lib.qdc_pauli_xlayer_plan(1, z1, 1, 12, None) == ctypes.c_size_t(-1).value
    assert lib.qdc_pauli_xlayer_plan(1, None, 1, 12, (ctypes.c_uint * 6)()) == \
        ctypes.c_size_t(-1).value


def accuracy_case():
    """The accuracy test's layer: n = 12, x = 0b1111, 64 strings X0 X1 X2 X3 Z^{z'} with z' over
    subsets of qubits 4..11, theta uniform in [-pi, pi]."""
    rng = np.random.default_rng(1264)
    zs = [int(z) << 4 for z in rng.choice(256, size=64, replace=False)]
    th = rng.uniform(-np.pi, np.pi, 64)
    return 12, 0b1111, zs, th, rng


def long_double_reference(n, x, zs, th, psi):
    par, ph0, eps, hb = pair_terms(x, zs)
    p = np.arange(1 << (n - 1), dtype=np.uint64)
    low = np.uint64((1 << hb) - 1)
    i = (p & low) | ((p & ~low) << np.uint64(1))
    j = i ^ np.uint64(x)
    phi = np.zeros(p.size, np.longdouble)
    for e, t, z in zip(eps, th, zs):
        phi += np.longdouble(0.5) * np.longdouble(e * t) * signs(n - 1, delete_bit(z, hb)).astype(np.longdouble)
    psi = psi.astype(np.clongdouble)
    out = psi.copy()
    out[i] = np.cos(phi) * psi[i] - 1j * ph0 * np.sin(phi) * psi[j]
    out[j] = np.cos(phi) * psi[j] - 1j * np.conj(ph0) * np.sin(phi) * psi[i]
    return out


def test_fixed_point_phase_emulation_f32():
    """f32 emulation of the accuracy test of tests/test_gpu_pauli_xlayer.py: the layer with its
    phase summed in 2^-32 turns, one float32 sincos per pair and float32 mixing, against 64
    sequential float32 rotations, both measured against the long-double reference.  Measured here:
    the layer's error is 0.18 times the rotations' (must be below 1); a phase summed in float32
    gives 3.5 times."""
    n, x, zs, th, rng = accuracy_case()
    dim = 1 << n
    psi = (rng.standard_normal(dim) + 1j * rng.standard_normal(dim)).astype(np.complex64)
    psi /= np.float32(np.linalg.norm(psi))
    ref = long_double_reference(n, x, zs, th, psi)
    par, ph0, eps, hb = pair_terms(x, zs)
    assert par == 0
    p = np.arange(1 << (n - 1), dtype=np.uint64)
    low = np.uint64((1 << hb) - 1)
    i = (p & low) | ((p & ~low) << np.uint64(1))
    j = i ^ np.uint64(x)
    sg = [signs(n - 1, delete_bit(z, hb)) for z in zs]

    def mixed(c, s):
        out = psi.copy()
        mi = (-1j * psi[j]).astype(np.complex64)
        mj = (-1j * psi[i]).astype(np.complex64)
        out[i] = (c * psi[i] + s * mi).astype(np.complex64)
        out[j] = (c * psi[j] + s * mj).astype(np.complex64)
        return out

    # fixed point: t_k = round(eps theta / 4 pi 2^32) mod 2^32, exact signed sum, one conversion
    acc = np.zeros(p.size, dtype=np.int64)
    for e, t, s in zip(eps, th, sg):
        tk = int(round((e * t / (4 * np.pi)) % 1.0 * 2.0 ** 32)) % (1 << 32)
        acc = (acc + s.astype(np.int64) * tk) % (1 << 32)
    signed = np.where(acc >= 1 << 31, acc - (1 << 32), acc)
    xf = (signed.astype(np.float32) * np.float32(2.0 ** -31)).astype(np.float64)  # phi / pi
    fixed = mixed(np.cos(np.pi * xf).astype(np.float32), np.sin(np.pi * xf).astype(np.float32))
    # the phase summed in float32 instead
    phi32 = np.zeros(p.size, np.float32)
    for e, t, s in zip(eps, th, sg):
        phi32 += np.float32(0.5 * e * t) * s.astype(np.float32)
    working = mixed(np.cos(phi32.astype(np.float64)).astype(np.float32),
                    np.sin(phi32.astype(np.float64)).astype(np.float32))
    # 64 sequential rotations in float32, cos and sin rounded once each
    seq = psi.copy()
    full = [signs(n, z) for z in zs]
    idx = np.arange(dim, dtype=np.uint64) ^ np.uint64(x)
    for t, z, s in zip(th, zs, full):
        ph = np.complex64((1, 1j, -1, -1j)[popcount(x & z) % 4])
        pp = (ph * s[idx].astype(np.float32) * seq[idx]).astype(np.complex64)
        seq = (np.float32(np.cos(t / 2)) * seq
               + (np.complex64(-1j) * np.float32(np.sin(t / 2))) * pp).astype(np.complex64)
    err = [float(np.sqrt(np.sum(np.abs(v.astype(np.clongdouble) - ref) ** 2)))
           for v in (fixed, working, seq)]
    print(f"fixed point {err[0]:.3e}, float32 phase {err[1]:.3e}, rotations {err[2]:.3e}: "
          f"ratios {err[0] / err[2]:.2f}, {err[1] / err[2]:.2f}")
    assert err[0] < err[2]
    assert err[0] < err[1]

"""Pauli layers with a shared X/Y footprint on the GPU (include/qdc/pauli.h: qdc_pauli_xlayer,
qdc_pauli_xlayer_reverse; csrc/qdc_paulixlayer.hpp).

Expected values come from the host definition in complex128 on the build-precision inputs: psi <-
cos(theta_k/2) psi - i sin(theta_k/2) P_k psi for each k by the index rule (pinned to the pair
formula by tests/test_pauli_xlayer_cpu.py).  Tolerances are the rotation tests': normrel <= 1e-5
(f32) / 1e-12 (f64) for a state, |dtheta_k - ref| <= TOL 1/2 ||bwd|| ||fwd|| for a gradient."""
import ctypes as C

import numpy as np
import pytest

from floors import normrel
from oracle import oracle as O
from test_gpu_dense_grad import DT, TOL, tensor
from test_pauli_xlayer_cpu import (accuracy_case, long_double_reference, popcount, rotations,
                                   string_apply)

pytestmark = pytest.mark.gpu
SIZES = ["1", "2", "3", "L-1", "L", "L+1", "L+3"]


def span_bits(prec):
    import quantum_differentiable_circuit as q
    return q.pauli_layer_plan(1, ["Z0"], prec)["L"]


def size_of(name, lw):
    return {"L-1": lw - 1, "L": lw, "L+1": lw + 1, "L+3": lw + 3}.get(name) or int(name)


def x_masks_for(n, lw):
    """Footprints whose highest bit is bit 0 (self-paired chunks in f32, neighbour chunks in f64),
    bit 1, a thread bit, each slot bit (L - 2, L - 1), bit L and the top bit, and one that
    straddles the span; those that fit n qubits."""
    top = n - 1
    xs = [1, 0b10, 0b11, (1 << 4) | 0b101, (1 << (lw - 2)) | 0b11, (1 << (lw - 1)) | 0b1001,
          (1 << lw) | 0b110, (1 << top) | 0b11, 1 << top,
          (1 << (lw + 1)) | (1 << (lw - 1)) | (1 << 5) | 1]
    out = []
    for x in xs:
        if x >> n == 0 and x not in out:
            out.append(x)
    return out


def z_masks_for(n, lw, x, par):
    """For one footprint and one parity of nY: low-only, high-only and mixed masks around a span of
    2^lw, the deleted qubit (the highest of x) with a Y (z bit set) and with an X, the empty z
    (par 0), a duplicate, a weight-n string, and nY = 0 .. 3 as far as x has the bits.  A mask of
    the other parity gets a Y on the lowest qubit of x."""
    top, hb = n - 1, x.bit_length() - 1
    full = (1 << n) - 1
    bits = [b for b in range(n) if x >> b & 1]
    cand = [0, 1, full, 1 | (1 << top), 0b110, (1 << (lw - 1)) | (1 << (lw - 2)), 1 << (lw - 1),
            0b10 | (1 << (lw - 2)), 1 << lw, (1 << lw) | (1 << top), 0b1000 | (1 << lw),
            1 | (1 << (lw - 1)) | (1 << top), (1 << (lw + 1)) | (1 << (lw + 2)), 1 << top,
            1 << hb, (1 << hb) | 0b100 | (1 << (lw + 1)), full & ~x,
            sum(1 << b for b in bits[:2]), sum(1 << b for b in bits[:3]), x]
    zs = []
    for z in cand:
        if z >> n:
            continue
        if popcount(x & z) & 1 != par:
            z ^= 1 << bits[0]
        zs.append(z)
    zs.append(zs[1])  # a duplicate
    want = {r % 4 for r in range(par, len(bits) + 1, 2)}
    assert {popcount(x & z) % 4 for z in zs} == want, (x, par)
    assert any((x | z) == full for z in zs)
    return zs


def masks(x, zs):
    return x, np.array(zs, dtype=np.uint64)


def check_state(prec, t, want, what):
    got = t.get_cpu_state_copy()
    err = normrel(got, want)
    print(f"{prec} {what}: normrel {err:.2e}")
    assert err <= TOL[prec], what
    return got


def gradients_ref(n, x, zs, f_out, b):
    return np.array([0.5 * np.sum(b * string_apply(n, x, z, f_out)).imag for z in zs])


def check_layer(prec, n, x, zs, th, f_in, b_in):
    """apply, then the three forms of the reverse step, against the host definition."""
    import quantum_differentiable_circuit as q
    par = popcount(x & zs[0]) & 1
    what = f"n={n} x={x:#b} par={par} K={len(zs)}"
    m = masks(x, zs)
    f_out = rotations(n, x, zs, th, f_in)
    tf = tensor(prec, f_in)
    tf.apply_pauli_xlayer(m, th)
    check_state(prec, tf, f_out, what + " apply")
    t1, t2 = tf.clone(), tf.clone()
    tb, tb1 = tensor(prec, b_in), tensor(prec, b_in)
    d = q.pauli_xlayer_reverse(tf, tb, m, th)
    assert isinstance(d, np.ndarray) and d.dtype == np.float64 and d.shape == (len(zs),)
    scale = 0.5 * np.linalg.norm(b_in) * np.linalg.norm(f_in)
    want = gradients_ref(n, x, zs, f_out, b_in)  # fwd as the reverse receives it
    print(f"{prec} {what}: max gradient error / scale {np.abs(d - want).max() / scale:.2e}")
    assert np.abs(d - want).max() <= TOL[prec] * scale, what
    f_back = check_state(prec, tf, f_in, what + " uncompute")
    # U^T: P^T = (-1)^nY P
    b_back = check_state(prec, tb, rotations(n, x, zs, -th if par else th, b_in),
                         what + " pull-back")
    # a constant layer, and no cotangent yet: the same states, zeros
    z1 = q.pauli_xlayer_reverse(t1, tb1, m, th, want_grad=False)
    assert z1.shape == d.shape and not z1.any()
    assert normrel(t1.get_cpu_state_copy(), f_back) <= TOL[prec], what
    assert normrel(tb1.get_cpu_state_copy(), b_back) <= TOL[prec], what
    z2 = q.pauli_xlayer_reverse(t2, None, m, th)
    assert z2.shape == d.shape and not z2.any()
    assert normrel(t2.get_cpu_state_copy(), f_back) <= TOL[prec], what
    return want, scale


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_forward_and_reverse(prec, n):
    """Every footprint class of x_masks_for, both parities of nY: forward, uncompute only, the
    constant layer and the gradients; bwd is not normalised (norm^2 about 2)."""
    lw = span_bits(prec)
    n = size_of(n, lw)
    rng = np.random.default_rng(1600 + n)
    f = O.random_state(rng, n).astype(DT[prec]).astype(np.complex128)
    b = O.random_state(rng, n, normalise=False).astype(DT[prec]).astype(np.complex128)
    for x in x_masks_for(n, lw):
        for par in (0, 1):
            zs = z_masks_for(n, lw, x, par)
            th = rng.uniform(-3, 3, len(zs))
            check_layer(prec, n, x, zs, th, f, b)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_c_entry_point_adds_into_dtheta(prec):
    import quantum_differentiable_circuit as q
    lw = span_bits(prec)
    n = lw + 1
    rng = np.random.default_rng(1700)
    f = O.random_state(rng, n).astype(DT[prec]).astype(np.complex128)
    b = O.random_state(rng, n, normalise=False).astype(DT[prec]).astype(np.complex128)
    x = (1 << lw) | 0b110
    zs = z_masks_for(n, lw, x, 1)
    th = rng.uniform(-3, 3, len(zs))
    f_out = rotations(n, x, zs, th, f)
    want = gradients_ref(n, x, zs, f_out, b)
    scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f)
    lib = q._native.load(prec)
    tf, tb = tensor(prec, f_out), tensor(prec, b)
    start = np.arange(1.0, len(zs) + 1.0)
    d = start.copy()
    za = np.array(zs, dtype=np.uint64)
    ull, dbl = C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
    assert lib.qdc_pauli_xlayer_reverse(tf._p, tb._p, x, za.ctypes.data_as(ull),
                                        th.ctypes.data_as(dbl), len(zs), n,
                                        d.ctypes.data_as(dbl)) is None
    assert np.abs(d - start - want).max() <= TOL[prec] * scale and np.all(d != start)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_one_string_is_the_rotation(prec):
    import quantum_differentiable_circuit as q
    n = 12
    rng = np.random.default_rng(1800)
    f = O.random_state(rng, n).astype(DT[prec])
    b = O.random_state(rng, n).astype(DT[prec])
    scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f)
    for ops in ("X0", "Y0", "X3 Y5 Z7", "Y1 Y2 Y11 Z0", "X0 Y1 Y2 Y3 Z11"):
        th = float(rng.uniform(-3, 3))
        tl, tr = tensor(prec, f), tensor(prec, f)
        tl.apply_pauli_xlayer([ops], [th])
        tr.apply_pauli_rotation(ops, th)
        assert normrel(tl.get_cpu_state_copy(), tr.get_cpu_state_copy()) <= TOL[prec], ops
        bl, br = tensor(prec, b), tensor(prec, b)
        d = q.pauli_xlayer_reverse(tl, bl, [ops], [th])
        w = q.pauli_rot_reverse(tr, br, ops, th)
        assert abs(d[0] - w) <= TOL[prec] * scale, ops
        assert normrel(tl.get_cpu_state_copy(), tr.get_cpu_state_copy()) <= TOL[prec], ops
        assert normrel(bl.get_cpu_state_copy(), br.get_cpu_state_copy()) <= TOL[prec], ops


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_z_strings_take_the_diagonal_layer_bit_for_bit(prec):
    import quantum_differentiable_circuit as q
    lw = span_bits(prec)
    n = lw + 1
    rng = np.random.default_rng(1900)
    f = O.random_state(rng, n).astype(DT[prec])
    b = O.random_state(rng, n).astype(DT[prec])
    zs = np.array([0, 1, (1 << n) - 1, 1 << lw, 0b110 | (1 << (lw - 1)), 1], dtype=np.uint64)
    th = rng.uniform(-3, 3, zs.size)
    tx, td = tensor(prec, f), tensor(prec, f)
    tx.apply_pauli_xlayer((0, zs), th)
    td.apply_pauli_layer(zs, th)
    assert np.array_equal(tx.get_cpu_state_copy(), td.get_cpu_state_copy())
    assert not np.array_equal(tx.get_cpu_state_copy(), f)
    bx, bd = tensor(prec, b), tensor(prec, b)
    dx = q.pauli_xlayer_reverse(tx, bx, (0, zs), th)
    dd = q.pauli_layer_reverse(td, bd, zs, th)
    assert np.array_equal(dx, dd) and np.any(dx != 0.0)
    assert np.array_equal(tx.get_cpu_state_copy(), td.get_cpu_state_copy())
    assert np.array_equal(bx.get_cpu_state_copy(), bd.get_cpu_state_copy())
    tx.apply_pauli_xlayer(["Z0 Z3", ""], [0.3, 0.4])
    td.apply_pauli_layer(["Z0 Z3", ""], [0.3, 0.4])
    assert np.array_equal(tx.get_cpu_state_copy(), td.get_cpu_state_copy())


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_splitting(prec):
    """More terms than one launch holds at n = L + 1: K = 130 forward (two streaming launches),
    K = 70 with gradients (three reducing launches), the definition's state and gradients, and the
    plan's launch counts under the profile names, 2 S / 4 S bytes each."""
    import quantum_differentiable_circuit as q
    lw = span_bits(prec)
    n = lw + 1
    rng = np.random.default_rng(2000)
    x = (1 << lw) | (1 << 3) | 1
    f = O.random_state(rng, n).astype(DT[prec]).astype(np.complex128)
    b = O.random_state(rng, n, normalise=False).astype(DT[prec]).astype(np.complex128)
    s = float(np.dtype(DT[prec]).itemsize << n)

    def draw(k, par):
        zs = [int(z) for z in rng.integers(0, 1 << n, size=k)]
        return [z ^ 1 if popcount(x & z) & 1 != par else z for z in zs]

    zs = draw(130, 0)
    th = rng.uniform(-3, 3, len(zs))
    plan = q.pauli_xlayer_plan(n, masks(x, zs), prec)
    assert plan["forward_launches"] == 2 == plan["reverse_launches"]
    assert plan["reverse_grad_launches"] == 5 and plan["deleted_bit"] == lw
    tf = tensor(prec, f)
    q.primitives_profile(True, prec)
    try:
        tf.apply_pauli_xlayer(masks(x, zs), th)
        fwd_stats = q.primitives_profile_collect(prec)
        q.primitives_profile(True, prec)
        q.pauli_xlayer_reverse(tf, None, masks(x, zs), th)
        unc_stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    assert fwd_stats["pauli_xlayer"]["launches"] == 2
    assert fwd_stats["pauli_xlayer"]["algo_bytes"] == 2 * 2 * s
    assert unc_stats["pauli_xlayer_rev"]["launches"] == 2
    check_state(prec, tf, f, "K=130 round trip")
    tf.apply_pauli_xlayer(masks(x, zs), th)
    check_state(prec, tf, rotations(n, x, zs, th, f), "K=130 forward")

    zs = draw(70, 1)
    th = rng.uniform(-3, 3, len(zs))
    plan = q.pauli_xlayer_plan(n, masks(x, zs), prec)
    assert (plan["forward_launches"], plan["reverse_grad_launches"]) == (1, 3)
    check_layer(prec, n, x, zs, th, f, b)
    tf, tb = tensor(prec, f), tensor(prec, b)
    q.primitives_profile(True, prec)
    try:
        q.pauli_xlayer_reverse(tf, tb, masks(x, zs), th)
        grad_stats = q.primitives_profile_collect(prec)
        q.primitives_profile(True, prec)
        q.pauli_xlayer_reverse(tf, tb, masks(x, zs), th, want_grad=False)
        const_stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    assert grad_stats["pauli_xlayer_rev"]["launches"] == 3
    assert grad_stats["pauli_xlayer_rev"]["algo_bytes"] == 3 * 4 * s
    assert const_stats["pauli_xlayer_rev"]["launches"] == 1
    assert "pauli_xlayer" not in grad_stats and "pauli_layer" not in grad_stats


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_grids_and_determinism(monkeypatch, prec):
    """n = L + 3: four spans of pairs.  Three blocks walk 2, 1 and 1 of them and leave the bits of
    the default grid (every pair's phase is an exact integer sum); the same call twice returns the
    same bits, gradients included; one block adds the spans in another order."""
    import quantum_differentiable_circuit as q
    lw = span_bits(prec)
    n = lw + 3
    rng = np.random.default_rng(2100)
    f, b = (O.random_state(rng, n).astype(DT[prec]) for _ in range(2))
    x = (1 << (lw + 1)) | (1 << (lw - 1)) | (1 << 5) | 1
    zs = z_masks_for(n, lw, x, 0)
    m = masks(x, zs)
    th = rng.uniform(-3, 3, len(zs))
    runs = []
    for grid in (None, "3", "3", "1"):
        if grid is None:
            monkeypatch.delenv("QDC_PAULI_GRID", raising=False)
        else:
            monkeypatch.setenv("QDC_PAULI_GRID", grid)
        tf, tb = tensor(prec, f), tensor(prec, b)
        tf.apply_pauli_xlayer(m, th)
        applied = tf.get_cpu_state_copy()
        d = q.pauli_xlayer_reverse(tf, tb, m, th)
        runs.append((applied, tf.get_cpu_state_copy(), tb.get_cpu_state_copy(), d))
    monkeypatch.delenv("QDC_PAULI_GRID", raising=False)
    for r in runs[1:]:
        assert all(np.array_equal(a, c) for a, c in zip(r[:3], runs[0][:3]))
    assert np.array_equal(runs[1][3], runs[2][3]) and np.any(runs[1][3] != 0.0)
    scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f)
    assert np.abs(runs[1][3] - runs[0][3]).max() <= TOL[prec] * scale
    assert np.abs(runs[3][3] - runs[0][3]).max() <= TOL[prec] * scale
    # the knob took effect
    assert np.any(runs[3][3] != runs[1][3])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_accuracy_against_the_rotations(prec):
    """n = 12, x = 0b1111, 64 strings X0 X1 X2 X3 Z^{z'} with z' over subsets of qubits 4..11,
    theta uniform in [-pi, pi]: the layer's 2-norm error against a long-double reference is at most
    1.5 times that of the 64 sequential apply_pauli_rotation calls on the same input (the bound of
    tests/test_gpu_pauli_layer.py: the layer rounds once where the rotations round 64 times, and
    the margin covers the sincos).  CPU emulation in f32
    (tests/test_pauli_xlayer_cpu.py::test_fixed_point_phase_emulation_f32): 0.18 times for the
    fixed-point phase, 3.5 times for a phase summed in the working precision."""
    n, x, zs, th, rng = accuracy_case()
    psi = O.random_state(rng, n).astype(DT[prec])
    ref = long_double_reference(n, x, zs, th, psi)
    tl, ts = tensor(prec, psi), tensor(prec, psi)
    tl.apply_pauli_xlayer(masks(x, zs), th)
    for z, t in zip(zs, th):
        ops = [(b, "X") for b in range(4)] + [(b, "Z") for b in range(4, n) if z >> b & 1]
        ts.apply_pauli_rotation(ops, t)
    err = [float(np.sqrt(np.sum(np.abs(t.get_cpu_state_copy().astype(np.clongdouble) - ref) ** 2)))
           for t in (tl, ts)]
    print(f"{prec}: layer error {err[0]:.3e}, sequential rotations {err[1]:.3e}, "
          f"ratio {err[0] / err[1]:.2f}")
    assert err[0] <= 1.5 * err[1]


def test_panics():
    import quantum_differentiable_circuit as q
    t = q.QuantizedTensor.new_standard(6, precision="f32")
    u = q.QuantizedTensor.new_standard(6, precision="f32")
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        t.apply_pauli_xlayer(["X0", "X0 Z6"], [0.1, 0.2])
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        q.pauli_xlayer_reverse(t, u, [[(7, "X")]], [0.1])
    share = "The strings of a layer must share their X/Y positions."
    for bad in (["X1", "X2"], ["X0 X1", "Z0 X1"]):
        with pytest.raises(q.PanicException, match=share):
            t.apply_pauli_xlayer(bad, [0.1] * len(bad))
        with pytest.raises(q.PanicException, match=share):
            q.pauli_xlayer_reverse(t, u, bad, [0.1] * len(bad))
    for bad in (["X1", "Y1"], ["X0 X1 Z3", "X0 Y1"]):
        with pytest.raises(q.PanicException, match="The strings of a layer must commute."):
            t.apply_pauli_xlayer(bad, [0.1] * len(bad))
        with pytest.raises(q.PanicException, match="The strings of a layer must commute."):
            q.pauli_xlayer_reverse(t, u, bad, [0.1] * len(bad))
    with pytest.raises(q.PanicException, match="The layer has no terms."):
        t.apply_pauli_xlayer([], [])
    with pytest.raises(q.PanicException, match="The layer has no terms."):
        q.pauli_xlayer_reverse(t, u, (3, np.zeros(0, np.uint64)), [])
    for bad in ([0.1], [0.1, 0.2, 0.3], [[0.1, 0.2]], 0.5):
        with pytest.raises(q.PanicException, match="one angle per string"):
            t.apply_pauli_xlayer(["X0", "X0 Z1"], bad)
        with pytest.raises(q.PanicException, match="one angle per string"):
            q.pauli_xlayer_reverse(t, u, ["X0", "X0 Z1"], bad)
    with pytest.raises(q.PanicException, match="must be real"):
        t.apply_pauli_xlayer(["X0"], [0.1 + 0.2j])
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
            t.apply_pauli_xlayer(["X0", "X0 Z1"], [0.1, bad])
        with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
            q.pauli_xlayer_reverse(t, u, ["X0", "X0 Z1"], [bad, 0.1])
    with pytest.raises(q.PanicException, match="fwd and bwd must be different states."):
        q.pauli_xlayer_reverse(t, t, ["X1"], [0.1])
    with pytest.raises(q.PanicException, match="fwd and bwd have different lengths"):
        q.pauli_xlayer_reverse(t, q.QuantizedTensor.new_standard(7, precision="f32"), ["X1"], [0.1])
    # the C ABI validates too
    lib = q._native.load("f32")
    ull, dbl = C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
    z = np.array([4, 64], dtype=np.uint64)
    th = np.array([0.1, 0.2])
    d = np.zeros(2)
    zp, tp, dp = z.ctypes.data_as(ull), th.ctypes.data_as(dbl), d.ctypes.data_as(dbl)
    oob = b"pos is out of the bound."
    assert lib.qdc_pauli_xlayer(t._p, 3, zp, tp, 2, 6) == oob
    assert lib.qdc_pauli_xlayer_reverse(t._p, u._p, 3, zp, tp, 2, 6, dp) == oob
    z[1] = 8
    assert lib.qdc_pauli_xlayer(t._p, 64, zp, tp, 2, 6) == oob
    assert lib.qdc_pauli_xlayer_reverse(t._p, u._p, 64, zp, tp, 2, 6, dp) == oob
    assert lib.qdc_pauli_xlayer(t._p, 3, zp, tp, 0, 6) == b"The layer has no terms."
    assert lib.qdc_pauli_xlayer_reverse(t._p, u._p, 3, zp, tp, 0, 6, dp) == b"The layer has no terms."
    assert lib.qdc_pauli_xlayer(t._p, 3, None, tp, 2, 6) == b"The layer has no masks."
    assert lib.qdc_pauli_xlayer(t._p, 3, zp, None, 2, 6) == b"The layer has no angles."
    assert lib.qdc_pauli_xlayer_reverse(t._p, u._p, 3, zp, None, 2, 6, dp) == b"The layer has no angles."
    z[1] = 1  # nY 0 and 1
    commute = b"The strings of a layer must commute."
    assert lib.qdc_pauli_xlayer(t._p, 3, zp, tp, 2, 6) == commute
    assert lib.qdc_pauli_xlayer_reverse(t._p, u._p, 3, zp, tp, 2, 6, dp) == commute
    z[1] = 3
    th[1] = float("nan")
    assert lib.qdc_pauli_xlayer(t._p, 3, zp, tp, 2, 6) == b"Pauli coefficients must be finite."
    assert lib.qdc_pauli_xlayer_reverse(t._p, u._p, 3, zp, tp, 2, 6, dp) == \
        b"Pauli coefficients must be finite."
    th[1] = 0.2
    assert lib.qdc_pauli_xlayer_reverse(t._p, t._p, 3, zp, tp, 2, 6, dp) == \
        b"fwd and bwd must be different states."
    assert lib.qdc_pauli_xlayer_reverse(t._p, None, 3, zp, tp, 2, 6, dp) == \
        b"A gradient needs a bwd state."
    assert b"supported range" in lib.qdc_pauli_xlayer(t._p, 3, zp, tp, 2, 41)
    assert not d.any()
    # nothing above touched the state
    psi = np.zeros(64, np.complex64)
    psi[0] = 1
    assert np.array_equal(t.get_cpu_state_copy(), psi)
    assert np.array_equal(u.get_cpu_state_copy(), psi)

"""Diagonal Pauli layers exp(-i/2 sum_k theta_k Z^{z_k}) on the GPU (include/qdc/pauli.h:
qdc_pauli_layer, qdc_pauli_layer_reverse; csrc/qdc_paulilayer.hpp).

Expected values come from the host definition in complex128 on the build-precision inputs:
(U psi)[i] = e^{-i phi(i)} psi[i], phi(i) = 1/2 sum_k theta_k (-1)^popcount(i & z_k) (pinned to the
product of the rotations by tests/test_pauli_layer_cpu.py).  Tolerances are the rotation tests':
normrel <= 1e-5 (f32) / 1e-12 (f64) for a state, |dtheta_k - ref| <= TOL 1/2 ||bwd|| ||fwd|| for a
gradient."""
import ctypes as C

import numpy as np
import pytest

from floors import normrel
from oracle import oracle as O
from test_gpu_dense_grad import DT, TOL, states, tensor

pytestmark = pytest.mark.gpu
GCAP = 32  # terms of a reducing launch


def span_bits(prec):
    import quantum_differentiable_circuit as q
    return q.pauli_layer_plan(1, ["Z0"], prec)["L"]


def zstr(z):
    return [(b, "Z") for b in range(int(z).bit_length()) if int(z) >> b & 1]


def signs(n, z):
    """s(i) = (-1)^popcount(i & z) for every index, float64."""
    x = np.arange(1 << n, dtype=np.uint64) & np.uint64(z)
    for sh in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(sh)
    return 1.0 - 2.0 * (x & np.uint64(1)).astype(np.float64)


def phase(n, zs, thetas, dtype=np.float64):
    phi = np.zeros(1 << n, dtype)
    for z, t in zip(zs, thetas):
        phi += dtype(0.5) * dtype(t) * signs(n, z).astype(dtype)
    return phi


def layer_masks_for(n, lw):
    """Low-only, high-only and mixed terms around a span of 2^lw amplitudes (those that fit n
    qubits), the identity, a weight-n string, a duplicate; the slot bits (0 in f32, lw - 2 and
    lw - 1) and the thread bits both occur."""
    top = n - 1
    zs = [0, 1, (1 << n) - 1, 1 | (1 << top), 1, 0b110, (1 << (lw - 1)) | (1 << (lw - 2)),
          1 << (lw - 1), 0b10 | (1 << (lw - 2)), 1 << lw, (1 << lw) | (1 << top), 0b1000 | (1 << lw),
          1 | (1 << (lw - 1)) | (1 << top), (1 << (lw + 1)) | (1 << (lw + 2)), 1 << top]
    return [z for z in zs if z >> n == 0]


def check_state(prec, t, want, what):
    got = t.get_cpu_state_copy()
    err = normrel(got, want)
    print(f"{prec} {what}: normrel {err:.2e}")
    assert err <= TOL[prec], what
    return got


def size_of(name, lw):
    return {"L-1": lw - 1, "L": lw, "L+1": lw + 1, "L+3": lw + 3}.get(name) or int(name)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", ["1", "2", "3", "L-1", "L", "L+1", "L+3"])
def test_forward(prec, n):
    lw = span_bits(prec)
    n = size_of(n, lw)
    rng = np.random.default_rng(600 + n)
    psi = O.random_state(rng, n).astype(DT[prec])
    t = tensor(prec, psi)
    zs = layer_masks_for(n, lw)
    th = rng.uniform(-3, 3, len(zs))
    t.apply_pauli_layer([zstr(z) for z in zs], th)
    want = np.exp(-1j * phase(n, zs, th)) * psi.astype(np.complex128)
    check_state(prec, t, want, f"n={n} K={len(zs)}")
    # one term is the rotation, the identity string the global phase
    t2 = tensor(prec, psi)
    t2.apply_pauli_layer([""], [1.1])
    check_state(prec, t2, np.exp(-0.55j) * psi.astype(np.complex128), "global phase")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_grids_and_determinism(monkeypatch, prec):
    """n = L + 3: eight spans.  Three blocks walk 3, 3 and 2 of them and leave the bits of the
    default grid (every amplitude's phase is an exact integer sum); the same call twice returns
    the same bits, gradients included."""
    import quantum_differentiable_circuit as q
    lw = span_bits(prec)
    n = lw + 3
    rng = np.random.default_rng(700)
    f, b = (O.random_state(rng, n).astype(DT[prec]) for _ in range(2))
    zs = layer_masks_for(n, lw)
    strings = [zstr(z) for z in zs]
    th = rng.uniform(-3, 3, len(zs))
    runs = []
    for grid in (None, "3", "3", "1"):
        if grid is None:
            monkeypatch.delenv("QDC_PAULI_GRID", raising=False)
        else:
            monkeypatch.setenv("QDC_PAULI_GRID", grid)
        tf, tb = tensor(prec, f), tensor(prec, b)
        tf.apply_pauli_layer(strings, th)
        applied = tf.get_cpu_state_copy()
        d = q.pauli_layer_reverse(tf, tb, strings, th)
        runs.append((applied, tf.get_cpu_state_copy(), tb.get_cpu_state_copy(), d))
    monkeypatch.delenv("QDC_PAULI_GRID", raising=False)
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r[:3], runs[0][:3]))
    assert np.array_equal(runs[1][3], runs[2][3]) and np.any(runs[1][3] != 0.0)
    scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f)
    assert np.abs(runs[1][3] - runs[0][3]).max() <= TOL[prec] * scale
    assert np.abs(runs[3][3] - runs[0][3]).max() <= TOL[prec] * scale
    # the knob took effect: one block adds the eight spans in another order than three do
    assert np.any(runs[3][3] != runs[1][3])


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_accuracy_against_the_rotations(prec):
    """n = 12, the 66 ZZ pairs, theta uniform in [-pi, pi]: the layer's 2-norm error against a
    long-double reference is at most 1.5 times that of 66 apply_pauli_rotation calls on the same
    input.  (CPU emulation: 0.3 times for the fixed-point phase, more than 4 times for a phase
    summed in the working precision.)"""
    n = 12
    rng = np.random.default_rng(1266)
    zs = [(1 << i) | (1 << j) for i in range(n) for j in range(i)]
    th = rng.uniform(-np.pi, np.pi, len(zs))
    psi = O.random_state(rng, n).astype(DT[prec])
    phi = phase(n, zs, th, np.longdouble)
    ref = (np.cos(phi) - 1j * np.sin(phi)) * psi.astype(np.clongdouble)
    tl, ts = tensor(prec, psi), tensor(prec, psi)
    tl.apply_pauli_layer([zstr(z) for z in zs], th)
    for z, t in zip(zs, th):
        ts.apply_pauli_rotation(zstr(z), t)
    err = [float(np.sqrt(np.sum(np.abs(t.get_cpu_state_copy().astype(np.clongdouble) - ref) ** 2)))
           for t in (tl, ts)]
    print(f"{prec}: layer error {err[0]:.3e}, sequential rotations {err[1]:.3e}, "
          f"ratio {err[0] / err[1]:.2f}")
    assert err[0] <= 1.5 * err[1]


def check_reverse(prec, n, zs, th, f_in, b_in, tf_in=None):
    """apply, then the three forms of the reverse step, against the host definition."""
    import quantum_differentiable_circuit as q
    what = f"n={n} K={len(zs)}"
    strings = [zstr(z) for z in zs]
    e = np.exp(-1j * phase(n, zs, th))
    tf = tf_in.clone() if tf_in is not None else tensor(prec, f_in)
    tf.apply_pauli_layer(strings, th)
    check_state(prec, tf, e * f_in, what + " apply")
    t1, t2 = tf.clone(), tf.clone()
    tb, tb1 = tensor(prec, b_in), tensor(prec, b_in)
    d = q.pauli_layer_reverse(tf, tb, strings, th)
    assert isinstance(d, np.ndarray) and d.dtype == np.float64 and d.shape == (len(zs),)
    scale = 0.5 * np.linalg.norm(b_in) * np.linalg.norm(f_in)
    want = np.array([0.5 * np.sum(signs(n, z) * b_in * (e * f_in)).imag for z in zs])  # fwd as received
    print(f"{prec} {what}: max gradient error / scale {np.abs(d - want).max() / scale:.2e}")
    assert np.abs(d - want).max() <= TOL[prec] * scale, what
    f_back = check_state(prec, tf, f_in, what + " uncompute")
    b_back = check_state(prec, tb, e * b_in, what + " pull-back")
    # a constant layer, and no cotangent yet: the same states, zeros
    z1 = q.pauli_layer_reverse(t1, tb1, strings, th, want_grad=False)
    assert z1.shape == d.shape and not z1.any()
    assert normrel(t1.get_cpu_state_copy(), f_back) <= TOL[prec], what
    assert normrel(tb1.get_cpu_state_copy(), b_back) <= TOL[prec], what
    z2 = q.pauli_layer_reverse(t2, None, strings, th)
    assert z2.shape == d.shape and not z2.any()
    assert normrel(t2.get_cpu_state_copy(), f_back) <= TOL[prec], what
    return want, scale


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", ["1", "2", "3", "4", "L+1", "17"])
def test_reverse(prec, n):
    """bwd is not normalised (norm^2 about 2) except at n = 17, where the shared states are."""
    lw = span_bits(prec)
    n = size_of(n, lw)
    rng = np.random.default_rng(800 + n)
    zs = layer_masks_for(n, lw)
    th = rng.uniform(-3, 3, len(zs))
    if n == 17:
        tf, _, f, b = states(prec)
    else:
        f = O.random_state(rng, n).astype(DT[prec]).astype(np.complex128)
        b = O.random_state(rng, n, normalise=False).astype(DT[prec]).astype(np.complex128)
        tf = None
    want, scale = check_reverse(prec, n, zs, th, f, b, tf)
    # the C entry point adds into dtheta (fwd as the reverse receives it: after the layer)
    lib = __import__("quantum_differentiable_circuit")._native.load(prec)
    tf2, tb2 = tensor(prec, f), tensor(prec, b)
    tf2.apply_pauli_layer([zstr(z) for z in zs], th)
    start = np.arange(1.0, len(zs) + 1.0)
    d = start.copy()
    za = np.array(zs, dtype=np.uint64)
    ull, dbl = C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
    assert lib.qdc_pauli_layer_reverse(tf2._p, tb2._p, za.ctypes.data_as(ull),
                                       th.ctypes.data_as(dbl), len(zs), n,
                                       d.ctypes.data_as(dbl)) is None
    assert np.abs(d - start - want).max() <= TOL[prec] * scale and np.all(d != start)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("terms", [GCAP + 1, 129])
def test_splitting(prec, terms):
    """More terms than one launch holds, n = 9: the definition's state and gradients, and the
    launch counts of the plan under the profile names, 2 S / 4 S bytes each."""
    import quantum_differentiable_circuit as q
    n = 9
    rng = np.random.default_rng(900 + terms)
    zs = [int(z) for z in rng.integers(0, 1 << n, size=terms)]
    th = rng.uniform(-3, 3, terms)
    f = O.random_state(rng, n).astype(DT[prec]).astype(np.complex128)
    b = O.random_state(rng, n, normalise=False).astype(DT[prec]).astype(np.complex128)
    check_reverse(prec, n, zs, th, f, b)
    strings = [zstr(z) for z in zs]
    plan = q.pauli_layer_plan(n, strings, prec)
    assert plan["forward_launches"] == -(-terms // 128) == plan["reverse_launches"]
    assert plan["reverse_grad_launches"] == -(-terms // GCAP)
    tf, tb = tensor(prec, f), tensor(prec, b)
    q.primitives_profile(True, prec)
    try:
        tf.apply_pauli_layer(strings, th)
        fwd_stats = q.primitives_profile_collect(prec)
        q.primitives_profile(True, prec)
        q.pauli_layer_reverse(tf, tb, strings, th)
        grad_stats = q.primitives_profile_collect(prec)
        q.primitives_profile(True, prec)
        q.pauli_layer_reverse(tf, tb, strings, th, want_grad=False)
        const_stats = q.primitives_profile_collect(prec)
        q.primitives_profile(True, prec)
        q.pauli_layer_reverse(tf, None, strings, th)
        unc_stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    s = float(np.dtype(DT[prec]).itemsize << n)
    assert "pauli_layer_rev" not in fwd_stats and "pauli_layer" not in grad_stats
    for stats, name, launches, per in ((fwd_stats, "pauli_layer", plan["forward_launches"], 2),
                                       (grad_stats, "pauli_layer_rev", plan["reverse_grad_launches"], 4),
                                       (const_stats, "pauli_layer_rev", plan["reverse_launches"], 4),
                                       (unc_stats, "pauli_layer_rev", plan["reverse_launches"], 2)):
        assert stats[name]["launches"] == launches, name
        assert stats[name]["algo_bytes"] == launches * per * s, name


def test_agrees_with_the_rotation_route():
    """f64, n = 10: the layer forward, then its reverse with gradients, against K
    apply_pauli_rotation / pauli_rot_reverse calls: states to 1e-12, gradients to 1e-12 scale."""
    import quantum_differentiable_circuit as q
    n = 10
    tf0, tb0, f, b = states("f64", n=n, seed=79)
    rng = np.random.default_rng(1010)
    zs = [(1 << i) | (1 << j) for i in range(n) for j in range(i)] + [0, 1, (1 << n) - 1, 1]
    strings = [zstr(z) for z in zs]
    th = rng.uniform(-3, 3, len(zs))
    tl, tr = tf0.clone(), tf0.clone()
    tl.apply_pauli_layer(strings, th)
    for ops, t in zip(strings, th):
        tr.apply_pauli_rotation(ops, t)
    assert normrel(tl.get_cpu_state_copy(), tr.get_cpu_state_copy()) <= 1e-12
    bl, br = tb0.clone(), tb0.clone()
    d = q.pauli_layer_reverse(tl, bl, strings, th)
    want = np.zeros(len(zs))
    for k in reversed(range(len(zs))):
        want[k] = q.pauli_rot_reverse(tr, br, strings[k], th[k])
    scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f)
    print(f"max gradient difference / scale {np.abs(d - want).max() / scale:.2e}")
    assert np.abs(d - want).max() <= 1e-12 * scale and np.abs(want).max() > 1e-3 * scale
    assert normrel(tl.get_cpu_state_copy(), tr.get_cpu_state_copy()) <= 1e-12
    assert normrel(bl.get_cpu_state_copy(), br.get_cpu_state_copy()) <= 1e-12
    assert normrel(tl.get_cpu_state_copy(), f) <= 1e-12


def test_panics():
    import quantum_differentiable_circuit as q
    t = q.QuantizedTensor.new_standard(6, precision="f32")
    u = q.QuantizedTensor.new_standard(6, precision="f32")
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        t.apply_pauli_layer(["Z0", "Z6"], [0.1, 0.2])
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        q.pauli_layer_reverse(t, u, [[(7, "Z")]], [0.1])
    for bad in (["X1"], ["Z0", "Z1 Y2"]):
        with pytest.raises(q.PanicException, match="a Pauli layer takes Z strings only."):
            t.apply_pauli_layer(bad, [0.1] * len(bad))
        with pytest.raises(q.PanicException, match="a Pauli layer takes Z strings only."):
            q.pauli_layer_reverse(t, u, bad, [0.1] * len(bad))
    with pytest.raises(q.PanicException, match="The layer has no terms."):
        t.apply_pauli_layer([], [])
    with pytest.raises(q.PanicException, match="The layer has no terms."):
        q.pauli_layer_reverse(t, u, [], [])
    for bad in ([0.1], [0.1, 0.2, 0.3], [[0.1, 0.2]], 0.5):
        with pytest.raises(q.PanicException, match="one angle per string"):
            t.apply_pauli_layer(["Z0", "Z1"], bad)
        with pytest.raises(q.PanicException, match="one angle per string"):
            q.pauli_layer_reverse(t, u, ["Z0", "Z1"], bad)
    with pytest.raises(q.PanicException, match="must be real"):
        t.apply_pauli_layer(["Z0"], [0.1 + 0.2j])
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
            t.apply_pauli_layer(["Z0", "Z1"], [0.1, bad])
        with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
            q.pauli_layer_reverse(t, u, ["Z0", "Z1"], [bad, 0.1])
    with pytest.raises(q.PanicException, match="fwd and bwd must be different states."):
        q.pauli_layer_reverse(t, t, ["Z1"], [0.1])
    with pytest.raises(q.PanicException, match="fwd and bwd have different lengths"):
        q.pauli_layer_reverse(t, q.QuantizedTensor.new_standard(7, precision="f32"), ["Z1"], [0.1])
    # the C ABI validates too
    lib = q._native.load("f32")
    ull, dbl = C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)
    z = np.array([1, 64], dtype=np.uint64)
    th = np.array([0.1, 0.2])
    d = np.zeros(2)
    zp, tp, dp = z.ctypes.data_as(ull), th.ctypes.data_as(dbl), d.ctypes.data_as(dbl)
    assert lib.qdc_pauli_layer(t._p, zp, tp, 2, 6) == b"pos is out of the bound."
    assert lib.qdc_pauli_layer_reverse(t._p, u._p, zp, tp, 2, 6, dp) == b"pos is out of the bound."
    assert lib.qdc_pauli_layer(t._p, zp, tp, 0, 6) == b"The layer has no terms."
    assert lib.qdc_pauli_layer_reverse(t._p, u._p, zp, tp, 0, 6, dp) == b"The layer has no terms."
    z[1] = 2
    th[1] = float("nan")
    assert lib.qdc_pauli_layer(t._p, zp, tp, 2, 6) == b"Pauli coefficients must be finite."
    assert lib.qdc_pauli_layer_reverse(t._p, u._p, zp, tp, 2, 6, dp) == \
        b"Pauli coefficients must be finite."
    th[1] = 0.2
    assert lib.qdc_pauli_layer_reverse(t._p, t._p, zp, tp, 2, 6, dp) == \
        b"fwd and bwd must be different states."
    assert lib.qdc_pauli_layer_reverse(t._p, None, zp, tp, 2, 6, dp) is not None
    assert b"supported range" in lib.qdc_pauli_layer(t._p, zp, tp, 2, 41)
    assert not d.any()
    # nothing above touched the state
    psi = np.zeros(64, np.complex64)
    psi[0] = 1
    assert np.array_equal(t.get_cpu_state_copy(), psi)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_full_size(prec):
    """n = 28 (f32) / 27 (f64), the chain of n - 1 ZZ bonds on the uniform superposition.  Bond k
    has the sign (-1)^(bit k of g), g = i ^ (i >> 1), so phi(i) = 1/2 sum theta - sum_k theta_k g_k
    and the factor of amplitude i = (h, l) (l the low 14 bits) is E_hi[h] E_lo[l] C[bit 14, bit 13],
    C the factor of the bond across the cut: every amplitude is checked, in blocks.  Then the
    reverse without a cotangent returns the initial state."""
    import quantum_differentiable_circuit as q
    n = 28 if prec == "f32" else 27
    cut = 14
    rng = np.random.default_rng(2800 + n)
    th = rng.uniform(-np.pi, np.pi, n - 1)
    strings = [f"Z{k} Z{k + 1}" for k in range(n - 1)]
    amp = 1.0 / np.sqrt(float(1 << n))
    t = q.QuantizedTensor.new_from_host(np.full(1 << n, amp, DT[prec]), precision=prec)
    t.apply_pauli_layer(strings, th)
    got = t.get_cpu_state_copy().reshape(1 << (n - cut), 1 << cut)
    lo_z = [(1 << k) | (1 << (k + 1)) for k in range(cut - 1)]
    hi_z = [(1 << k) | (1 << (k + 1)) for k in range(n - cut - 1)]
    e_lo = np.exp(-1j * phase(cut, lo_z, th[:cut - 1]))
    e_hi = np.exp(-1j * phase(n - cut, hi_z, th[cut:])) * amp
    tc = th[cut - 1]
    worst = 0.0
    rows = 1 << 9
    for r0 in range(0, 1 << (n - cut), rows):
        want = e_hi[r0:r0 + rows, None] * e_lo[None, :]
        hbit = (np.arange(r0, r0 + rows) & 1)[:, None]
        lbit = (np.arange(1 << cut) >> (cut - 1) & 1)[None, :]
        want = want * np.exp(-0.5j * tc * (1.0 - 2.0 * (hbit ^ lbit)))
        worst = max(worst, float(np.abs(got[r0:r0 + rows] - want).max()))
    print(f"full size {prec}: worst amplitude error / amplitude {worst / amp:.2e}")
    assert worst <= TOL[prec] * amp
    del got
    assert not q.pauli_layer_reverse(t, None, strings, th).any()
    back = t.get_cpu_state_copy()
    back -= DT[prec](amp)
    print(f"full size {prec}: worst round-trip error / amplitude {np.abs(back).max() / amp:.2e}")
    assert np.abs(back).max() <= TOL[prec] * amp

"""Pauli rotations exp(-i theta/2 P) on the GPU (include/qdc/pauli.h: qdc_pauli_rot,
qdc_pauli_rot_reverse; csrc/qdc_paulirot.hpp).

Expected values come from the host definition in complex128 on the build-precision inputs:
R psi = cos(theta/2) psi - i sin(theta/2) PauliSum(n, [(1, ops)]).apply(psi) (pinned to the matrix
by tests/test_pauli_rot_cpu.py).  Tolerances are those of tests/test_gpu_pauli.py: normrel <=
1e-5 (f32) / 1e-12 (f64) for a state, and |dtheta - ref| <= TOL 1/2 ||bwd|| ||fwd|| for the angle's
gradient, the Cauchy-Schwarz scale of its sum."""
import ctypes as C

import numpy as np
import pytest

from floors import normrel
from oracle import oracle as O
from test_gpu_dense_grad import DT, TOL, states, tensor
from test_gpu_pauli import tile_width

pytestmark = pytest.mark.gpu


def pauli(n, ops):
    from quantum_differentiable_circuit import PauliSum
    return PauliSum(n, [(1.0, ops)])


def n_y(n, ops):
    (_, x, z), = pauli(n, ops).terms()
    return bin(x & z).count("1")


def rot_ref(n, ops, theta, psi, transpose=False):
    """R(theta) psi, or R(theta)^T psi = cos psi - i sin (-1)^nY P psi."""
    psi = np.asarray(psi, np.complex128)
    sign = (-1) ** n_y(n, ops) if transpose else 1
    return np.cos(theta / 2) * psi - 1j * np.sin(theta / 2) * sign * pauli(n, ops).apply(psi)


def dtheta_ref(n, ops, theta, fwd_in, bwd):
    """Re sum_i bwd[i] (dR/dtheta fwd_in)[i], dR/dtheta = -(i/2) P R."""
    return float(np.sum(bwd * (-0.5j * pauli(n, ops).apply(rot_ref(n, ops, theta, fwd_in)))).real)


def strings(n, w):
    """The list shape of test_gpu_pauli.single_terms for an n-qubit state, strings that name a
    qubit >= n or one twice left out: x = 0 (identity, Z strings), x = 1, x = 2^(n-1), lowest x
    bit 0 with highest n - 1, one to four Y's inside and past a tile, a weight-n string."""
    terms = ["", "Z0", f"Z0 Z{n - 1}", "X0", "Y0", f"X{n - 1}", f"Y{n - 1}", f"X0 X{n - 1}",
             f"X0 Z1 Y{n - 1}", f"X1 X{n - 1}"]
    for p in (w - 1, w):
        terms += [f"Z{p}", f"X{p}", f"Y{p}"]
    terms += ["Y2", "Y1 Y5", "Y0 Y3 Y9", f"Y1 Y4 Y8 Y{w - 1}"]
    terms += [f"Y3 Y{n - 1}", f"Y0 Y{w} Y{n - 1}", f"Y1 Y{w - 1} Y{w} Y{n - 1}"]
    terms += [f"Y2 Z6 X{w - 2}", f"Z0 Y{w + 1} Z{n - 1}", f"Z1 X{w} Y{n - 1}"]
    terms.append(" ".join("XYZ"[q % 3] + str(q) for q in range(n)))  # weight n
    terms.append(" ".join("YXZ"[q % 3] + str(q) for q in range(n)))  # weight n, Y on qubit 0
    out = []
    for ops in terms:
        qs = [int(tok[1:]) for tok in ops.split()]
        if all(p < n for p in qs) and len(set(qs)) == len(qs) and ops not in out:
            out.append(ops)
    return out


def check_state(prec, t, want, what):
    got = t.get_cpu_state_copy()
    err = normrel(got, want)
    print(f"{prec} {what}: normrel {err:.2e}")
    assert err <= TOL[prec], what
    return got


def check_reverse(prec, n, ops, theta, f_in, b_in, tf_in=None):
    """apply, then the three forms of the reverse step, against the host definition."""
    import quantum_differentiable_circuit as q
    what = f"n={n} {ops!r}"
    f_out = rot_ref(n, ops, theta, f_in)
    tf = (tf_in.clone() if tf_in is not None else tensor(prec, f_in))
    tf.apply_pauli_rotation(ops, theta)
    check_state(prec, tf, f_out, what + " apply")
    t1, t2 = tf.clone(), tf.clone()
    tb, tb1 = tensor(prec, b_in), tensor(prec, b_in)
    d = q.pauli_rot_reverse(tf, tb, ops, theta)
    want = dtheta_ref(n, ops, theta, f_in, b_in)
    scale = 0.5 * np.linalg.norm(b_in) * np.linalg.norm(f_in)
    print(f"{prec} {what}: dtheta {d:.15e} want {want:.15e} err/scale {abs(d - want) / scale:.2e}")
    assert isinstance(d, float) and abs(d - want) <= TOL[prec] * scale, what
    f_back = check_state(prec, tf, f_in, what + " uncompute")
    b_back = check_state(prec, tb, rot_ref(n, ops, theta, b_in, transpose=True), what + " pull-back")
    # a constant gate, and no cotangent yet: the same states, 0.0
    assert q.pauli_rot_reverse(t1, tb1, ops, theta, want_grad=False) == 0.0
    assert normrel(t1.get_cpu_state_copy(), f_back) <= TOL[prec], what
    assert normrel(tb1.get_cpu_state_copy(), b_back) <= TOL[prec], what
    assert q.pauli_rot_reverse(t2, None, ops, theta) == 0.0
    assert normrel(t2.get_cpu_state_copy(), f_back) <= TOL[prec], what


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", ["1", "2", "3", "W-1", "W", "W+1"])
def test_apply_every_path_at_small_sizes(prec, n):
    """States of one chunk and less, below one span, around the tile width of the observables'
    kernels; random complex states that are not normalised."""
    w = tile_width(prec)
    n = {"W-1": w - 1, "W": w, "W+1": w + 1}.get(n) or int(n)
    rng = np.random.default_rng(300 + n)
    psi = O.random_state(rng, n, normalise=False).astype(DT[prec])
    t0, psi = tensor(prec, psi), psi.astype(np.complex128)
    assert abs(np.vdot(psi, psi).real - 1) > 0.25
    for ops in strings(n, w):
        theta = float(rng.uniform(-3, 3))
        t = t0.clone()
        t.apply_pauli_rotation(ops, theta)
        check_state(prec, t, rot_ref(n, ops, theta, psi), f"n={n} {ops!r} theta={theta:.3f}")
    # the identity string is the global phase, theta = 0 the identity, 2 pi the sign
    t = t0.clone()
    t.apply_pauli_rotation("", 1.1)
    check_state(prec, t, np.exp(-0.55j) * psi, "global phase")
    t.apply_pauli_rotation(f"Y{n - 1}", 0.0)
    t.apply_pauli_rotation("X0", 2 * np.pi)
    check_state(prec, t, -np.exp(-0.55j) * psi, "theta = 0, 2 pi")


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 17])
def test_reverse(prec, n):
    w = tile_width(prec)
    rng = np.random.default_rng(400 + n)
    if n == 17:
        tf, _, f, b = states(prec)
        todo = ["", "Z0", f"Z0 Z{n - 1}", "X0", "Y0", f"X{n - 1}", f"X1 X{n - 1}", "Y1 Y5",
                f"Y0 Y{w} Y{n - 1}", f"Y1 Y{w - 1} Y{w} Y{n - 1}", strings(n, w)[-2], strings(n, w)[-1]]
    else:
        f, b = (O.random_state(rng, n, normalise=False).astype(DT[prec]).astype(np.complex128)
                for _ in range(2))
        tf, todo = None, strings(n, w)
    for ops in todo:
        check_reverse(prec, n, ops, float(rng.uniform(-3, 3)), f, b, tf)


def test_agrees_with_the_dense_route():
    """f64, n = 9, strings on 1..5 qubits (positions from most to least significant; the matrix
    is PauliSum(k, ...).to_matrix() on relabelled qubits): the state after apply_qk_gate, dtheta
    as Re sum(get_qk_grad . dU/dtheta), the pulled-back bwd after apply_qk_gate_tr."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    n, theta = 9, 0.91
    tf0, tb0, f, b = states("f64", n=9, seed=78)
    cases = [[(4, "Y")], [(8, "X"), (0, "Z")], [(7, "Y"), (3, "Y"), (1, "X")],
             [(8, "Z"), (6, "Y"), (5, "X"), (0, "Y")], [(8, "Y"), (5, "Z"), (3, "Y"), (2, "Y"), (1, "X")],
             [(6, "Z"), (2, "Z")], [(0, "X")]]
    for ops in cases:
        pos = [p for p, _ in ops]
        k = len(pos)
        assert pos == sorted(pos, reverse=True)
        # local index bit k-1-b is qubit pos[b]
        pk = PauliSum(k, [(1.0, [(k - 1 - i, l) for i, (_, l) in enumerate(ops)])]).to_matrix()
        u = np.cos(theta / 2) * np.eye(1 << k) - 1j * np.sin(theta / 2) * pk
        du = -0.5j * pk @ u
        tf, td, tb, te = tf0.clone(), tf0.clone(), tb0.clone(), tb0.clone()
        tf.apply_pauli_rotation(ops, theta)
        td.apply_qk_gate(u.reshape(-1), pos)
        f_out = td.get_cpu_state_copy()
        assert normrel(tf.get_cpu_state_copy(), f_out) <= 1e-12, ops
        d = q.pauli_rot_reverse(tf, tb, ops, theta)
        want = float(np.sum(q.get_qk_grad(tf0, tb0, pos) * du.reshape(-1)).real)
        scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f)
        print(f"{ops}: dtheta {d:.15e} dense route {want:.15e}")
        assert abs(d - want) <= 1e-12 * scale, ops
        te.apply_qk_gate_tr(u.reshape(-1), pos)
        assert normrel(tb.get_cpu_state_copy(), te.get_cpu_state_copy()) <= 1e-12, ops
        assert normrel(tf.get_cpu_state_copy(), f) <= 1e-12, ops


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_grid_stride_loops_tails_and_determinism(monkeypatch, prec):
    """Three blocks and one at n = 13 (several spans per block, a block without a span) and at
    n = 10 (fewer pairs than one span: the bounded tail) against the uncapped launches; two
    identical reverse calls return identical bits."""
    import quantum_differentiable_circuit as q
    for n in (13, 10):
        rng = np.random.default_rng(500 + n)
        f, b = (O.random_state(rng, n, normalise=False).astype(DT[prec]) for _ in range(2))
        for ops in ("Z0 Z5", "X0", f"Y0 X{n - 1}", f"X3 Z4 Y{n - 2}", strings(n, 10)[-1]):
            theta = float(rng.uniform(-3, 3))
            runs = []
            for grid in (None, "3", "1", "3"):
                if grid is None:
                    monkeypatch.delenv("QDC_PAULI_GRID", raising=False)
                else:
                    monkeypatch.setenv("QDC_PAULI_GRID", grid)
                tf, tb = tensor(prec, f), tensor(prec, b)
                tf.apply_pauli_rotation(ops, theta)
                applied = tf.get_cpu_state_copy()
                d = q.pauli_rot_reverse(tf, tb, ops, theta)
                runs.append((applied, d, tf.get_cpu_state_copy(), tb.get_cpu_state_copy()))
            scale = 0.5 * np.linalg.norm(b) * np.linalg.norm(f)
            for r in runs[1:]:
                assert normrel(r[0], runs[0][0]) <= TOL[prec], (n, ops)
                assert abs(r[1] - runs[0][1]) <= TOL[prec] * scale, (n, ops)
                assert normrel(r[2], runs[0][2]) <= TOL[prec] and normrel(r[3], runs[0][3]) <= TOL[prec]
            # the same call, the same bits (grid 3 twice)
            assert runs[1][1] == runs[3][1]
            assert all(np.array_equal(x, y) for x, y in zip(runs[1], runs[3])), (n, ops)
            assert normrel(runs[0][0], rot_ref(n, ops, theta, f)) <= TOL[prec]
    monkeypatch.delenv("QDC_PAULI_GRID", raising=False)
    tf0, tb0, _, _ = states(prec)
    outs = []
    for _ in range(2):
        tf, tb = tf0.clone(), tb0.clone()
        d = q.pauli_rot_reverse(tf, tb, "Y0 Z3 X11 Y16", 0.37)
        outs.append((d, tf.get_cpu_state_copy(), tb.get_cpu_state_copy()))
    assert outs[0][0] == outs[1][0] and outs[0][0] != 0.0
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def test_profile_names_and_bytes():
    """Both calls run on the primitives' stream under names of their own: 2 S for the gate and
    the uncompute alone, 4 S for the reverse over both states."""
    import quantum_differentiable_circuit as q
    tf0, tb0, _, _ = states("f32")
    tf, tb = tf0.clone(), tb0.clone()
    q.primitives_profile(True, "f32")
    try:
        tf.apply_pauli_rotation("X0 Z9", 0.3)
        tf.apply_pauli_rotation("Z1", 0.3)
        q.pauli_rot_reverse(tf, tb, "Z1", 0.3)
        q.pauli_rot_reverse(tf, None, "X0 Z9", 0.3)
        stats = q.primitives_profile_collect("f32")
    finally:
        q.primitives_profile(False, "f32")
    s = float(8 << 17)
    assert stats["pauli_rot"]["launches"] == 2 and stats["pauli_rot"]["algo_bytes"] == 4 * s
    assert stats["pauli_rot_rev"]["launches"] == 2 and stats["pauli_rot_rev"]["algo_bytes"] == 6 * s


def test_panics():
    import quantum_differentiable_circuit as q
    t = q.QuantizedTensor.new_standard(6, precision="f32")
    u = q.QuantizedTensor.new_standard(6, precision="f32")
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        t.apply_pauli_rotation("X6", 0.1)
    with pytest.raises(q.PanicException, match="pos is out of the bound."):
        q.pauli_rot_reverse(t, u, [(7, "Z")], 0.1)
    with pytest.raises(q.PanicException, match="a qubit appears twice in a Pauli term."):
        t.apply_pauli_rotation("X1 Y1", 0.1)
    with pytest.raises(q.PanicException, match="a qubit appears twice in a Pauli term."):
        q.pauli_rot_reverse(t, u, "Z2 Z2", 0.1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
            t.apply_pauli_rotation("X1", bad)
        with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
            q.pauli_rot_reverse(t, u, "X1", bad)
    with pytest.raises(q.PanicException, match="fwd and bwd must be different states."):
        q.pauli_rot_reverse(t, t, "X1", 0.1)
    with pytest.raises(q.PanicException, match="fwd and bwd have different lengths"):
        q.pauli_rot_reverse(t, q.QuantizedTensor.new_standard(7, precision="f32"), "X1", 0.1)
    with pytest.raises(q.PanicException, match="must be real"):
        t.apply_pauli_rotation("X1", 0.1 + 0.2j)
    # the C ABI validates too
    lib = q._native.load("f32")
    d = C.c_double(0.0)
    assert lib.qdc_pauli_rot(t._p, 64, 0, 0.1, 6) == b"pos is out of the bound."
    assert lib.qdc_pauli_rot(t._p, 0, 64, 0.1, 6) == b"pos is out of the bound."
    assert lib.qdc_pauli_rot_reverse(t._p, u._p, 1, 64, 0.1, 6, C.byref(d)) == b"pos is out of the bound."
    assert lib.qdc_pauli_rot(t._p, 1, 0, float("nan"), 6) == b"Pauli coefficients must be finite."
    msg = lib.qdc_pauli_rot_reverse(t._p, u._p, 1, 0, float("inf"), 6, C.byref(d))
    assert msg == b"Pauli coefficients must be finite."
    msg = lib.qdc_pauli_rot_reverse(t._p, t._p, 1, 0, 0.1, 6, C.byref(d))
    assert msg == b"fwd and bwd must be different states."
    assert lib.qdc_pauli_rot_reverse(t._p, None, 1, 0, 0.1, 6, C.byref(d)) is not None
    assert b"supported range" in lib.qdc_pauli_rot(t._p, 1, 0, 0.1, 41)
    assert d.value == 0.0
    # nothing above touched the state; a valid raw call adds into *dtheta
    psi = np.zeros(64, np.complex64)
    psi[0] = 1
    assert np.array_equal(t.get_cpu_state_copy(), psi)
    d = C.c_double(5.0)
    assert lib.qdc_pauli_rot_reverse(t._p, u._p, 0, 1, 0.0, 6, C.byref(d)) is None
    assert d.value == 5.0  # 1/2 Im(<0|Z0|0>) = 0


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_full_size(prec):
    """n = 28 (f32) / 27 (f64) from |0..0>, P = Y0 Z3 X20 X(n-1), theta = 0.7.  P anticommutes
    with Z0 and Z20, commutes with Z3, and <0|Z P|0> = 0: <Z0> = <Z20> = cos 0.7, <Z3> = 1.  The
    cotangent of <Z0> pulled through the gate gives d<Z0>/dtheta = -sin 0.7, and the reverse
    leaves fwd at |0..0>."""
    import quantum_differentiable_circuit as q
    n = 28 if prec == "f32" else 27
    ops, theta = f"Y0 Z3 X20 X{n - 1}", 0.7
    t = q.QuantizedTensor.new_standard(n, precision=prec)
    t.apply_pauli_rotation(ops, theta)
    for z, want in (("Z0", np.cos(theta)), ("Z20", np.cos(theta)), ("Z3", 1.0)):
        e = t.pauli_energy(pauli(n, z))
        print(f"full size {prec}: <{z}> = {e:.9f}")
        assert abs(e - want) < 1e-5, z
    bwd = q.QuantizedTensor(n, prec)
    q.pauli_inject(t, bwd, pauli(n, "Z0"), 1.0, accumulate=False)
    d = q.pauli_rot_reverse(t, bwd, ops, theta)
    print(f"full size {prec}: dtheta = {d:.9f}")
    assert abs(d + np.sin(theta)) < 1e-5
    del bwd
    back = t.get_cpu_state_copy()
    back[0] -= 1
    assert np.abs(back).max() <= (1e-5 if prec == "f32" else 1e-12)

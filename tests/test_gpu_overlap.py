"""Overlaps and transition elements on the GPU (include/qdc/overlap.h: qdc_overlap,
qdc_pauli_overlap, qdc_overlap_inject, qdc_pauli_overlap_inject; csrc/qdc_overlap.hpp).

The reference is numpy in complex128 on the build-precision inputs (tests/test_overlap_cpu.py:
overlap_ref, inject_ref, over apply_ref of tests/test_gpu_pauli.py).  The states are those of
tests/test_gpu_dense_grad.py (two different states at n = 17, seed 77), the tolerances the
primitives' own: 1e-5 (f32), 1e-12 (f64), on |o - o_ref| / (sum |c_t| ||a|| ||b||) and on the
norm-relative error of an injected state."""
import ctypes as C

import numpy as np
import pytest

from floors import normrel
from oracle import oracle as O
from test_gpu_dense_grad import DT, TOL, states, tensor
from test_gpu_pauli import N, random_sum, single_terms, sums, tile_width
from test_overlap_cpu import inject_ref, overlap_ref, scale_of

pytestmark = pytest.mark.gpu
G = 0.6 - 1.1j  # a properly complex upstream weight


def check_o(prec, got, want, scale, what):
    assert isinstance(got, complex), what
    print(f"overlap {prec} {what}: got {got:.12e} want {want:.12e} err/scale "
          f"{abs(got - want) / scale:.2e}")
    assert abs(got - want) <= TOL[prec] * scale, what
    return got


def check_pair(prec, ta, tb, a, b, obs, what):
    """<a|H|b> (obs None: <a|b>) against the reference."""
    got = ta.overlap(tb) if obs is None else ta.pauli_overlap(tb, obs)
    return check_o(prec, got, overlap_ref(a, b, obs), scale_of(a, b, obs), what)


def check_inject(prec, ts, src, obs, what, g=G, onto=None):
    """accumulate=False into a bwd full of NaN (a kernel that read it, or skipped an amplitude,
    would leave one), or accumulate=True onto the known state `onto`."""
    import quantum_differentiable_circuit as q
    want = inject_ref(src, g, obs)
    if onto is None:
        tb = tensor(prec, np.full(src.size, np.nan + 1j * np.nan))
        q.overlap_inject(ts, tb, g, obs, accumulate=False)
    else:
        tb = tensor(prec, onto)
        want = want + onto.astype(DT[prec]).astype(np.complex128)
        q.overlap_inject(ts, tb, g, obs)
    got = tb.get_cpu_state_copy()
    assert np.isfinite(got.view(got.real.dtype)).all(), what
    err = normrel(got, want)
    print(f"overlap inject {prec} {what}: normrel {err:.2e}")
    assert err <= TOL[prec], what
    return got


def window_only(w):
    from quantum_differentiable_circuit import PauliSum
    return PauliSum(N, [(0.7, "Z0 Z1"), (-0.4, "X3 Y5"), (1.2, f"Y{w - 1} Z{N - 1}"),
                        (0.3, ""), (-0.9, f"Y0 Y2 X{w - 2}")])


def far_only(w):
    from quantum_differentiable_circuit import PauliSum
    return PauliSum(N, [(0.9, f"X{N - 1}"), (-0.4, f"Y{w} Z3"), (0.6, f"X{w + 1} X0"),
                        (1.1, f"X{N - 1} Z{w}")])


def small_pair(prec, n, seed):
    rng = np.random.default_rng(seed)
    a, b = (O.random_state(rng, n, normalise=False).astype(DT[prec]) for _ in range(2))
    return tensor(prec, a), tensor(prec, b), a.astype(np.complex128), b.astype(np.complex128), rng


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_plain_overlap(prec):
    ta, tb, a, b = states(prec)
    o = check_pair(prec, ta, tb, a, b, None, "<a|b>")
    assert abs(o) > 10 * TOL[prec]  # (two random states: |o| ~ 2^-8.5, well above the bound)
    check_pair(prec, tb, ta, b, a, None, "<b|a>")
    # an unnormalised pair
    tu, tv, u, v, _ = small_pair(prec, N, 9)
    assert abs(np.vdot(u, u).real - 1) > 0.5 and abs(np.vdot(v, v).real - 1) > 0.5
    check_pair(prec, tu, tv, u, v, None, "unnormalised")
    # <u|u> is the squared norm
    n2 = np.vdot(u, u).real
    o = check_pair(prec, tu, tu, u, u, None, "<u|u>")
    assert abs(o.real - tu.norm_sq()) <= TOL[prec] * n2 and abs(o.imag) <= TOL[prec] * n2


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [1, 3, 9])
def test_small_states(prec, n):
    """Below one chunk (n = 1 in f32 is exactly one, 0 is below) and below a tile: the plain
    overlap, a random sum on the top qubit, and the two injections."""
    ta, tb, a, b, rng = small_pair(prec, n, 200 + n)
    check_pair(prec, ta, tb, a, b, None, f"n={n}")
    obs = random_sum(rng, n, 12, top=True)
    check_pair(prec, ta, tb, a, b, obs, f"n={n} sum")
    onto = O.random_state(rng, n)
    for o in (None, obs):
        check_inject(prec, ta, a, o, f"n={n} {'I' if o is None else 'sum'}")
        check_inject(prec, ta, a, o, f"n={n} {'I' if o is None else 'sum'} accumulate", onto=onto)
    if n == 1:
        t0, t1, s0, s1, _ = small_pair(prec, 0, 7)
        check_pair(prec, t0, t1, s0, s1, None, "n=0")
        check_inject(prec, t0, s0, None, "n=0")
        check_inject(prec, t0, s0, None, "n=0 accumulate", onto=s1)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_single_terms(prec):
    """Every string of the energy test between two DIFFERENT states: the four i^nY phases inside
    and past a tile, far groups with lowest x bit 0 and W, weight 17, the identity — where the two
    ends of a far pair, or the conj side, can be swapped without an a = b test noticing."""
    from quantum_differentiable_circuit import PauliSum
    ta, tb, a, b = states(prec)
    for ops in single_terms(tile_width(prec)):
        check_pair(prec, ta, tb, a, b, PauliSum(N, [(1.0, ops)]), repr(ops))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sums(prec):
    from quantum_differentiable_circuit import observable
    ta, tb, a, b = states(prec)
    for name, obs in sums(prec).items():
        check_pair(prec, ta, tb, a, b, obs, name)
    w = tile_width(prec)
    p = observable.plan(window_only(w), prec)
    assert p["window_groups"] > 0 and p["far_groups"] == 0
    check_pair(prec, ta, tb, a, b, window_only(w), "window only")
    p = observable.plan(far_only(w), prec)
    assert p["window_groups"] == 0 and p["far_groups"] == 3
    check_pair(prec, ta, tb, a, b, far_only(w), "far only")
    # more launches than one batch of reduction slots
    many = random_sum(np.random.default_rng(6), N, 64, top=True)
    assert observable.plan(many, prec)["energy_launches"] > 32
    check_pair(prec, ta, tb, a, b, many, "random64")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_symmetries(prec):
    ta, tb, a, b = states(prec)
    obs = sums(prec)["random40"]
    scale = scale_of(a, b, obs)
    ab = check_pair(prec, ta, tb, a, b, obs, "<a|H|b>")
    ba = check_pair(prec, tb, ta, b, a, obs, "<b|H|a>")
    # H is Hermitian; each side carries its own error
    assert abs(ab - np.conj(ba)) <= 2 * TOL[prec] * scale
    # a = b: the energy, real
    aa = check_pair(prec, ta, ta, a, a, obs, "<a|H|a>")
    saa = scale_of(a, a, obs)
    assert abs(aa.real - ta.pauli_energy(obs)) <= TOL[prec] * saa and abs(aa.imag) <= TOL[prec] * saa
    # linear in the ket: b2 = b + lam c, rounded to the build precision (an error eps ||b2||, far
    # below the bound); the three values carry one error each
    lam = 0.3 - 0.8j
    c = O.random_state(np.random.default_rng(78), N).astype(DT[prec]).astype(np.complex128)
    b2 = (b + lam * c).astype(DT[prec])
    tc, tb2 = tensor(prec, c), tensor(prec, b2)
    ac, ab2 = ta.pauli_overlap(tc, obs), ta.pauli_overlap(tb2, obs)
    bound = TOL[prec] * (scale + abs(lam) * scale_of(a, c, obs) + scale_of(a, b2, obs))
    print(f"linearity {prec}: {abs(ab2 - (ab + lam * ac)):.2e} bound {bound:.2e}")
    assert abs(ab2 - (ab + lam * ac)) <= bound


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("grid", ["1", "3"])
def test_grid_stride_loops_and_tails(monkeypatch, prec, grid):
    """n = 13: 2^(13-W) tiles, 4 spans of pairs and 4 (f32) or 8 (f64) spans of chunks over one
    and three blocks; every kernel agrees with its default grid."""
    import quantum_differentiable_circuit as q
    n = 13
    ta, tb, a, b, rng = small_pair(prec, n, 300)
    obs = random_sum(rng, n, 20, top=True)
    onto = O.random_state(rng, n).astype(DT[prec])

    def run():
        out = [ta.overlap(tb), ta.pauli_overlap(tb, obs)]
        for o in (None, obs):
            t1, t2 = q.QuantizedTensor(n, prec), tensor(prec, onto)
            q.overlap_inject(ta, t1, G, o, accumulate=False)
            q.overlap_inject(ta, t2, G, o, accumulate=True)
            out += [t1.get_cpu_state_copy(), t2.get_cpu_state_copy()]
        return out

    want = run()
    monkeypatch.setenv("QDC_PAULI_GRID", grid)
    got = run()
    check_o(prec, got[0], overlap_ref(a, b), scale_of(a, b), f"grid {grid}")
    check_o(prec, got[1], overlap_ref(a, b, obs), scale_of(a, b, obs), f"grid {grid} sum")
    assert abs(got[0] - want[0]) <= TOL[prec] * scale_of(a, b)
    assert abs(got[1] - want[1]) <= TOL[prec] * scale_of(a, b, obs)
    for x, y in zip(got[2:], want[2:]):
        # (the injections do not reduce: a thread computes the same amplitude on any grid)
        assert np.array_equal(x, y)
    assert normrel(got[4], inject_ref(a, G, obs)) <= TOL[prec]
    assert normrel(got[5], inject_ref(a, G, obs) + onto.astype(np.complex128)) <= TOL[prec]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_deterministic_and_accumulating(prec):
    import quantum_differentiable_circuit as q
    ta, tb, _, _ = states(prec)
    obs = sums(prec)["random40"]
    once, once_h = ta.overlap(tb), ta.pauli_overlap(tb, obs)
    assert ta.overlap(tb) == once and ta.pauli_overlap(tb, obs) == once_h
    for o in (None, obs):
        x, y = (q.QuantizedTensor(N, prec) for _ in range(2))
        q.overlap_inject(ta, x, G, o, accumulate=False)
        q.overlap_inject(ta, y, G, o, accumulate=False)
        assert np.array_equal(x.get_cpu_state_copy(), y.get_cpu_state_copy())
    # the C calls add to out[]
    out = (C.c_double * 2)(5.0, -3.0)
    assert ta._lib.qdc_overlap(ta._p, tb._p, N, out) is None
    assert (out[0], out[1]) == (5.0 + once.real, -3.0 + once.imag)
    out = (C.c_double * 2)(5.0, -3.0)
    assert ta._lib.qdc_pauli_overlap(ta._p, tb._p, *obs._args(), N, out) is None
    assert (out[0], out[1]) == (5.0 + once_h.real, -3.0 + once_h.imag)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_injection(prec):
    import quantum_differentiable_circuit as q
    ta, _, a, b = states(prec)
    w = tile_width(prec)
    cases = {"I": None, "window only": window_only(w), "far only": far_only(w), **sums(prec)}
    for name, obs in cases.items():
        check_inject(prec, ta, a, obs, name)
        check_inject(prec, ta, a, obs, name + " accumulate", onto=b)
    check_inject(prec, ta, a, cases["random40"], "imaginary g", g=-0.8j)
    # src = fwd and a real g = 2 w: the one-state injection
    for name in ("window only", "far only", "random40"):
        wgt = -0.65
        x, y = (q.QuantizedTensor(N, prec) for _ in range(2))
        q.overlap_inject(ta, x, 2 * wgt, cases[name], accumulate=False)
        q.pauli_inject(ta, y, cases[name], wgt, accumulate=False)
        err = normrel(x.get_cpu_state_copy(), y.get_cpu_state_copy())
        print(f"inject {prec} {name} against pauli_inject: normrel {err:.2e}")
        assert err <= TOL[prec]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_launch_counts(prec):
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import observable
    ta, tb, _, _ = states(prec)
    obs = sums(prec)["ising"]
    p = observable.plan(obs, prec)
    out = q.QuantizedTensor(N, prec)
    q.primitives_profile(True, prec)
    try:
        ta.overlap(tb)
        ta.pauli_overlap(tb, obs)
        for o in (None, obs):
            q.overlap_inject(ta, out, G, o, accumulate=False)
            q.overlap_inject(ta, out, G, o)
        stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    count = lambda name: stats.get(name, {"launches": 0})["launches"]
    s = float(16 << N if prec == "f64" else 8 << N)
    assert count("overlap") == 1 and stats["overlap"]["algo_bytes"] == 2 * s
    assert count("pauli_overlap_window") == 1 and count("pauli_overlap_far") == p["far_groups"]
    assert stats["pauli_overlap_window"]["algo_bytes"] == 2 * s
    assert stats["pauli_overlap_far"]["algo_bytes"] == 2 * s * p["far_groups"]
    # 2 S storing, 3 S accumulating; the one-state kernels are not used
    assert count("overlap_inj") == 2 and stats["overlap_inj"]["algo_bytes"] == 5 * s
    assert count("pauli_overlap_window_inj") == 2
    assert stats["pauli_overlap_window_inj"]["algo_bytes"] == 5 * s
    assert count("pauli_overlap_far_inj") == 2 * p["far_groups"]
    assert stats["pauli_overlap_far_inj"]["algo_bytes"] == 6 * s * p["far_groups"]
    for name in ("pauli_window", "pauli_far", "pauli_window_inj", "pauli_far_inj"):
        assert count(name) == 0


def test_panics():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum
    t = q.QuantizedTensor.new_standard(6, precision="f32")
    u = q.QuantizedTensor.new_standard(6, precision="f32")
    t7 = q.QuantizedTensor.new_standard(7, precision="f32")
    d = q.QuantizedTensor.new_standard(6, precision="f64")
    obs = PauliSum(6, [(1.0, "X0 Z5")])
    for other in (t7, d):
        match = "different sizes" if other is t7 else "different precisions"
        with pytest.raises(q.PanicException, match=match):
            t.overlap(other)
        with pytest.raises(q.PanicException, match=match):
            t.pauli_overlap(other, obs)
        with pytest.raises(q.PanicException, match=match):
            q.overlap_inject(t, other, 1.0)
        with pytest.raises(q.PanicException, match=match):
            q.overlap_inject(t, other, 1.0, obs)
    with pytest.raises(q.PanicException, match="The observable and the tensor have different sizes."):
        t.pauli_overlap(u, PauliSum(7, [(1.0, "X0")]))
    with pytest.raises(q.PanicException, match="The observable and the tensor have different sizes."):
        q.overlap_inject(t, u, 1.0, PauliSum(5, [(1.0, "X0")]))
    with pytest.raises(q.PanicException, match="The observable has no terms."):
        t.pauli_overlap(u, PauliSum(6, []))
    with pytest.raises(q.PanicException, match="The observable has no terms."):
        q.overlap_inject(t, u, 1.0, PauliSum(6, []))
    for o in (None, obs):
        with pytest.raises(q.PanicException, match="fwd and bwd must be different states."):
            q.overlap_inject(t, t, 1.0, o)
        for bad in (float("inf"), complex(0.0, float("nan"))):
            with pytest.raises(q.PanicException, match="Pauli coefficients must be finite."):
                q.overlap_inject(t, u, bad, o)
    assert t.overlap(t) == 1.0 and t.overlap(u) == 1.0  # a == b is allowed
    # the C ABI validates too
    lib = q._native.load("f32")
    ull, dbl = C.c_ulonglong * 2, C.c_double * 2
    out = dbl(0.0, 0.0)
    x, z, c = ull(1, 64), ull(0, 0), dbl(1.0, 1.0)
    assert lib.qdc_pauli_overlap(t._p, u._p, x, z, c, 2, 6, out) == b"pos is out of the bound."
    assert lib.qdc_pauli_overlap_inject(t._p, u._p, z, x, c, 2, 6, 1.0, 0.0, 1) == \
        b"pos is out of the bound."
    x = ull(1, 32)
    assert lib.qdc_pauli_overlap(t._p, u._p, x, z, c, 0, 6, out) == b"The observable has no terms."
    assert lib.qdc_pauli_overlap_inject(t._p, u._p, x, z, c, 0, 6, 1.0, 0.0, 0) == \
        b"The observable has no terms."
    msg = lib.qdc_pauli_overlap(t._p, u._p, x, z, dbl(1.0, float("inf")), 2, 6, out)
    assert msg == b"Pauli coefficients must be finite."
    msg = lib.qdc_pauli_overlap_inject(t._p, u._p, x, z, c, 2, 6, 1.0, float("nan"), 1)
    assert msg == b"Pauli coefficients must be finite."
    assert lib.qdc_overlap_inject(t._p, u._p, 6, float("inf"), 0.0, 1) == \
        b"Pauli coefficients must be finite."
    assert lib.qdc_overlap_inject(t._p, t._p, 6, 1.0, 0.0, 1) == \
        b"fwd and bwd must be different states."
    assert lib.qdc_pauli_overlap_inject(t._p, t._p, x, z, c, 2, 6, 1.0, 0.0, 1) == \
        b"fwd and bwd must be different states."
    for msg in (lib.qdc_overlap(t._p, u._p, 41, out),
                lib.qdc_pauli_overlap(t._p, u._p, x, z, c, 2, 41, out),
                lib.qdc_overlap_inject(t._p, u._p, 41, 1.0, 0.0, 1)):
        assert msg is not None and b"supported range" in msg
    assert (out[0], out[1]) == (0.0, 0.0)
    # and a valid call through the raw symbol: <0|(Z5 + Z5 X0)|0> = 1
    assert lib.qdc_pauli_overlap(t._p, u._p, ull(0, 1), ull(32, 32), c, 2, 6, out) is None
    assert (out[0], out[1]) == (1.0, 0.0)

"""Sampling from |psi|^2 on the host (include/qdc/sample.h: qdc_sample, qdc_sample_plan,
qdc_sample_assign; csrc/qdc_sample.hpp): the entry points, the plan, the step between the two
passes against numpy (long-double cumsum, searchsorted(side="right"), a clamp to the last
segment with mass), and the panics that need no GPU."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
PRECS = ["f32", "f64"]
LAST_U = np.nextafter(1.0, 0.0)


def reference_segments(seg_sums, u):
    """(segment, t, inclusive long-double prefix, N) by the definition: the first segment whose
    inclusive prefix exceeds t = u N, clamped to the last segment with mass."""
    ss = np.asarray(seg_sums, dtype=np.float64)
    c = np.cumsum(ss.astype(np.longdouble))
    total = float(c[-1])
    t = np.asarray(u, dtype=np.float64) * total
    seg = np.searchsorted(c, t.astype(np.longdouble), side="right")
    return np.minimum(seg, np.flatnonzero(ss > 0)[-1]), t, c, total


def test_symbols_present():
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import _native
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    header = (ROOT / "include" / "qdc" / "sample.h").read_text()
    for name in ("qdc_sample", "qdc_sample_plan", "qdc_sample_assign"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _native.RUNTIME
        for prec in PRECS:
            assert hasattr(ctypes.CDLL(str(_native.lib_path(prec))), name), (name, prec)
    for name in ("sample_plan", "sample_assign"):
        assert name in q.__all__ and callable(getattr(q, name))
    for name in ("sample", "sample_counts", "norm_sq"):
        assert callable(getattr(q.QuantizedTensor, name))
    assert callable(DenseCircuit.get_sample_op)


@pytest.mark.parametrize("prec", PRECS)
def test_plan(prec):
    from quantum_differentiable_circuit import sample_plan
    g = sample_plan(20, prec)["G"]
    assert 1 <= g <= 16
    for n in (0, 1, g - 1, g, g + 1, 28, 40):
        p = sample_plan(n, prec)
        want = max(1, 1 << max(0, n - g))
        assert p["G"] == g and p["segments"] == want and p["locate_blocks"] == want, (n, p)
        assert p["span"] == (1 << 11 if prec == "f32" else 1 << 10)
    assert sample_plan(41, prec) is None


@pytest.mark.parametrize("prec", PRECS)
def test_assign_hand_made_segments(prec):
    """Zero-mass segments at the start, in the middle and at the end are never chosen; u = 0
    gives the first segment with mass, u = nextafter(1, 0) the last; a u exactly on a boundary
    (exact binary fractions: boundaries at 1/4, 1/2, 3/4) goes to the upper segment."""
    from quantum_differentiable_circuit import sample_assign
    ss = np.array([0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0])  # N = 4
    u = np.array([0.0, LAST_U, 0.25, 0.5, 0.75, 0.125, np.nextafter(0.25, 0.0),
                  np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), 0.2, 0.3, 0.9])
    seg, resid, perm, total = sample_assign(ss, u, prec)
    assert total == 4.0
    assert list(seg) == [2, 8, 4, 7, 8, 2, 2, 4, 7, 2, 4, 8]
    assert np.all(ss[seg.astype(np.int64)] > 0)
    want_seg, t, c, _ = reference_segments(ss, u)
    assert np.array_equal(seg, want_seg.astype(np.uint64))
    excl = np.concatenate([[0.0], np.asarray(c[:-1], dtype=np.float64)])  # exact here
    assert np.array_equal(resid, t - excl[seg.astype(np.int64)])
    assert resid[0] == 0.0 and resid[2] == 0.0 and resid[3] == 0.0 and resid[4] == 0.0


def check_perm(seg, resid, perm):
    n = seg.size
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.uint64))
    p = perm.astype(np.int64)
    s, r = seg[p].astype(np.int64), resid[p]
    assert np.all(np.diff(s) >= 0)
    same = np.diff(s) == 0
    assert np.all(np.diff(r)[same] >= 0)


@pytest.mark.parametrize("prec", PRECS)
def test_assign_random_against_numpy(prec):
    """10^5 shots over 64 random segment sums (some zero): numpy's segment for every shot, at
    most 5 exceptions and those inside the bracket at segment level; perm orders by (segment,
    residual); every residual in [0, seg_sum] up to one ulp of N."""
    from quantum_differentiable_circuit import sample_assign
    rng = np.random.default_rng(5)
    ss = rng.random(64) * 10.0 ** rng.integers(-6, 3, 64)
    ss[[0, 1, 17, 40, 41, 63]] = 0.0
    u = rng.random(100_000)
    u[0], u[1] = 0.0, LAST_U
    seg, resid, perm, total = sample_assign(ss, u, prec)
    want, t, c, n = reference_segments(ss, u)
    assert total == n
    s = seg.astype(np.int64)
    assert np.all(ss[s] > 0)
    assert s[0] == 2 and s[1] == 62
    bad = np.flatnonzero(s != want)
    print(f"{prec}: {bad.size} of {u.size} shots off numpy's segment")
    assert bad.size <= 5
    tol = np.longdouble((64 + 4) * 2.0 ** -52 * n)
    cl = np.concatenate([[np.longdouble(0)], c])
    for k in bad:
        assert cl[s[k]] - tol <= t[k] < cl[s[k] + 1] + tol
    check_perm(seg, resid, perm)
    ulp = np.spacing(n)
    assert np.all(resid >= 0.0) and np.all(resid <= ss[s] + ulp)
    # the residual is t minus the exclusive prefix, rounded once
    want_r = np.maximum((t.astype(np.longdouble) - cl[s]).astype(np.float64), 0.0)
    assert np.array_equal(resid, want_r)


@pytest.mark.parametrize("prec", PRECS)
def test_assign_ties_and_single_segment(prec):
    from quantum_differentiable_circuit import sample_assign
    u = np.array([0.5, 0.25, 0.5, 0.0, 0.25])
    seg, resid, perm, total = sample_assign([3.0], u, prec)
    assert total == 3.0 and not seg.any()
    assert np.array_equal(resid, u * 3.0)
    assert list(perm) == [3, 1, 4, 0, 2]  # ties keep the caller's order
    seg, resid, perm, total = sample_assign([1.0, 0.0, 2.0], np.zeros(0), prec)
    assert total == 3.0 and seg.size == 0 and perm.size == 0
    # no shots: a zero or non-finite total is returned, not raised
    assert sample_assign([0.0, 0.0], np.zeros(0), prec)[3] == 0.0
    assert sample_assign([1.0, np.inf], np.zeros(0), prec)[3] == np.inf


@pytest.mark.parametrize("prec", PRECS)
def test_panics(prec):
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import sample_assign
    ss = [1.0, 2.0]
    for bad in (np.nan, -0.25, 1.0, 1.5, -np.inf, np.inf):
        with pytest.raises(q.PanicException, match=r"uniforms must be in \[0, 1\)\."):
            sample_assign(ss, [0.5, bad], prec)
    with pytest.raises(q.PanicException, match="The state has zero norm."):
        sample_assign([0.0, 0.0, 0.0], [0.5], prec)
    for bad in (np.inf, np.nan):
        with pytest.raises(q.PanicException, match="The state is not finite."):
            sample_assign([1.0, bad], [0.5], prec)
    with pytest.raises(q.PanicException, match="The sample has no segment sums."):
        sample_assign([], [0.5], prec)
    # -0.0 is a uniform (it equals 0); the largest double below 1 is one too
    seg, _, _, _ = sample_assign(ss, [-0.0, LAST_U], prec)
    assert list(seg) == [0, 1]
    lib = q._native.load(prec)
    one = (ctypes.c_double * 1)(0.5)
    out = (ctypes.c_ulonglong * 1)()
    # the checks that come before any GPU work (this box may have none)
    assert lib.qdc_sample_plan(41, (ctypes.c_uint * 4)()) == ctypes.c_size_t(-1).value
    assert lib.qdc_sample_plan(3, None) == ctypes.c_size_t(-1).value
    err = lib.qdc_sample_assign(one, 1, None, 1, out, one, out, None)
    assert err and b"The sample has no uniforms." in err
    err = lib.qdc_sample_assign(one, 1, one, 1, None, one, out, None)
    assert err and b"The sample has no output buffers." in err

"""Sampling from |psi|^2 on the device (QuantizedTensor.sample / sample_counts / norm_sq over
qdc_sample, include/qdc/sample.h; k_sample_sums and k_sample_locate, csrc/qdc_sample.hpp).

The reference is numpy: p = re^2 + im^2 in double, C = a sequential long-double cumsum, N = C[-1],
t = u N, searchsorted(C, t, side="right"), a clamp to the last index with p > 0.  The sizes come
from sample_plan (G = log2 of a segment, L = log2 of a span): a state below a chunk, below a
span, exactly one span, exactly one segment, 2 and 4 segments."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PRECS = ["f32", "f64"]
DTYPE = {"f32": np.complex64, "f64": np.complex128}
LAST_U = np.nextafter(1.0, 0.0)


@functools.lru_cache(maxsize=None)
def geometry(prec):
    """(G, L, amplitudes of a chunk, amplitudes of a thread's run, the test sizes)"""
    from quantum_differentiable_circuit import sample_plan
    p = sample_plan(20, prec)
    g, span = int(p["G"]), int(p["span"])
    lw = span.bit_length() - 1
    vec = 16 // np.dtype(DTYPE[prec]).itemsize
    sizes = sorted({0, 1, 2, lw - 1, lw, lw + 1, g - 1, g, g + 1, g + 2})
    return g, lw, vec, span // 256, sizes


def tensor(psi, prec):
    from quantum_differentiable_circuit import QuantizedTensor
    return QuantizedTensor.new_from_host(np.ascontiguousarray(psi, dtype=DTYPE[prec]), prec)


@functools.lru_cache(maxsize=None)
def half_zero_state(n, prec):
    """numpy seed 7, complex normal, half the entries exactly 0 (not normalised)"""
    rng = np.random.default_rng(7)
    size = 1 << n
    psi = rng.standard_normal(size) + 1j * rng.standard_normal(size)
    psi[rng.random(size) < 0.5] = 0.0
    if not psi.any():
        psi[size - 1] = 1.0
    psi = psi.astype(DTYPE[prec])
    psi.setflags(write=False)
    return psi


def probabilities(psi):
    return psi.real.astype(np.float64) ** 2 + psi.imag.astype(np.float64) ** 2


@functools.lru_cache(maxsize=None)
def reference_cdf(n, prec):
    """(p, C, N) of half_zero_state(n, prec): computed once, shared, read-only"""
    p = probabilities(half_zero_state(n, prec))
    c = np.cumsum(p.astype(np.longdouble))
    p.setflags(write=False)
    c.setflags(write=False)
    return p, c, float(c[-1])


def reference_sample(p, c, total, u):
    t = u * total
    idx = np.searchsorted(c, t.astype(np.longdouble), side="right")
    return np.minimum(idx, np.flatnonzero(p > 0)[-1]).astype(np.uint64), t


@functools.lru_cache(maxsize=None)
def shots_200k():
    u = np.random.default_rng(11).random(200_000)
    u[0], u[1] = 0.0, LAST_U
    u.setflags(write=False)
    return u


def boundary_indices(n, prec):
    g, lw, vec, run, _ = geometry(prec)
    js = {0, 1, (1 << n) - 1}
    for b in (vec, run, 1 << lw, 1 << g, 3 << g):
        js |= {b - 1, b, b + 1}
    return sorted(j for j in js if 0 <= j < (1 << n))


@pytest.mark.parametrize("prec", PRECS)
def test_basis_states(prec):
    """|j> for j = 0, 1, 2^n - 1 and one below, on and one above every chunk, thread-run, span
    and segment boundary that exists at n: 4096 shots each, all equal to j."""
    u = np.random.default_rng(1).random(4096)
    u[0], u[1] = 0.0, LAST_U
    for n in geometry(prec)[4]:
        psi = np.zeros(1 << n, DTYPE[prec])
        t = tensor(psi, prec)
        for j in boundary_indices(n, prec):
            psi[:] = 0
            psi[j] = 1.0
            t.set_from_host(psi)
            out = t.sample(u.size, uniforms=u)
            assert out.dtype == np.uint64 and out.shape == (u.size,)
            assert np.all(out == j), (n, j, np.unique(out)[:8])


@pytest.mark.parametrize("prec", PRECS)
def test_exact_quarters(prec):
    """Amplitude 1/2 on four indices in different threads, spans and segments where n allows;
    u_k = k / 4096: exactly idx[floor(4 u_k)], u = 1/4, 1/2, 3/4 going to the upper index."""
    g, lw, vec, run, sizes = geometry(prec)
    u = np.arange(4096) / 4096.0
    for n in sizes:
        if n < 2:
            continue
        size = 1 << n
        prefer = [1, run + 2, (1 << lw) + run + 3, (1 << g) + (3 << lw) + 5, (3 << g) + 7,
                  size - 1, size - 2, 0, 2]
        idx = []
        for c in prefer:
            if 0 <= c < size and c not in idx and len(idx) < 4:
                idx.append(c)
        idx = np.array(sorted(idx), dtype=np.uint64)
        psi = np.zeros(size, DTYPE[prec])
        psi[idx.astype(np.int64)] = 0.5
        t = tensor(psi, prec)
        assert t.norm_sq() == 1.0
        out = t.sample(u.size, uniforms=u)
        assert np.array_equal(out, idx[np.floor(4.0 * u).astype(np.int64)]), (n, idx)
        for k, q in ((1024, 1), (2048, 2), (3072, 3)):
            assert out[k] == idx[q] and out[k - 1] == idx[q - 1]


def random_sizes(prec):
    g, lw, _, _, _ = geometry(prec)
    return sorted({lw + 1, 14, g + 2})


@pytest.mark.parametrize("prec", PRECS)
def test_random_half_zero_state(prec):
    """200 000 shots (seed 11, u[0] = 0, u[1] = nextafter(1, 0)) at n = L + 1, 14, G + 2: every
    shot has p > 0 and lies inside the bracket C[out - 1] - tol <= t < C[out] + tol with
    tol = (2^n + 4) 2^-52 N (the worst case of two double summations of 2^n non-negative terms);
    at most 5 shots differ from the reference index (a cap: on the host, sequential double,
    sequential long double and a two-level blocked order agree on every shot at these sizes)."""
    u = shots_200k()
    for n in random_sizes(prec):
        p, c, total = reference_cdf(n, prec)
        want, t = reference_sample(p, c, total, u)
        out = tensor(half_zero_state(n, prec), prec).sample(u.size, uniforms=u)
        o = out.astype(np.int64)
        assert np.all(out < (1 << n))
        assert np.all(p[o] > 0)
        assert o[0] == np.flatnonzero(p > 0)[0] and o[1] == np.flatnonzero(p > 0)[-1]
        tol = np.longdouble((2.0 ** n + 4) * 2.0 ** -52 * total)
        cl = np.concatenate([[np.longdouble(0)], c])
        tl = t.astype(np.longdouble)
        assert np.all(cl[o] - tol <= tl) and np.all(tl < cl[o + 1] + tol)
        diff = int(np.count_nonzero(out != want))
        print(f"{prec} n={n}: {diff} of {u.size} shots off the reference, tol/N {float(tol) / total:.1e}")
        assert diff <= 5


@pytest.mark.parametrize("prec", PRECS)
def test_monotone_and_order(prec):
    """Sorted uniforms give non-decreasing indices; a shuffled copy gives the same index for the
    same uniform (out[k] follows u[k])."""
    u = shots_200k()
    rng = np.random.default_rng(12)
    for n in random_sizes(prec):
        t = tensor(half_zero_state(n, prec), prec)
        out = t.sample(u.size, uniforms=u)
        srt = t.sample(u.size, uniforms=np.sort(u))
        assert np.all(np.diff(srt.astype(np.int64)) >= 0)
        assert np.array_equal(srt, np.sort(out))
        perm = rng.permutation(u.size)
        assert np.array_equal(t.sample(u.size, uniforms=u[perm]), out[perm])


@pytest.mark.parametrize("prec", PRECS)
def test_scale_determinism_and_norm(prec):
    """The state times 4 (an exact scaling): the same indices bit for bit, norm_sq exactly 16
    times; two calls agree; the state is unchanged; norm_sq against the long-double sum."""
    u = shots_200k()[:50_000]
    for n in geometry(prec)[4]:
        psi = half_zero_state(n, prec)
        p, c, total = reference_cdf(n, prec)
        t = tensor(psi, prec)
        out = t.sample(u.size, uniforms=u)
        assert np.array_equal(t.sample(u.size, uniforms=u), out)
        assert np.array_equal(t.get_cpu_state_copy().view(np.uint8), psi.view(np.uint8))
        n2 = t.norm_sq()
        assert abs(n2 - total) <= (2.0 ** n) * 2.0 ** -52 * total
        t4 = tensor(psi * DTYPE[prec](4.0), prec)
        assert np.array_equal(t4.sample(u.size, uniforms=u), out)
        assert t4.norm_sq() == 16.0 * n2


@pytest.mark.parametrize("prec", PRECS)
def test_qubits_counts_and_generators(prec):
    n = geometry(prec)[0] + 1
    t = tensor(half_zero_state(n, prec), prec)
    u = shots_200k()[:20_000]
    full = t.sample(u.size, uniforms=u)
    qs = [3, 0, n - 1, 7]
    want = np.zeros(u.size, np.uint64)
    for b, q in enumerate(qs):
        want |= ((full >> np.uint64(q)) & np.uint64(1)) << np.uint64(b)
    assert np.array_equal(t.sample(u.size, uniforms=u, qubits=qs), want)
    assert np.array_equal(t.sample(u.size, uniforms=u, qubits=[]), np.zeros(u.size, np.uint64))
    vals, cnt = t.sample_counts(u.size, uniforms=u)
    assert cnt.sum() == u.size and np.array_equal(vals, np.unique(full))
    vals, cnt = t.sample_counts(u.size, uniforms=u, qubits=[n - 1])
    assert cnt.sum() == u.size and set(vals) <= {0, 1}
    # seed: default_rng(seed).random(shots); a Generator is advanced
    by_seed = t.sample(1000, seed=5)
    assert np.array_equal(by_seed, t.sample(1000, uniforms=np.random.default_rng(5).random(1000)))
    assert np.array_equal(by_seed, t.sample(1000, 5))
    rng = np.random.default_rng(5)
    assert np.array_equal(t.sample(1000, rng=rng), by_seed)
    assert not np.array_equal(t.sample(1000, rng=rng), by_seed)
    assert t.sample(0).shape == (0,) and t.sample(0).dtype == np.uint64


def exact_uniform_state(n, prec):
    """Every p = 2^-n exactly, built on the device from |0..0> by exact one-qubit gates (entries
    1 or 1/2: sums with zero, products with powers of two), so no 2^n host array is needed."""
    from quantum_differentiable_circuit import QuantizedTensor
    dt = DTYPE[prec]
    t = QuantizedTensor.new_standard(n, prec)
    halves = (n + 1) // 2
    for q in range(n):
        a = 0.5 if q < halves else 1.0
        t.apply_q1_gate(np.full(4, a, dt), q)
    if n & 1:  # amplitude 2^-(n+1)/2: times (1 + i) gives p = 2^-n
        t.apply_q1_gate(np.array([1 + 1j, 0, 0, 1 + 1j], dt), 0)
    return t


def ghz_state(n, prec):
    from quantum_differentiable_circuit import QuantizedTensor, get_cnot, get_hadamard
    t = QuantizedTensor.new_standard(n, prec)
    t.apply_q1_gate(get_hadamard(prec), 0)
    cnot = get_cnot(prec)
    for q in range(n - 1):
        t.apply_q2_gate(cnot, q, q + 1)  # control q (pos2), target q + 1
    return t


@pytest.mark.parametrize("prec", PRECS)
def test_device_built_states_are_exact(prec):
    """The constructions of the full-size test, checked amplitude by amplitude at n = 11, 12."""
    for n in (11, 12):
        psi = exact_uniform_state(n, prec).get_cpu_state_copy()
        amp = (1 + 1j) * 2.0 ** (-(n + 1) // 2) if n & 1 else 2.0 ** (-n // 2)
        assert np.array_equal(psi, np.full(1 << n, amp, DTYPE[prec]))
        assert np.all(probabilities(psi) == 2.0 ** -n)
        ghz = ghz_state(n, prec).get_cpu_state_copy()
        assert ghz[0] == ghz[-1] != 0 and np.count_nonzero(ghz) == 2


@pytest.mark.parametrize("prec", PRECS)
def test_full_size(prec):
    """n = 28 (f32) / 27 (f64), 2 GiB of state.  The uniform state (all partial sums exact):
    out[k] == floor(u_k 2^n) for every one of 10^5 shots.  GHZ: only 0 and 2^n - 1, split at
    u = 1/2 exactly."""
    n = 28 if prec == "f32" else 27
    u = np.random.default_rng(13).random(100_000)
    u[:4] = 0.0, LAST_U, 0.5, np.nextafter(0.5, 0.0)
    t = exact_uniform_state(n, prec)
    assert t.norm_sq() == 1.0
    out = t.sample(u.size, uniforms=u)
    assert np.array_equal(out, np.floor(u * 2.0 ** n).astype(np.uint64))
    del t
    t = ghz_state(n, prec)
    out = t.sample(u.size, uniforms=u)
    assert np.array_equal(out, np.where(u < 0.5, 0, (1 << n) - 1).astype(np.uint64))
    assert out[2] == (1 << n) - 1 and out[3] == 0


@pytest.mark.parametrize("prec", PRECS)
def test_panics(prec):
    import quantum_differentiable_circuit as q
    n = 5
    t = tensor(half_zero_state(n, prec), prec)
    for bad in (np.nan, -0.5, 1.0, np.inf):
        with pytest.raises(q.PanicException, match=r"uniforms must be in \[0, 1\)\."):
            t.sample(3, uniforms=[0.1, bad, 0.2])
    for qs in ([0, 0], [n], [1, 2, 1], [-1]):
        with pytest.raises(q.PanicException, match="pos is out of the bound."):
            t.sample(10, seed=1, qubits=qs)
    with pytest.raises(q.PanicException, match="positions must be different."):
        t.sample(10, seed=1, rng=np.random.default_rng(1))
    zero = tensor(np.zeros(1 << n), prec)
    assert zero.norm_sq() == 0.0
    with pytest.raises(q.PanicException, match="The state has zero norm."):
        zero.sample(4, seed=0)
    assert zero.sample(0).size == 0
    psi = np.array(half_zero_state(n, prec))
    psi[3] = np.inf
    with pytest.raises(q.PanicException, match="The state is not finite."):
        tensor(psi, prec).sample(4, seed=0)
    psi[3] = np.nan
    with pytest.raises(q.PanicException, match="The state is not finite."):
        tensor(psi, prec).sample(4, seed=0)
    lib = q._native.load(prec)
    err = lib.qdc_sample(t._p, 41, None, 0, None, None)
    assert err and b"pos is out of the bound." in err
    err = lib.qdc_sample(t._p, n, None, 2, None, None)
    assert err and b"The sample has no uniforms." in err

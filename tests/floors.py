"""Measured floating-point floors for multi-gate parity tests (test infrastructure).

A fixed tolerance on a circuit either hides real errors (a wrong gradient stage of relative
size 1e-4 passes a 2e-3 bound) or fails deep circuits, because rounding error grows with depth.
Instead, every multi-gate GPU parity test measures the floor of THE SAME circuit: the
reference's own algorithm run in the build's precision — the C restatement of its kernels
(oracle/cpu_ref.c, index rules of src/primitives.cu:176-953) driven by the oracle's
restatement of src/circuit.rs:164-429 (unfused: uncompute, gradient, pull-back per gate,
allocate-conj-gate-add per density) — against the exact result (the einsum oracle in
complex128).  The HIP path must stay within RATIO x that floor (plus ATOL, one rounding of
the working precision, for outputs whose floor is exactly zero).  Every check prints the
measured error, the floor and their ratio.

Norm-relative error throughout: max |a - b| / max |b| over the flattened output group.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle.cref import CRefOps

RATIO = 4.0
ATOL = {"f32": 2.4e-7, "f64": 1e-15}
DT = {"f32": np.complex64, "f64": np.complex128}


def flat(xs):
    if isinstance(xs, np.ndarray):
        return xs.reshape(-1)
    return np.concatenate([np.asarray(x).reshape(-1) for x in xs]) if len(xs) else np.zeros(0)


def l2rel(a, b):
    """2-norm relative error ||a - b|| / ||b||: an aggregate over every element, so one circuit's
    value is a stable statistic of its rounding (the max-norm of normrel is the extreme of 2^n
    random-walk endpoints and varies ~0.3-2x between realizations, tools/drift_trace.py)."""
    a, b = flat(a).astype(np.complex128), flat(b).astype(np.complex128)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))


def normrel(a, b):
    a, b = flat(a).astype(np.complex128), flat(b).astype(np.complex128)
    den = np.abs(b).max() if b.size else 0.0
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a - b).max())


def sigma_z_cots(dens, dt):
    """Cotangents of sum Re tr(rho Z x Z...) (diagonal +-1, Hermitian)."""
    return [np.ascontiguousarray(np.diag([1.0, -1.0] if d.shape == (2, 2)
                                         else [1.0, -1.0, -1.0, 1.0]).astype(dt)) for d in dens]


def tsallis_cots(dens, dt):
    """conj of the JAX cotangents of the mean Tsallis-2 entropy (test_autodiff.py:87-92,
    circuit.py:193), from complex128 densities."""
    _, cots = O.tsallis_loss_and_cotangents([np.asarray(d, np.complex128) for d in dens])
    return [np.ascontiguousarray(x.conj(), dtype=dt) for x in cots]


def oracle_outputs(n, ins, const, var, psi0=None, cots=None, ops=None, run=True):
    """run / forward densities, gradients and the states of one call sequence
    (run, forward, backward) on the oracle circuit with op table `ops` (None: complex128
    einsum).  `cots`: the cotangents to feed backward (a callable of the forward densities,
    or a list)."""
    o = O.OracleCircuit(n, np.complex128, ops=ops or O.EinsumOps)
    for kind, pos in ins:
        o.add(kind, *pos)
    if psi0 is not None:
        o.set_state_from_vector(psi0)
    out = {}
    if run:
        out["run"] = o.run(const, var)
    out["forward"] = o.forward(const, var)
    out["state"] = np.asarray(o.state, np.complex128).copy()
    if cots is not None:
        cl = cots(out["forward"]) if callable(cots) else cots
        out["cots"] = cl
        out["grads"] = o.backward(cl, const, var)
        out["uncomputed"] = np.asarray(o.state, np.complex128).copy()
        if o.bwd is not None:
            out["bwd"] = np.asarray(o.bwd, np.complex128).copy()
    return out


class Floor:
    """The exact outputs of a circuit and the floor of each output group."""

    def __init__(self, prec, n, ins, const, var, psi0=None, cots=sigma_z_cots, run=True,
                 exact_ops=None):
        """exact_ops: the op table of the exact result (None: the complex128 einsum oracle;
        CRefOps("f64") at sizes where einsum is too slow — then `prec` must be "f32", whose
        floor is ~1e9 times the f64 restatement's own rounding)."""
        self.prec = prec
        dt = DT[prec]
        self.const = [np.ascontiguousarray(g, dtype=dt) for g in const]
        self.var = [np.ascontiguousarray(g, dtype=dt) for g in var]
        self.psi0 = None if psi0 is None else np.ascontiguousarray(psi0, dtype=dt)
        # exact result of the build-precision inputs; the cotangents are computed once (from
        # the exact forward densities) and fed to every run
        exact = oracle_outputs(n, ins, self.const, self.var, self.psi0,
                               (lambda d: cots(d, dt)) if cots is not None else None, ops=exact_ops,
                               run=run)
        self.cots = exact.get("cots")
        ref = oracle_outputs(n, ins, self.const, self.var, self.psi0, self.cots, ops=CRefOps(prec),
                             run=run)
        self.exact = exact
        self.ref = ref
        self.floor = {k: normrel(ref[k], exact[k]) for k in exact if k != "cots"}
        self.floor_l2 = {k: l2rel(ref[k], exact[k]) for k in exact if k != "cots"}

    def check(self, key, got, what="", ratio=RATIO):
        err = normrel(got, self.exact[key])
        fl = self.floor[key]
        bound = ratio * fl + ATOL[self.prec]
        # which term admits the result: ratio x floor alone, or only with the one-rounding ATOL
        binding = "floor" if err <= ratio * fl else "ATOL"
        print(f"[floor] {what}{key}: err {err:.3e}  floor {fl:.3e}  "
              f"ratio {err / fl if fl > 0 else float('inf'):.2f}  bound {bound:.3e}  "
              f"passes-by {binding}")
        assert err <= bound, f"{what}{key}: error {err:.3e} > {ratio} x floor {fl:.3e} + atol"
        return err


    def check_l2(self, key, got, what="", ratio=RATIO):
        """As check, in the 2-norm: the stable aggregate of the same rounding (state outputs)."""
        err = l2rel(got, self.exact[key])
        fl = self.floor_l2[key]
        bound = ratio * fl + ATOL[self.prec]
        binding = "floor" if err <= ratio * fl else "ATOL"
        print(f"[floor-l2] {what}{key}: err {err:.3e}  floor {fl:.3e}  "
              f"ratio {err / fl if fl > 0 else float('inf'):.2f}  bound {bound:.3e}  "
              f"passes-by {binding}")
        assert err <= bound, f"{what}{key}: 2-norm error {err:.3e} > {ratio} x floor {fl:.3e} + atol"
        return err


def check_pair(prec, a, b, floor_value, what, ratio=2 * RATIO):
    """Two HIP results of the same circuit (e.g. sharded vs unsharded, fused vs unfused): each is
    within RATIO x floor of the exact result, so they differ by at most 2 RATIO x floor."""
    err = normrel(a, b)
    bound = ratio * floor_value + 2 * ATOL[prec]
    binding = "floor" if err <= ratio * floor_value else "ATOL"
    print(f"[floor] {what}: diff {err:.3e}  floor {floor_value:.3e}  bound {bound:.3e}  "
          f"passes-by {binding}")
    assert err <= bound, f"{what}: difference {err:.3e} > {ratio} x floor {floor_value:.3e}"
    return err


# ---------------------------------------------------------------------------------------
# Element-scale accuracy on polarised states
#
# normrel divides by the largest element of a group and cmp_complex_slices sees only Haar-like
# states, whose density diagonals all sit near 2^-k: neither notices a kernel that forms a small
# output as the difference of two large ones, or a summation order that swamps small terms.
# Here the inputs are near-product states with up to three qubits polarised to `small`, and every
# output element is measured against ITS OWN scale, the Cauchy-Schwarz bound of its sum:
#   density on positions:  scale[r, c] = sqrt(rho_rr rho_cc)
#   gradient G[r, c] = sum_g bwd[r, g] fwd[c, g]:  scale[r, c] = ||bwd_r|| ||fwd_c||
# (|err| <= gamma sum |b||f| <= gamma scale for a sum in any order, so the metric is fair to any
# correct kernel).  The bound is the usual one: RATIO x floor + ATOL, the floor being the same
# metric of the reference's algorithm (CRefOps) in build precision on the same inputs, worst
# over a case's positions and both phase variants.
# ---------------------------------------------------------------------------------------
SMALL = {"f32": 1e-6, "f64": 1e-12}
# smallest |psi_i|^2 a polarised state may hold, so that nothing depends on denormal handling
# (which the CPU reference and the GPU may do differently): 1e-30 in f32, eight decades above
# the smallest normal 1.2e-38.  Three qubits polarised to 1e-12 put f64 amplitudes at
# |psi|^2 ~ 1e-36 2^-(n-3), so f64 keeps the same eight decades above ITS smallest normal
# (2.2e-308) instead.
MIN_POWER = {"f32": 1e-30, "f64": 1e-300}


def polarised_state(n, small, near_one=(), near_zero=(), phases="product", seed=0, prec="f64"):
    """psi[i] = prod_q a_q(bit_q(i)) exp(i phi_i) (1 + 1e-3 g_i), normalised, in complex128.
    A qubit of near_one has |a_q(0)|^2 = small, one of near_zero |a_q(1)|^2 = small, every other
    qubit is balanced; g_i is standard complex normal.  phases="product": phi_i is a sum of
    per-qubit phases (coherent off-diagonals at full Cauchy-Schwarz scale); "random": one
    uniform phase per amplitude (off-diagonals are sums of 2^(n-k) random terms).  Asserts that
    every |psi_i|^2 of the cast to `prec` is at least MIN_POWER[prec]."""
    assert phases in ("product", "random"), phases
    assert not set(near_one) & set(near_zero)
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0, 2 * np.pi, n)
    psi = np.ones(1, np.complex128)
    for q in range(n - 1, -1, -1):  # kron: the last factor is bit 0
        p0 = small if q in near_one else 1 - small if q in near_zero else 0.5
        a = np.sqrt(np.array([p0, 1 - p0])).astype(np.complex128)
        if phases == "product":
            a[1] *= np.exp(1j * theta[q])
        psi = np.kron(psi, a)
    if phases == "random":
        psi = psi * np.exp(1j * rng.uniform(0, 2 * np.pi, psi.size))
    g = (rng.standard_normal(psi.size) + 1j * rng.standard_normal(psi.size)) / np.sqrt(2)
    psi = psi * (1 + 1e-3 * g)
    psi /= np.linalg.norm(psi)
    power = np.abs(psi.astype(DT[prec]).astype(np.complex128)) ** 2
    assert power.min() >= MIN_POWER[prec], \
        f"polarised state holds |psi|^2 = {power.min():.1e} < {MIN_POWER[prec]:.0e} in {prec}"
    return psi


def groups(state, positions):
    """state as [local index on `positions` (positions[0] most significant), everything else]."""
    n, k = O.qubits_of(np.asarray(state).size), len(positions)
    axes = [n - 1 - p for p in positions]
    return np.moveaxis(np.asarray(state).reshape([2] * n), axes, range(k)).reshape(1 << k, -1)


def grad_scale(fwd, bwd, positions):
    """scale[r, c] = ||bwd_r|| ||fwd_c|| of G[r, c] = sum_g bwd[r, g] fwd[c, g], flat."""
    nb = np.linalg.norm(groups(np.asarray(bwd, np.complex128), positions), axis=1)
    nf = np.linalg.norm(groups(np.asarray(fwd, np.complex128), positions), axis=1)
    return np.outer(nb, nf).reshape(-1)


def grad_diag_scale(fwd, bwd, positions):
    """The four ||bwd_r|| ||fwd_r|| of get_q2_grad_diag."""
    nb = np.linalg.norm(groups(np.asarray(bwd, np.complex128), positions), axis=1)
    nf = np.linalg.norm(groups(np.asarray(fwd, np.complex128), positions), axis=1)
    return nb * nf


def density_scale(state, positions):
    """scale[r, c] = sqrt(rho_rr rho_cc), flat."""
    return grad_scale(state, state, positions)


def density_scale_of(rho):
    """The same scale from an exact density matrix (a circuit's densities)."""
    d = np.sqrt(np.abs(np.diag(np.asarray(rho, np.complex128))))
    return np.outer(d, d).reshape(-1)


def elemrel(got, want, scale):
    """max over elements of |got - want| / scale, in complex128."""
    got = np.asarray(got).astype(np.complex128).reshape(-1)
    want = np.asarray(want).astype(np.complex128).reshape(-1)
    scale = np.asarray(scale, np.float64).reshape(-1)
    assert got.shape == want.shape == scale.shape, (got.shape, want.shape, scale.shape)
    return float((np.abs(got - want) / scale).max())


def check_elem(prec, what, err, floor, ratio=RATIO, failures=None):
    """As Floor.check, for an elemrel error against its floor.  failures: a list that collects the
    failing checks instead of raising at the first (the caller asserts it is empty)."""
    bound = ratio * floor + ATOL[prec]
    binding = "floor" if err <= ratio * floor else "ATOL" if err <= bound else "FAILS"
    print(f"[floor-elem] {what}: err {err:.3e}  floor {floor:.3e}  "
          f"ratio {err / floor if floor > 0 else float('inf'):.2f}  bound {bound:.3e}  "
          f"passes-by {binding}")
    if failures is not None:
        if not err <= bound:
            failures.append(f"{what}: {err:.3e} > {bound:.3e}")
    else:
        assert err <= bound, f"{what}: elemrel {err:.3e} > {ratio} x floor {floor:.3e} + atol"
    return err


# ---- the polarised primitive cases shared by tests/test_polarised_cpu.py and
# tests/test_gpu_polarised.py ----
PHASES = ("product", "random")
BALANCED = (3, 7)  # balanced in both sets at every n >= 11


def polarised_sets(n):
    """Two sets of three polarised qubits: between them the in-chunk bit, the lane bits, the
    tile bits and the top bit."""
    return ({"near_one": (0, n - 1), "near_zero": (5,)},
            {"near_one": (1, 9), "near_zero": (n - 2,)})


def polarised_qubits(n, which):
    s = polarised_sets(n)[which]
    return tuple(s["near_one"]) + tuple(s["near_zero"])


def structured_pairs(n, which):
    """Both orders of (polarised, polarised), (polarised, balanced), (balanced, balanced)."""
    p = polarised_qubits(n, which)
    b0, b1 = BALANCED
    pairs = [(p[0], p[1]), (p[0], p[2]), (p[2], b0), (p[0], b1), (p[1], b0), (b0, b1)]
    return pairs + [(c, d) for d, c in pairs]


_PAIRS = {}


def polarised_pair(prec, n, which, phases):
    """(fwd, bwd) in build precision, shared and never modified: fwd polarised on set `which`;
    bwd another seed with one polarisation flipped, so the gradient's element scales span
    about 12 (f32) / 24 (f64) orders of magnitude."""
    key = (prec, n, which, phases)
    if key not in _PAIRS:
        s = polarised_sets(n)[which]
        one, zero = tuple(s["near_one"]), tuple(s["near_zero"])
        seed = 1000 * n + 10 * which + PHASES.index(phases)
        f = polarised_state(n, SMALL[prec], one, zero, phases, seed, prec)
        b = polarised_state(n, SMALL[prec], one[1:], zero + one[:1], phases, seed + 5, prec)
        pair = tuple(np.ascontiguousarray(x.astype(DT[prec])) for x in (f, b))
        for x in pair:
            x.setflags(write=False)
        _PAIRS[key] = pair
    return _PAIRS[key]


def wide(state):
    """The complex128 image of a state in the widest complex type numpy has (x87 extended where
    long double is wider than double).  The oracle's einsums sum in their inputs' type, and a
    complex128 sum of 2^16 positive terms is itself 1e-13 off — a thousand f64 roundings — so the
    exact side of every elemrel is the same einsum of wide(state), rounded once to complex128."""
    return np.asarray(state).astype(np.complex128).astype(np.clongdouble)


def exact(fn, *args):
    """fn (an einsum restatement of oracle.oracle or a test's own) on the wide images of its
    array arguments, rounded to complex128."""
    return np.asarray(fn(*[wide(a) if isinstance(a, np.ndarray) else a for a in args])).astype(
        np.complex128)


# One row per kind of call: the einsum that defines it (fwd, bwd, positions), its element scale
# and the op-table method that computes it.  A test may add rows (the dense k-qubit calls of
# tests/test_gpu_polarised.py).
EXACT = {
    "q1dens": (lambda f, b, p: O.get_q1_density(f, *p), lambda f, b, p: density_scale(f, p)),
    "q2dens": (lambda f, b, p: O.get_q2_density(f, *p), lambda f, b, p: density_scale(f, p)),
    "q1grad": (lambda f, b, p: O.get_q1_grad(f, b, *p), grad_scale),
    "q2grad": (lambda f, b, p: O.get_q2_grad(f, b, *p), grad_scale),
    "q2diag": (lambda f, b, p: O.get_q2_grad_diag(f, b, *p), grad_diag_scale),
}
CALL = {
    "q1dens": lambda ops, f, b, p: ops.get_q1_density(f, *p),
    "q2dens": lambda ops, f, b, p: ops.get_q2_density(f, *p),
    "q1grad": lambda ops, f, b, p: ops.get_q1_grad(f, b, *p),
    "q2grad": lambda ops, f, b, p: ops.get_q2_grad(f, b, *p),
    "q2diag": lambda ops, f, b, p: ops.get_q2_grad_diag(f, b, *p),
}
KINDS = tuple(CALL)


def primitive_calls(q1, q2, kinds=KINDS):
    """[(kind, positions)]: every kind of `kinds` at the q1 positions and the q2 pairs (each
    call once, in order)."""
    calls = [(k, (int(p),)) for p in q1 for k in ("q1dens", "q1grad") if k in kinds] + \
        [(k, (int(p2), int(p1))) for p2, p1 in q2 for k in ("q2dens", "q2grad", "q2diag")
         if k in kinds]
    return list(dict.fromkeys(calls))


_TABLES = {}


def polarised_table(prec, n, which, phases, calls):
    """{(kind, positions): (exact value, element scale)} of `calls` on polarised_pair(prec, n,
    which, phases): computed once, shared by the floor and by every kernel variant."""
    tab = _TABLES.setdefault((prec, n, which, phases), {})
    missing = [c for c in calls if c not in tab]
    if missing:
        f64, b64 = (x.astype(np.complex128) for x in polarised_pair(prec, n, which, phases))
        fw, bw = wide(f64), wide(b64)
        for kind, pos in missing:
            fn, scale = EXACT[kind]
            tab[(kind, pos)] = (np.asarray(fn(fw, bw, list(pos))).astype(np.complex128).reshape(-1),
                                scale(f64, b64, list(pos)))
    return {c: tab[c] for c in calls}


def elemrels(ops, f, b, table):
    """[(kind, positions, elemrel)] of the op table `ops` (oracle.cref.CRefOps, or a test's table
    over device tensors) on the states f, b (whatever `ops` takes) for every call of `table`."""
    return [(kind, pos, elemrel(CALL[kind](ops, f, b, list(pos)), want, scale))
            for (kind, pos), (want, scale) in table.items()]


_PFLOORS = {}


def primitive_floors(prec, n, which, calls):
    """{kind: floor}: the worst elemrel of CRefOps(prec) over `calls` and both phase variants of
    one polarised case."""
    key = (prec, n, which, tuple(calls))
    if key not in _PFLOORS:
        ops = CRefOps(prec)
        worst = {}
        for phases in PHASES:
            f, b = polarised_pair(prec, n, which, phases)
            for kind, _, err in elemrels(ops, f, b, polarised_table(prec, n, which, phases, calls)):
                worst[kind] = max(worst.get(kind, 0.0), err)
        _PFLOORS[key] = worst
    return _PFLOORS[key]

"""Mirrored reverse sweeps (QDC_MIRROR) on the GPU against the oracle floors.

With QDC_MIRROR the forward is scheduled so that its fused passes, run in reverse, are the
backward's passes, and each backward stage uncomputes with exactly the adjoint of the stage
matrix the forward applied (qdc_circuit.hpp mirror_schedule / mirror_adjoint).  The uncompute then
drifts like the reference's gate-by-gate U, U^dagger pairs (src/circuit.rs:266-429) instead of
accumulating the rounding of independently formed forward and reverse stage products.
QDC_MIRROR=2 makes a backward that cannot mirror its forward an error, so these tests prove the
mirrored schedule ran.  Every output must stay within 4x the floor of the reference's own
algorithm (tests/floors.py); the uncomputed state is the output the mirror exists for.
"""
import numpy as np
import pytest

import floors as F
from oracle import oracle as O
from quantum_differentiable_circuit import workloads as W

pytestmark = pytest.mark.gpu


def build(prec, n, ins, **kw):
    import quantum_differentiable_circuit as q
    c = q.circuit_class(prec)(n, **kw)
    for kind, pos in ins:
        c._push(kind, *pos)
    return c


@pytest.fixture
def strict_mirror(monkeypatch):
    monkeypatch.setenv("QDC_MIRROR", "2")


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_mirror_c5_depth_10k_gates(strict_mirror, prec):
    n = 14
    ins, var = W.deep_random_circuit(n, 10000, seed=33)
    fl = F.Floor(prec, n, ins, [], var, run=False)
    c = build(prec, n, ins)
    what = f"mirror C5 n={n} 10k {prec} "
    fl.check("forward", c.forward([], fl.var), what)
    _check_states(fl, c, what, "state")
    fl.check("grads", c.backward(fl.cots, [], fl.var), what)
    _check_states(fl, c, what, "uncomputed", "bwd")


# The uncomputed state's max-norm error is the extreme of 2^n rounding random walks around
# |0..0>: one circuit's value depends on the realization, not only on the algorithm.  The
# reference's own gate-by-gate algorithm on C5 n = 14 (seed 33) gives max-norm 1.41e-7 in the C
# restatement (the floor) and 7.16e-7 with numpy's complex64 arithmetic — 5x apart — but 2-norm
# 6.17e-6 and 6.93e-6; the runtime's own program emulated on the host (tools/drift_trace.py,
# profiles/r6/r6_drift_trace_c5_n14.txt) spreads 0.3-2.2x in max-norm and 0.85-0.92x in 2-norm
# over 8 circuits and 1 / 2 / 8 shards.  So the 2-norm carries the claim (<= 2x the floor), and
# the max-norm of the uncomputed state is held to 2 RATIO (a localised error would exceed both).
UNCOMPUTED_MAX_RATIO = 2 * F.RATIO
L2_RATIO = 2.0


def _check_states(fl, c, what, *keys):
    """Max-norm floor lines and their 2-norm counterparts (the stable aggregate)."""
    for key in keys:
        st = c.get_state(2 if key == "bwd" else 0)
        fl.check(key, st, what, ratio=UNCOMPUTED_MAX_RATIO if key == "uncomputed" else F.RATIO)
        fl.check_l2(key, st, what, ratio=L2_RATIO)


@pytest.fixture(scope="module")
def c5_floors():
    """C5 at depth: one 10k-gate circuit at n = 14 and its floors per precision (shared by the
    sharded configurations below; each floor costs the reference's algorithm on the CPU)."""
    n = 14
    ins, var = W.deep_random_circuit(n, 10000, seed=33)
    return n, ins, {p: F.Floor(p, n, ins, [], var, run=False) for p in ("f32", "f64")}


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("kw", [{"local_shards": 2}, {"local_shards": 8}, {"devices": [0, 0]}],
                         ids=["2shards", "8shards", "2streams"])
def test_c5_depth_10k_gates_sharded(strict_mirror, c5_floors, prec, kw):
    """Config C5's depth on the sharded path (the path the 8-GPU config runs): the forward's
    remap plan keeps both directions' order relations and the backward undoes every remap in
    reverse (qdc_circuit.hpp remap, inverse), so each reverse pass uncomputes with the adjoint of the
    forward's stage matrix in the layout the forward applied it.  QDC_MIRROR=2: a sharded
    backward that did not mirror its forward is an error.  Every output within 4x the floor of
    the reference's own gate-by-gate algorithm (src/circuit.rs:280-392)."""
    n, ins, fls = c5_floors
    fl = fls[prec]
    c = build(prec, n, ins, **kw)
    phys, world, _, nloc = c.layout()
    assert world == nloc == len(kw.get("devices", [None])) * kw.get("local_shards", 1)
    what = f"mirror C5 n={n} 10k {prec} {kw} "
    fl.check("forward", c.forward([], fl.var), what)
    _check_states(fl, c, what, "state")
    assert c.layout()[0] != list(range(n)), "the forward must have remapped"
    fl.check("grads", c.backward(fl.cots, [], fl.var), what)
    assert c.layout()[0] == list(range(n)), "every remap undone"
    _check_states(fl, c, what, "uncomputed", "bwd")


def test_push_between_forward_and_backward():
    """A Diff density pushed after the forward runs in the backward (the mirrored record of the
    forward no longer covers the circuit: the backward schedules itself), as in the reference,
    whose backward walks every instruction from the forward's final state."""
    import quantum_differentiable_circuit as q
    n = 12
    ins, var = O.layered_circuit(n, layers=3, seed=8)
    dt = np.complex64
    c = build("f32", n, ins)
    o = O.OracleCircuit(n)
    for kind, pos in ins:
        o.add(kind, *pos)
    vg = [np.ascontiguousarray(g, dtype=dt) for g in var]
    v128 = [g.astype(np.complex128) for g in vg]
    d = c.forward([], vg)
    od = o.forward([], v128)
    c.get_q2_dens_op_with_grad(3, 7)
    o.add(O.DIFF_Q2_DENSITY, 3, 7)
    cots = F.sigma_z_cots(list(d) + [np.zeros((4, 4))], dt)
    cots[-1] = np.ascontiguousarray(np.arange(16).reshape(4, 4) / 16.0 + 0.5j, dtype=dt)
    g = np.concatenate(c.backward(cots, [], vg))
    want = np.concatenate(o.backward([x.astype(np.complex128) for x in cots], [], v128))
    assert F.normrel(g, want) < 1e-5, F.normrel(g, want)
    assert len(od) == len(d)
    del q


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_mirror_layered_c2(strict_mirror, prec):
    n = 12
    ins, var = O.layered_circuit(n, layers=4, seed=24)
    fl = F.Floor(prec, n, ins, [], var, run=False)
    c = build(prec, n, ins)
    what = f"mirror C2 n={n} {prec} "
    fl.check("forward", c.forward([], fl.var), what)
    fl.check("grads", c.backward(fl.cots, [], fl.var), what)
    fl.check("uncomputed", c.get_state(0), what)


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [12, 17])
def test_mirror_random_every_kind(strict_mirror, prec, n):
    """Every gate kind (NonU kinds uncompute with the inverse, not the mirrored adjoint),
    perturbed non-unitary variable gates (inexact ordering rules) and densities between the
    passes, from a random initial state, Tsallis cotangents."""
    ins, const, var = O.random_circuit(n, 160, seed=100 + n, density_every=40)
    rng = np.random.default_rng(n)
    var = [g + 1e-3 * (rng.standard_normal(g.shape) + 1j * rng.standard_normal(g.shape))
           for g in var]
    psi0 = O.random_state(np.random.default_rng(n), n)
    fl = F.Floor(prec, n, ins, const, var, psi0=psi0, cots=F.tsallis_cots, run=False)
    c = build(prec, n, ins)
    c.set_state_from_vector(fl.psi0)
    what = f"mirror random n={n} {prec} "
    fl.check("forward", c.forward(fl.const, fl.var), what)
    fl.check("grads", c.backward(fl.cots, fl.const, fl.var), what)
    fl.check("uncomputed", c.get_state(0), what)
    fl.check("bwd", c.get_state(2), what)


def test_mirror_needs_the_forwards_gates(strict_mirror):
    """A backward with gates other than its forward's cannot mirror it (QDC_MIRROR=2: error;
    QDC_MIRROR=1 schedules the backward itself)."""
    n = 12
    ins, var = O.layered_circuit(n, layers=2, seed=5)
    fl = F.Floor("f32", n, ins, [], var, run=False)
    c = build("f32", n, ins)
    c.forward([], fl.var)
    other = [(g * np.exp(0.1j)).astype(np.complex64) for g in fl.var]
    with pytest.raises(BaseException, match="mirror"):  # PanicException (as the reference's)
        c.backward(fl.cots, [], other)

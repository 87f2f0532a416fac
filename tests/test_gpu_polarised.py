"""Element-scale accuracy of every density and gradient kernel on polarised states.

The other GPU parity tests draw Haar-like states (every density diagonal near 2^-k) or measure
against the largest element of a group, so a kernel that forms a small output as the difference
of two large ones, or whose summation order swamps small terms, passes them.  Here the states
are near-product states with three qubits polarised to 1e-6 (f32) / 1e-12 (f64) — what a VQSE /
VQE / Tsallis loop converges to — and every output element is measured against its own
Cauchy-Schwarz scale (tests/floors.py: polarised_state, elemrel) and bounded by RATIO x the same
metric of the reference's algorithm in build precision (CRefOps) + ATOL.
tests/test_polarised_cpu.py shows that this bound discriminates.

The exact side of every comparison is the oracle's einsum of the complex128 image of the
build-precision inputs, summed in extended precision (floors.wide): summed in complex128 it is
itself 1e-13 off at n = 17, a thousand f64 roundings.

Measured on an MI355X, worst err / floor per kernel family (f32, f64): q1 density 1.2, 1.0; q2
density 0.9, 1.0; q1 gradient 1.2, 0.5; q2 gradient 1.3, 0.7; q2 diagonal gradient 2.0, 1.0;
k-qubit density 1.1, 1.7; k-qubit gradient 7.3, 5.5 (inside the bound by ATOL: 0.3 of it — the
gradients' floors are 1e-8 / 3e-17, far below one rounding); the LANE and tile families
(QDC_LANE=6, QDC_TILE_FAR=7) at most 2.4; fused runtime, every variant, 0.5-1.2.  Before k_dens1 summed rho00 directly, the default-knob q1 case stood at 1e4-2e5
(f32) and 1e10-1e11 (f64) floors."""
import itertools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import floors as F
from oracle import oracle as O
from test_gpu_dense_grad import POSITIONS, qk_density_ref, qk_grad_ref
from test_gpu_fusion import build, build_env
from test_gpu_primitives import q2_positions

pytestmark = pytest.mark.gpu
DT = F.DT

# the dense k-qubit calls as rows of the floors tables
F.EXACT.setdefault("qkdens", (lambda f, b, p: qk_density_ref(f, p), lambda f, b, p: F.density_scale(f, p)))
F.EXACT.setdefault("qkgrad", (lambda f, b, p: qk_grad_ref(f, b, p), F.grad_scale))
F.CALL.setdefault("qkdens", lambda ops, f, b, p: ops.get_qk_density(f, p))
F.CALL.setdefault("qkgrad", lambda ops, f, b, p: ops.get_qk_grad(f, b, p))


class GpuOps:
    """The primitives ABI over device tensors, as an op table."""

    @staticmethod
    def get_q1_density(f, pos):
        return f.get_q1_density(pos)

    @staticmethod
    def get_q2_density(f, pos2, pos1):
        return f.get_q2_density(pos2, pos1)

    @staticmethod
    def get_qk_density(f, positions):
        return f.get_qk_density(positions)

    @staticmethod
    def get_q1_grad(f, b, pos):
        import quantum_differentiable_circuit as q
        return q.get_q1_grad(f, b, pos)

    @staticmethod
    def get_q2_grad(f, b, pos2, pos1):
        import quantum_differentiable_circuit as q
        return q.get_q2_grad(f, b, pos2, pos1)

    @staticmethod
    def get_q2_grad_diag(f, b, pos2, pos1):
        import quantum_differentiable_circuit as q
        return q.get_q2_grad_diag(f, b, pos2, pos1)

    @staticmethod
    def get_qk_grad(f, b, positions):
        import quantum_differentiable_circuit as q
        return q.get_qk_grad(f, b, positions)


_TENSORS = {}


def tensors(prec, n, which, phases):
    """The device copies of floors.polarised_pair, shared and never modified."""
    import quantum_differentiable_circuit as q
    key = (prec, n, which, phases)
    if key not in _TENSORS:
        _TENSORS[key] = tuple(q.QuantizedTensor.new_from_host(x, prec)
                              for x in F.polarised_pair(prec, n, which, phases))
    return _TENSORS[key]


def q12_calls(n, which):
    """get_q1_density / get_q1_grad at every position; the q2 calls on the 27 pairs of
    test_gpu_primitives that exist at n and both orders of (polarised, polarised), (polarised,
    balanced) and (balanced, balanced)."""
    base = [p for p in q2_positions(np.random.default_rng(7)) if max(p) < n]
    return F.primitive_calls(range(n), base + F.structured_pairs(n, which))


def qk_lists(n, k, which):
    """test_gpu_dense_grad.POSITIONS[k] as far as it exists at n, and one list that holds all
    three polarised qubits (unsorted, filled up with balanced ones)."""
    p = F.polarised_qubits(n, which)
    return [list(pos) for pos in POSITIONS[k] if max(pos) < n] + \
        [[p[1], F.BALANCED[1], p[0], p[2], F.BALANCED[0]][:k] if k > 3 else [p[1], p[0], p[2]]]


def qk_calls(n, k, which):
    return [(kind, tuple(pos)) for pos in qk_lists(n, k, which) for kind in ("qkdens", "qkgrad")]


def gpu_elemrels(prec, n, which, calls):
    """[(kind, phases, positions, elemrel)] of the HIP kernels."""
    out = []
    for phases in F.PHASES:
        tf, tb = tensors(prec, n, which, phases)
        out += [(kind, phases, pos, err) for kind, pos, err in
                F.elemrels(GpuOps, tf, tb, F.polarised_table(prec, n, which, phases, calls))]
    return out


def check_records(prec, what, records, floors):
    """One [floor-elem] line and one bound per call; every failing call is reported."""
    bad = []
    worst = {}
    for kind, phases, pos, err in records:
        F.check_elem(prec, f"{what}{kind} {phases} {list(pos)}", err, floors[kind], failures=bad)
        worst[kind] = max(worst.get(kind, 0.0), err)
    for kind, err in worst.items():
        print(f"[floor-elem-worst] {what}{kind}: err {err:.3e}  floor {floors[kind]:.3e}  "
              f"ratio {err / floors[kind]:.2f}")
    assert not bad, f"{len(bad)} of {len(records)} calls above the bound: " + "; ".join(bad[:20])


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [12, 17])
@pytest.mark.parametrize("which", [0, 1])
def test_q1_q2_densities_and_gradients(prec, n, which):
    calls = q12_calls(n, which)
    check_records(prec, f"{prec} n={n} set {which} ", gpu_elemrels(prec, n, which, calls),
                  F.primitive_floors(prec, n, which, calls))


def knob_child_records(prec):
    """The q1 / q2 calls of every (n, set): what a child process under a Context-scope knob
    prints (the knob is read when the device context is created, qdc_device.hpp)."""
    return [(n, which, kind, phases, pos, err) for n in (12, 17) for which in (0, 1)
            for kind, phases, pos, err in gpu_elemrels(prec, n, which, q12_calls(n, which))]


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("knob", ["QDC_LANE=6", "QDC_TILE_FAR=7"])
def test_q1_q2_on_lane_and_tile_families(prec, knob):
    """QDC_LANE=6: densities and gradients on the LANE family; QDC_TILE_FAR=7: far-target
    densities and gradients on the tile family — their reducing variants, in a child process."""
    here = Path(__file__).resolve().parent
    code = (f"import sys, json; sys.path[:0] = [{str(here)!r}, {str(here.parent)!r}, "
            f"{str(here.parent / 'differentiable-quantum-circuit-cuda_amd')!r}]\n"
            "import test_gpu_polarised as t\n"
            f"print(json.dumps(t.knob_child_records({prec!r})))\n")
    name, value = knob.split("=")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{name: value}),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    records = json.loads(r.stdout.strip().splitlines()[-1])
    for n in (12, 17):
        for which in (0, 1):
            mine = [(kind, phases, tuple(pos), err) for n_, w_, kind, phases, pos, err in records
                    if (n_, w_) == (n, which)]
            assert len(mine) == 2 * len(q12_calls(n, which))
            check_records(prec, f"{knob} {prec} n={n} set {which} ", mine,
                          F.primitive_floors(prec, n, which, q12_calls(n, which)))


def qk_floors(prec, n, k, which):
    """No C restatement for k >= 3: the worst q2 floor over the qubit pairs drawn from the same
    position lists (a k-qubit element sums fewer terms of the same amplitudes than a q2 element)."""
    pairs = sorted({pr for pos in qk_lists(n, k, which) for pr in itertools.combinations(pos, 2)})
    fl = F.primitive_floors(prec, n, which, F.primitive_calls([], pairs, ("q2dens", "q2grad")))
    return {"qkdens": fl["q2dens"], "qkgrad": fl["q2grad"]}


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [12, 17])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_qk_densities_and_gradients(prec, n, k):
    for which in (0, 1):
        check_records(prec, f"{prec} n={n} k={k} set {which} ",
                      gpu_elemrels(prec, n, which, qk_calls(n, k, which)), qk_floors(prec, n, k, which))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_qk_grid_stride_loop(monkeypatch, prec):
    """Three blocks (QDC_QKG_GRID=3): every wave walks many tiles and sums them in its registers."""
    monkeypatch.setenv("QDC_QKG_GRID", "3")
    n, which = 17, 0
    for k in (3, 4, 5):
        check_records(prec, f"QDC_QKG_GRID=3 {prec} n={n} k={k} ",
                      gpu_elemrels(prec, n, which, qk_calls(n, k, which)), qk_floors(prec, n, k, which))


# ---------------------------------------------------------------------------------------
# The fused runtime
# ---------------------------------------------------------------------------------------
def circuit(n, final):
    """One brick layer of Haar VAR_Q2 gates on pairs of balanced qubits, VAR_Q2_DIAG gates with
    unit-modulus entries on pairs that touch polarised qubits (they keep the populations), then
    the densities: final="q1": DIFF_Q1_DENSITY on every qubit (at n = 16 exactly DENS1_MAX in one
    pass); "q2": DIFF_Q2_DENSITY on (polarised, polarised), (polarised, balanced) and (balanced,
    polarised) pairs."""
    p = F.polarised_qubits(n, 0)  # (0, n - 1, 5)
    rng = np.random.default_rng(40 + n)
    bal = [q for q in range(n) if q not in p]
    ins, var = [], []
    for a, b in zip(bal[0::2], bal[1::2]):
        ins.append((O.VAR_Q2, (b, a)))
        var.append(O.haar_unitary(rng, 4))
    for pr in ((p[0], bal[0]), (bal[-1], p[1]), (p[2], bal[3]), (p[0], p[1]), (p[1], p[2])):
        ins.append((O.VAR_Q2_DIAG, pr))
        var.append(np.exp(1j * rng.uniform(0, 2 * np.pi, 4)))
    if final == "q1":
        ins += [(O.DIFF_Q1_DENSITY, (q,)) for q in range(n)]
    else:
        ins += [(O.DIFF_Q2_DENSITY, pr) for pr in ((p[0], p[1]), (p[2], p[0]), (p[1], bal[2]),
                                                   (p[2], bal[-2]), (bal[1], p[0]), (bal[4], p[2]))]
    return ins, var


_CIRCUITS = {}


def circuit_case(prec, n, final, phases):
    """(instructions, Floor, exact densities, their scales, the CRefOps circuit's elemrel)."""
    key = (prec, n, final, phases)
    if key not in _CIRCUITS:
        ins, var = circuit(n, final)
        s = F.polarised_sets(n)[0]
        psi0 = F.polarised_state(n, F.SMALL[prec], s["near_one"], s["near_zero"], phases,
                                 7 * n + F.PHASES.index(phases), prec)
        fl = F.Floor(prec, n, ins, [], var, psi0=psi0, run=False)
        # every density is taken of the final state: the oracle's einsum of its wide image
        state = fl.exact["state"]
        dens = [F.exact(O.get_q1_density, state, *pos) if len(pos) == 1 else
                F.exact(O.get_q2_density, state, *pos) for kind, pos in ins
                if kind in (O.DIFF_Q1_DENSITY, O.DIFF_Q2_DENSITY)]
        scales = [F.density_scale_of(d.reshape(2 if d.size == 4 else 4, -1)) for d in dens]
        floor = max(F.elemrel(r, d, s_) for r, d, s_ in zip(fl.ref["forward"], dens, scales))
        _CIRCUITS[key] = (ins, fl, dens, scales, floor)
    return _CIRCUITS[key]


VARIANTS = {
    "default": {},
    "dens1=0": {"QDC_DENS1": 0},
    "dens1=0,split=0": {"QDC_DENS1": 0, "QDC_DENS_SPLIT": 0},
    "fuse_meas=0": {"QDC_FUSE_MEAS": 0},
    "fuse=0": {"QDC_FUSE": 0},
    "rq=0": {"QDC_RQ": 0},
    "spec=2": {"QDC_SPEC": 2, "QDC_SPEC_MAX": 400},
    "shards=2": None,
}


@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("n", [13, 16])
@pytest.mark.parametrize("final", ["q1", "q2"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_runtime_densities(prec, n, final, variant):
    """forward's densities element by element, under every schedule that can produce them; then
    backward (sigma-z cotangents): the polarised input does not break the reverse sweep."""
    import quantum_differentiable_circuit as q
    floor = max(circuit_case(prec, n, final, ph)[4] for ph in F.PHASES)
    bad = []
    for phases in F.PHASES:
        ins, fl, dens, scales, _ = circuit_case(prec, n, final, phases)
        env = VARIANTS[variant]
        c = build(prec, n, ins, 1, local_shards=2) if env is None else build_env(prec, n, ins, env)
        c.set_state_from_vector(fl.psi0)
        c.profile(True)
        launched = q.jit_stats(prec)["launched"]
        got = c.forward([], fl.var)
        stats = c.profile_collect()
        what = f"{variant} {prec} n={n} {final} {phases} "
        for (kind, pos), g, d, s in zip(ins[-len(dens):], got, dens, scales):
            F.check_elem(prec, f"{what}density {list(pos)}", F.elemrel(g, d, s), floor, failures=bad)
        if variant == "default" and final == "q1":
            assert stats["fused_density"]["launches"] >= 1, sorted(stats)
        grads = c.backward(fl.cots, [], fl.var)
        c.synchronize()
        if variant == "spec=2":  # (a failed compile would fall back to the interpreted kernels)
            assert q.jit_stats(prec)["launched"] > launched, q.jit_stats(prec)
        fl.check("grads", grads, what)
        fl.check("uncomputed", c.get_state(0), what)
    assert not bad, f"{len(bad)} densities above the bound: " + "; ".join(bad[:20])

"""The runtime's program trace (qdc_trace_program, host only): every matrix a forward call then a
backward call apply to the forward state, from the runtime's own dry run — the plan, remaps,
permuting passes, fusion into stages and the mirrored reverse sweep — mapped to logical qubits.

Replayed in complex128 on the f64 build's trace, the forward must give the oracle's final state
(src/circuit.rs:164-262) and the backward must undo it (circuit.rs:266-429 uncomputes with U^-1
per gate), on 1, 2 and 8 shards.  This pins the input of the host drift emulator
(tools/drift_trace.py) to what the GPU kernels are given."""
import functools

import numpy as np
import pytest

import floors
from oracle import oracle as O
from quantum_differentiable_circuit import workloads as W


def _apply(psi, u, qs, n):
    k = len(qs)
    t = psi.reshape((2,) * n)
    ax = [n - 1 - p for p in qs]
    t = np.moveaxis(t, ax, list(range(k))).reshape(1 << k, -1)
    t = u @ t
    return np.moveaxis(t.reshape((2,) * n), list(range(k)), ax).reshape(-1)


def _replay(tr, n, psi, direction):
    for op in tr[tr["dir"] == direction]:
        R = int(op["R"])
        u = np.asarray(op["m"][:R * R], np.complex128).reshape(R, R)
        psi = _apply(psi, u, [int(op["q2"])] if R == 2 else [int(op["q2"]), int(op["q1"])], n)
    return psi


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("circuit", ["deep", "every_kind"])
def test_trace_replays_forward_and_uncompute(world, circuit):
    import quantum_differentiable_circuit as q
    n = 11
    if circuit == "deep":
        ins, var = W.deep_random_circuit(n, 600, seed=4)
        const = []
    else:
        ins, const, var = O.random_circuit(n, 300, seed=9, density_every=50)
    instr = [(k, *p) for k, p in ins]
    cg = [np.ascontiguousarray(g, dtype=np.complex128) for g in const]
    vg = [np.ascontiguousarray(g, dtype=np.complex128) for g in var]
    o = O.OracleCircuit(n, np.complex128)
    for kind, pos in ins:
        o.add(kind, *pos)
    dens = o.forward(cg, vg)
    cots = [np.ascontiguousarray(np.eye(d.shape[0]), dtype=np.complex128) for d in dens]
    tr = q.trace_program(n, instr, cg, vg, cots, world=world, precision="f64")
    fw, bw = tr[tr["dir"] == 0], tr[tr["dir"] == 1]
    assert len(fw) > 0 and len(bw) == len(fw)
    psi0 = np.zeros(1 << n, np.complex128)
    psi0[0] = 1
    psi = _replay(tr, n, psi0, 0)
    assert np.abs(psi - o.state).max() < 1e-12
    back = _replay(tr, n, psi, 1)
    assert np.abs(back - psi0).max() < 1e-10
    # the mirrored sweep: every reverse stage of unitary gates is the adjoint of the forward's
    # recorded matrix (non-unitary stages keep their exact inverse)
    fused = bw[bw["single"] == 0]
    if circuit == "deep":
        assert fused["mirrored"].all()
    elif len(fused):  # (8 shards of 11 qubits leave 8 local ones: no fused tile, single gates)
        assert fused["mirrored"].sum() > 0


# --- single gates and fused stages take their matrices from one rule (qdc_device.hpp GateMats) ---
N_KINDS = 11
# the runtime's unitarity criterion (qdc_circuit.hpp mark_inexact): max |U^+ U - I| in f64
UTOL = {"f32": 1e-6, "f64": 1e-13}
# |U^-1 U - I| of a non-unitary gate.  f32: the inverse is formed in long double and rounded once
# to f32, each entry by at most 2^-24 of its size; the gates are Haar unitaries plus 0.05 N(0,1)
# per entry (entries of U and U^-1 below 1.5), so an entry of (fl(U^-1) - U^-1) U is at most
# 4 x 2^-24 x 1.5 x 1.5 = 5.4e-7
INV_TOL = {"f32": 5.4e-7, "f64": 1e-10}


@functools.lru_cache(maxsize=None)
def _every_kind(prec):
    """The every_kind circuit with its gates rounded to the build's precision, and the floor
    object of that circuit (exact complex128 results, sigma-z cotangents), computed once."""
    ins, const, var = O.random_circuit(N_KINDS, 300, seed=9, density_every=50)
    return ins, floors.Floor(prec, N_KINDS, ins, const, var, run=False)


def _trace(prec, world):
    import quantum_differentiable_circuit as q
    ins, F = _every_kind(prec)
    return q.trace_program(N_KINDS, [(k, *p) for k, p in ins], F.const, F.var, F.cots, world=world,
                           precision=prec)


def _replay_both_ways(tr):
    psi0 = np.zeros(1 << N_KINDS, np.complex128)
    psi0[0] = 1
    psi = _replay(tr, N_KINDS, psi0, 0)
    return psi0, psi, _replay(tr, N_KINDS, psi, 1)


def _check_adjoint_pairs(tr, prec, exact_reverse):
    """QDC_FUSE=0: the backward's single gates are the forward's in reverse (exact_reverse), or,
    on a sharded circuit whose remap planner may exchange gates on disjoint qubits, in reverse
    among the gates on the same qubits (which it cannot exchange).  A unitary gate is uncomputed
    with exactly the forward matrix's adjoint, a non-unitary one with its inverse."""
    fw, bw = tr[tr["dir"] == 0], tr[tr["dir"] == 1]
    assert len(fw) > 0 and len(bw) == len(fw)
    assert (tr["single"] == 1).all()
    key = lambda op: (int(op["R"]), int(op["q2"]), int(op["q1"]))
    if exact_reverse:
        assert [key(b) for b in bw[::-1]] == [key(f) for f in fw]
    undo = {}
    for b in bw:
        undo.setdefault(key(b), []).append(b)
    seen = {"unitary": 0, "inverse": 0}
    for f in fw:
        R = int(f["R"])
        assert undo.get(key(f)), f"no uncompute of the forward gate on {key(f)}"
        b = undo[key(f)].pop()  # the last forward gate on these qubits is undone first
        u = np.asarray(f["m"][:R * R]).reshape(R, R)
        v = np.asarray(b["m"][:R * R]).reshape(R, R)
        u64 = u.astype(np.complex128)
        if np.abs(u64.conj().T @ u64 - np.eye(R)).max() <= UTOL[prec]:
            assert np.array_equal(v, u.conj().T)
            seen["unitary"] += 1
        else:
            assert np.abs(v.astype(np.complex128) @ u64 - np.eye(R)).max() < INV_TOL[prec]
            seen["inverse"] += 1
    print(f"[adjoint pairs] {prec}: {seen}")
    assert seen["unitary"] > 0 and seen["inverse"] > 0  # (seed 9 has gates of both classes)


@pytest.mark.parametrize("fuse", ["0", None])
def test_single_and_fused_paths_report_the_same_algebra(monkeypatch, fuse):
    if fuse is not None:
        monkeypatch.setenv("QDC_FUSE", fuse)
    _, F = _every_kind("f64")
    tr = _trace("f64", 1)
    assert ((tr["single"] == 1).all()) == (fuse == "0")
    psi0, psi, back = _replay_both_ways(tr)
    assert np.abs(psi - F.exact["state"]).max() < 1e-12
    assert np.abs(back - psi0).max() < 1e-10


def test_single_gate_uncompute_is_the_forward_adjoint(monkeypatch):
    monkeypatch.setenv("QDC_FUSE", "0")
    _check_adjoint_pairs(_trace("f64", 1), "f64", exact_reverse=True)


@pytest.mark.parametrize("fuse", ["0", None])
def test_f32_two_shards_report_the_same_algebra(monkeypatch, fuse):
    """The f32 build on 2 shards (remaps, f32 rounding of the shared helper's matrices), replayed
    in complex128 against the complex128 oracle, within the f32 floor of this circuit
    (tests/floors.py: RATIO x the reference algorithm's own f32 error, plus one rounding).
    (A shard's 10 local qubits hold no fused f32 tile: both settings trace single gates here.)"""
    if fuse is not None:
        monkeypatch.setenv("QDC_FUSE", fuse)
    _, F = _every_kind("f32")
    tr = _trace("f32", 2)
    if fuse == "0":
        assert (tr["single"] == 1).all()
    _, psi, back = _replay_both_ways(tr)
    F.check("state", psi, what=f"f32 world 2 fuse {fuse}: ")
    F.check("uncomputed", back, what=f"f32 world 2 fuse {fuse}: ")


def test_f32_two_shards_single_gate_uncompute_is_the_forward_adjoint(monkeypatch):
    monkeypatch.setenv("QDC_FUSE", "0")
    _check_adjoint_pairs(_trace("f32", 2), "f32", exact_reverse=False)

"""Passes on searched qubit sets (QDC_FUSE_SEARCH, qdc_fusion.hpp search_pass) on the GPU.

The search changes which gates share a pass and how a pass splits into stages, never what is
computed: every output stays within the floors of the reference's own algorithm
(tests/floors.py; max-norm RATIO as test_gpu_fusion.py / test_gpu_mirror.py, 2-norm 2x), and
the searched and the scanned schedule agree with each other to 2x the floor in the 2-norm.
Circuit knobs are read when a circuit is created, so each run builds its circuit under the
environment it tests.
"""
from functools import lru_cache

import numpy as np
import pytest

import floors as F
from oracle import oracle as O
from quantum_differentiable_circuit import workloads as W
from test_fusion_schedule import make

pytestmark = pytest.mark.gpu

# as tests/test_gpu_mirror.py: the 2-norm carries the claim, the max-norm of the uncomputed state
# (the extreme of 2^n rounding random walks) is held to twice RATIO
L2_RATIO = 2.0
UNCOMPUTED_MAX_RATIO = 2 * F.RATIO

LAYERS = 12
VAR_KINDS = (W.VAR_Q2, W.VAR_Q2_NONU, W.VAR_Q2_DIAG, W.VAR_Q1, W.VAR_Q1_NONU)
KEYS = ("forward", "state", "grads", "uncomputed", "bwd")


@lru_cache(maxsize=None)
def brickwork(prec, n):
    """12 layers of one-qubit gates on every qubit and two-qubit gates on even then odd pairs
    (C2's generator), and its floors."""
    ins, var = W.layered_circuit(n, LAYERS, seed=24)
    return ins, F.Floor(prec, n, ins, [], var, run=False)


def run(prec, n, ins, fl, **kw):
    import quantum_differentiable_circuit as q
    c = q.circuit_class(prec)(n, **kw)
    for kind, pos in ins:
        c._push(kind, *pos)
    if fl.psi0 is not None:
        c.set_state_from_vector(fl.psi0)
    out = {"forward": F.flat(c.forward(fl.const, fl.var)), "state": c.get_state(0)}
    out["grads"] = F.flat(c.backward(fl.cots, fl.const, fl.var))
    out["uncomputed"], out["bwd"] = c.get_state(0), c.get_state(2)
    return out


def max_gamma_stages(monkeypatch, prec, n, ins):
    """The deepest pass of the host-only mirrored forward schedule on the runtime's settings."""
    import quantum_differentiable_circuit as q
    with monkeypatch.context() as m:
        m.setenv("QDC_SCHED_RQ", "1")
        m.setenv("QDC_SCHED_MIRROR", "1")
        if prec == "f64":
            m.setenv("QDC_SCHED_PERM", "0")
        ops, items = q.fusion_schedule(n, [(k, *p) for k, p in ins], 1, precision=prec)
    return max(sum(any(ins[ops[i]["instr"]][0] in VAR_KINDS for i in st) for st in it["stages"])
               for it in items if it["type"] == 2)


@pytest.mark.parametrize("prec,n", [("f32", 12), ("f32", 14), ("f64", 11), ("f64", 13)])
def test_brickwork_searched_and_scanned(monkeypatch, prec, n):
    """The smallest sizes with full two-state tiles and one above each, deep enough for a pass at
    the Gamma cap."""
    ins, fl = brickwork(prec, n)
    monkeypatch.setenv("QDC_MIRROR", "2")
    got = {}
    for search in ("1", "0"):
        monkeypatch.setenv("QDC_FUSE_SEARCH", search)
        deepest = max_gamma_stages(monkeypatch, prec, n, ins)
        print(f"[sched] brickwork n={n} {prec} search={search}: deepest pass {deepest} Gamma stages")
        assert deepest >= 15
        got[search] = out = run(prec, n, ins, fl)
        what = f"brickwork n={n} {prec} search={search} "
        for key in ("forward", "grads", "uncomputed"):
            fl.check(key, out[key], what,
                     ratio=UNCOMPUTED_MAX_RATIO if key == "uncomputed" else F.RATIO)
            fl.check_l2(key, out[key], what, ratio=L2_RATIO)
    for key in ("forward", "grads", "uncomputed"):
        d = F.l2rel(got["1"][key], got["0"][key])
        bound = L2_RATIO * fl.floor_l2[key] + 2 * F.ATOL[prec]
        print(f"[floor-l2] brickwork n={n} {prec} {key} searched vs scanned: diff {d:.3e}  "
              f"floor {fl.floor_l2[key]:.3e}  bound {bound:.3e}")
        assert d <= bound, f"{key}: searched and scanned schedules differ by {d:.3e} > {bound:.3e}"


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_random_every_kind_with_densities(monkeypatch, prec):
    """Every gate kind, constant and variable, perturbed non-unitary matrices, densities and
    differentiable densities between the gates (the order classes), from a random state."""
    n = 14
    monkeypatch.setenv("QDC_FUSE_SEARCH", "1")
    ins, const, var, _, _ = make(n, 1, 1e-3)
    assert any(k == O.Q1_DENSITY for k, _ in ins[:40])
    assert any(k in (O.DIFF_Q1_DENSITY, O.DIFF_Q2_DENSITY) for k, _ in ins[:40])
    psi0 = O.random_state(np.random.default_rng(n), n)
    fl = F.Floor(prec, n, ins, const, var, psi0=psi0, cots=F.tsallis_cots, run=False)
    out = run(prec, n, ins, fl)
    what = f"random n={n} {prec} searched "
    for key in ("forward", "grads", "uncomputed", "bwd"):
        fl.check(key, out[key], what)


@pytest.mark.parametrize("shards", [2, 8])
def test_sharded_mirrored(monkeypatch, shards):
    """Searched passes across remaps (relabel_remap) under QDC_MIRROR=2: a sharded backward that
    did not mirror its forward is an error."""
    n, prec = 14, "f32"
    ins, fl = brickwork(prec, n)
    monkeypatch.setenv("QDC_FUSE_SEARCH", "1")
    monkeypatch.setenv("QDC_MIRROR", "2")
    a = run(prec, n, ins, fl)
    b = run(prec, n, ins, fl, local_shards=shards)
    for key in ("forward", "grads"):
        fl.check(key, b[key], f"brickwork n={n} {shards} shards searched ")
        F.check_pair(prec, b[key], a[key], fl.floor[key],
                     f"brickwork n={n} {shards} shards vs unsharded {key}")


def test_specialized_bit_identical(monkeypatch):
    """The specialized kernels of the searched brickwork program against the generic ones."""
    import quantum_differentiable_circuit as q
    n, prec = 14, "f32"
    ins, fl = brickwork(prec, n)
    monkeypatch.setenv("QDC_FUSE_SEARCH", "1")
    monkeypatch.setenv("QDC_MIRROR", "2")
    monkeypatch.setenv("QDC_SPEC_ASYNC", "0")
    monkeypatch.setenv("QDC_SPEC", "0")
    gen = run(prec, n, ins, fl)
    monkeypatch.setenv("QDC_SPEC", "2")
    monkeypatch.setenv("QDC_SPEC_MAX", "100000")
    s0 = q.jit_stats(prec)
    spec = run(prec, n, ins, fl)
    s1 = q.jit_stats(prec)
    launched = int(s1["launched"] - s0["launched"])
    print(f"[jit] brickwork n={n} searched: {launched} specialized launches, "
          f"{int(s1['compiled'] - s0['compiled'])} kernels compiled in the test")
    assert s1["enabled"] and launched > 0, s1
    for key in KEYS:
        assert np.array_equal(gen[key], spec[key]), f"specialized {key} differs from generic"

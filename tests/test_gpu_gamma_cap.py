"""Reverse passes of more than 16 Gamma stages (QDC_RQ_GCAP; storage bound FMAX_GRAD_RQ = 32)
on the GPU.

A fuller pass changes which stages share an HBM pass, never what is computed: at cap 32 every
output stays within the floors of the reference's own algorithm (tests/floors.py; the
uncomputed state as tests/test_gpu_fusion_search.py holds it), and the runs at cap 32 and at
cap 16 agree within those floors.  Interpreted (QDC_SPEC=0: the generic kernels with 32
accumulators) and specialized (QDC_SPEC=2: the generated kernels with 32).  f32 only: the f64
default stays at 16.  Circuit knobs are read when a circuit is created, so each run builds its
circuit under the environment it tests.
"""
import re
from functools import lru_cache

import numpy as np
import pytest

import floors as F
from quantum_differentiable_circuit import workloads as W

pytestmark = pytest.mark.gpu

PREC = "f32"
LAYERS = 8
L2_RATIO = 2.0                      # as tests/test_gpu_fusion_search.py
UNCOMPUTED_MAX_RATIO = 2 * F.RATIO  # (the max-norm of 2^n rounding random walks)
VAR_KINDS = (W.VAR_Q2, W.VAR_Q2_NONU, W.VAR_Q2_DIAG, W.VAR_Q1, W.VAR_Q1_NONU)
CAP = {32: {"QDC_RQ_GCAP": "32", "QDC_FUSE_MAX_OPS": "64"},
       16: {"QDC_RQ_GCAP": "16", "QDC_FUSE_MAX_OPS": "32"}}


@lru_cache(maxsize=None)
def layered(n):
    """C2's generator, 8 layers, and its floors (computed once, never modified)."""
    ins, var = W.layered_circuit(n, LAYERS, seed=24)
    return ins, F.Floor(PREC, n, ins, [], var, run=False)


def run(monkeypatch, n, ins, fl, env):
    import quantum_differentiable_circuit as q
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        c = q.circuit_class(PREC)(n)
    for kind, pos in ins:
        c._push(kind, *pos)
    out = {"forward": F.flat(c.forward(fl.const, fl.var))}
    out["grads"] = F.flat(c.backward(fl.cots, fl.const, fl.var))
    out["uncomputed"] = c.get_state(0)
    return out


def deepest_pass(monkeypatch, n, ins, cap):
    """Gamma stages of the deepest pass of the host-only mirrored forward schedule at `cap`."""
    import quantum_differentiable_circuit as q
    with monkeypatch.context() as m:
        m.setenv("QDC_SCHED_RQ", "1")
        m.setenv("QDC_SCHED_MIRROR", "1")
        m.setenv("QDC_SCHED_GCAP", str(cap))
        ops, items = q.fusion_schedule(n, [(k, *p) for k, p in ins], 1, precision=PREC,
                                       max_ops=2 * cap)
    return max(sum(any(ins[ops[i]["instr"]][0] in VAR_KINDS for i in st) for st in it["stages"])
               for it in items if it["type"] == 2)


@pytest.mark.parametrize("spec", ["0", "2"])
@pytest.mark.parametrize("n", [14, 16])
def test_cap_32_within_floors_and_of_cap_16(monkeypatch, capfd, n, spec):
    """n = 14, 16: the 11-bit two-state tile holds most of the register, so passes run to the cap."""
    import quantum_differentiable_circuit as q
    ins, fl = layered(n)
    assert deepest_pass(monkeypatch, n, ins, 32) > 16 >= deepest_pass(monkeypatch, n, ins, 16)
    base = {"QDC_MIRROR": "2", "QDC_SPEC": spec, "QDC_SPEC_ASYNC": "0", "QDC_SPEC_MAX": "100000",
            "QDC_RQ_STATS": "1"}
    got = {}
    for cap in (32, 16):
        capfd.readouterr()
        s0 = q.jit_stats(PREC)
        got[cap] = run(monkeypatch, n, ins, fl, {**base, **CAP[cap]})
        s1 = q.jit_stats(PREC)
        stages = [int(x) for x in re.findall(r"rq pass: (\d+) stages", capfd.readouterr().err)]
        launched = int(s1["launched"] - s0["launched"])
        print(f"[rq] n={n} spec={spec} cap={cap}: {len(stages)} register-resident passes, deepest "
              f"{max(stages)} stages, {launched} specialized launches")
        # (every stage of this circuit holds a variable gate: stages are Gamma stages)
        assert (max(stages) > 16) == (cap == 32) and max(stages) <= cap
        if spec == "2":
            assert s1["enabled"] and launched > 0, s1
        else:
            assert launched == 0
    what = f"layered n={n} spec={spec} cap 32 "
    for key in ("forward", "grads", "uncomputed"):
        fl.check(key, got[32][key], what,
                 ratio=UNCOMPUTED_MAX_RATIO if key == "uncomputed" else F.RATIO)
        fl.check_l2(key, got[32][key], what, ratio=L2_RATIO)
    for key in ("forward", "grads"):
        F.check_pair(PREC, got[32][key], got[16][key], fl.floor[key],
                     f"layered n={n} spec={spec} cap 32 vs cap 16 {key}")
    d = F.l2rel(got[32]["uncomputed"], got[16]["uncomputed"])
    bound = L2_RATIO * fl.floor_l2["uncomputed"] + 2 * F.ATOL[PREC]
    print(f"[floor-l2] layered n={n} spec={spec} uncomputed cap 32 vs cap 16: diff {d:.3e}  "
          f"bound {bound:.3e}")
    assert d <= bound


def test_deep_passes_are_deterministic(monkeypatch, capfd):
    """n = 22: passes of more than 16 Gamma slots write and finalize one partial per block and
    slot (32 slots pending at once) and, where the launch takes a dynamic tail, one per granule.
    Two identical calls, and two circuits, give bit-identical densities and gradients — with the
    default grid, and with a grid of 256 blocks, where the 2048 tiles of a pass are at least
    four per block and the tail is on."""
    import quantum_differentiable_circuit as q
    n = 22
    ins, var = W.layered_circuit(n, LAYERS, seed=5)
    vg = [np.ascontiguousarray(g, dtype=F.DT[PREC]) for g in var]
    cots = F.sigma_z_cots([np.zeros((2, 2))] * n, F.DT[PREC])

    def once(env):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            c = q.circuit_class(PREC)(n)
        for kind, pos in ins:
            c._push(kind, *pos)
        d = F.flat(c.forward([], vg))
        g = F.flat(c.backward(cots, [], vg))
        d2 = F.flat(c.forward([], vg))
        g2 = F.flat(c.backward(cots, [], vg))
        assert np.array_equal(d, d2) and np.array_equal(g, g2), f"repeat calls differ ({env})"
        return d, g

    capfd.readouterr()
    d1, g1 = once({"QDC_RQ_STATS": "1"})
    stages = [int(x) for x in re.findall(r"rq pass: (\d+) stages", capfd.readouterr().err)]
    assert max(stages) > 16, stages
    d2, g2 = once({})
    assert np.array_equal(d1, d2) and np.array_equal(g1, g2), "two circuits differ"
    d3, g3 = once({"QDC_FUSED_BLOCKS": "256"})
    d4, g4 = once({"QDC_FUSED_BLOCKS": "256"})
    assert np.array_equal(d3, d4) and np.array_equal(g3, g4), "two circuits differ (dynamic tail)"
    print(f"[dyn] n={n}: deepest pass {max(stages)} stages; 256-block grid vs default, grads "
          f"{F.normrel(g3, g1):.2e}")
    assert F.normrel(g3, g1) <= 1e-5 and F.normrel(d3, d1) <= 1e-5

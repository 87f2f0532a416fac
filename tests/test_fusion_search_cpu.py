"""The fused-pass scheduler's search for each pass's qubit set (QDC_FUSE_SEARCH), on CPU.

The search only chooses the set of physical positions a pass may use; the pass itself is still
built by the first-fit scan, which enforces every ordering rule (qdc_fusion.hpp scan_pass).  So:

1. QDC_FUSE_SEARCH=0 is the scan of the commit before the search, item for item
   (tests/golden/fusion_search_parent.json: one SHA-256 per schedule, recorded from that commit
   by `python tests/test_fusion_search_cpu.py --record`).
2. With the search on, the invariants of tests/test_fusion_schedule.py hold on the same grid,
   mirrored forwards reverse into valid backward sweeps within 16 Gamma stages, and the
   scheduled order replayed with the oracle's primitives equals the sequential oracle.
3. The passes it saves on the runtime's f32 settings (mirrored forward), and what it costs to
   schedule.
"""
import hashlib
import json
import os
import sys
import time
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_fusion_schedule import (CONST, DENS, DIAG, Q1, Q2, T, check_invariants, make,  # noqa: E402
                                  mirrored, replay, schedule)

from oracle import oracle as O  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "fusion_search_parent.json"
VAR_KINDS = set(Q1 + Q2 + DIAG) - set(CONST)
ENV = ("QDC_FUSE_SEARCH", "QDC_SCHED_RQ", "QDC_SCHED_MIRROR")


@lru_cache(maxsize=None)
def circuit(name):
    """(n, ins, sens) of the grid's circuits."""
    from quantum_differentiable_circuit import workloads as W
    if name == "c2":
        ins, _ = W.layered_circuit(28, 20, 24)
    elif name == "c4":
        ins, _ = W.brickwall_circuit(30, 40, 30)
    elif name == "c5_26":
        ins, _ = W.deep_random_circuit(26, 2000, seed=33)
    elif name == "c5_33":
        ins, _ = W.deep_random_circuit(33, 10000, seed=33)
    else:  # "make_<n>_<seed>": tests/test_fusion_schedule.py make(), perturbed for even seeds
        _, n, seed = name.split("_")
        ins, _, _, _, sens = make(int(n), int(seed), 1e-3 if int(seed) % 2 == 0 else 0.0)
        return int(n), ins, sens
    n = 1 + max(max(p) for _, p in ins)
    return n, ins, [0] * len(ins)


CIRCUITS = ("c2", "c4", "c5_26", "make_12_11", "make_14_1", "make_17_2", "make_24_3")
GRID = [(c, mode, rq, mir) for c in CIRCUITS for mode in (0, 1, 2) for rq in ("0", "1")
        for mir in ("0", "1")]


def run(name, mode, rq, mir, search, prec="f32"):
    """One schedule under the hook's knobs (restored afterwards)."""
    n, ins, sens = circuit(name)
    old = {k: os.environ.get(k) for k in ENV}
    os.environ.update(QDC_FUSE_SEARCH=search, QDC_SCHED_RQ=rq, QDC_SCHED_MIRROR=mir)
    try:
        ops, items = schedule(n, ins, mode, sens, prec)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return n, ins, sens, ops, items


def digest(items):
    canon = [[it["type"], it["lc"], it["h"], it["hb"], it["stages"]] for it in items]
    return hashlib.sha256(json.dumps(canon, separators=(",", ":")).encode()).hexdigest()


def gate_passes(ins, ops, items):
    """(fused passes holding a gate, their gate stages)."""
    passes = stages = 0
    for it in items:
        if it["type"] != 2:
            continue
        gst = sum(1 for s in it["stages"] if ins[ops[s[0]]["instr"]][0] not in DENS)
        passes += 1 if gst else 0
        stages += gst
    return passes, stages


def case_id(c, mode, rq, mir, prec="f32"):
    return f"{c}-mode{mode}-rq{rq}-mirror{mir}-{prec}"


def precisions(c):
    return ("f32", "f64") if c.startswith("make") else ("f32",)


@pytest.mark.parametrize("c,mode,rq,mir", GRID)
def test_search_off_is_the_parent_scan(c, mode, rq, mir):
    golden = json.loads(GOLDEN.read_text())
    for prec in precisions(c):
        _, ins, _, ops, items = run(c, mode, rq, mir, "0", prec)
        want = golden[case_id(c, mode, rq, mir, prec)]
        assert [len(items), *gate_passes(ins, ops, items)] == want["counts"]
        assert digest(items) == want["sha256"]


def gamma_stages(ins, ops, it):
    return sum(any(ins[ops[i]["instr"]][0] in VAR_KINDS for i in st) for st in it["stages"])


@pytest.mark.parametrize("c,mode,rq,mir", GRID)
def test_search_keeps_the_invariants(c, mode, rq, mir):
    for prec in precisions(c):
        n, ins, sens, ops, items = run(c, mode, rq, mir, "1", prec)
        two = mode == 2 or mir == "1"
        tbits = T[2] if two else None
        check_invariants(n, ins, sens, mode, prec, ops, items, permuted=rq == "1", tbits=tbits)
        if mir == "1" and mode == 1:
            ops_b, items_b = mirrored(ops, items, ins)
            check_invariants(n, ins, sens, 2, prec, ops_b, items_b, permuted=rq == "1",
                             tbits=T[2])
            for it in items:
                if it["type"] != 2:
                    continue
                meas = [ins[ops[st[0]]["instr"]][0] in DENS for st in it["stages"]]
                assert meas == sorted(meas)  # gate stages, then densities
        if (two and rq == "1") or (mir == "1" and mode == 1):
            assert all(gamma_stages(ins, ops, it) <= 16 for it in items if it["type"] == 2)


@pytest.mark.parametrize("mirror", ["0", "1"])
@pytest.mark.parametrize("sched_rq", ["0", "1"])
@pytest.mark.parametrize("perturb", [0.0, 1e-3])
def test_search_replay_matches_sequential_oracle(monkeypatch, perturb, sched_rq, mirror):
    """test_fusion_schedule's replay construction at n = 12 with the search on."""
    monkeypatch.setenv("QDC_FUSE_SEARCH", "1")
    monkeypatch.setenv("QDC_SCHED_RQ", sched_rq)
    monkeypatch.setenv("QDC_SCHED_MIRROR", mirror)
    n = 12
    ins, const, var, gates, sens = make(n, 11, perturb)
    ops, items = {}, {}
    ops["fwd"], items["fwd"] = schedule(n, ins, 1, sens, "f32")
    if mirror == "1":
        ops["bwd"], items["bwd"] = mirrored(ops["fwd"], items["fwd"], ins)
    else:
        ops["bwd"], items["bwd"] = schedule(n, ins, 2, sens, "f32")
    assert sum(it["type"] == 2 for it in items["fwd"]) > 3
    assert sum(it["type"] == 2 for it in items["bwd"]) > 3
    psi0 = O.random_state(np.random.default_rng(4), n)
    o = O.OracleCircuit(n)
    for k, p in ins:
        o.add(k, *p)
    o.set_state_from_vector(psi0)
    want_d = o.forward(const, var)

    def cot_fn(d):
        return [c.conj() for c in O.tsallis_loss_and_cotangents(d)[1]]

    want_g = o.backward(cot_fn(want_d), const, var)
    got_d, got_g, final = replay(n, ins, ops, items, gates, psi0, cot_fn)
    assert len(got_d) == len(want_d) and len(got_g) == len(want_g)
    for a, b in zip(got_d, want_d):
        assert np.abs(a - b).max() < 1e-12
    ga, gb = np.concatenate(got_g), np.concatenate(want_g)
    assert np.abs(ga - gb).max() < 1e-11 * np.abs(gb).max()
    assert np.abs(final - o.state).max() < 1e-11


# gate passes of the mirrored forward on the runtime's f32 settings: (bound, bound on stages)
PASS_BOUNDS = {"c2": (42, 542), "c4": (92, None), "c5_26": (114, None), "c5_33": (668, None)}


@pytest.mark.parametrize("c", list(PASS_BOUNDS))
def test_search_saves_passes(c):
    bound, stage_bound = PASS_BOUNDS[c]
    _, ins, _, ops0, items0 = run(c, 1, "1", "1", "0")
    _, ins, _, ops1, items1 = run(c, 1, "1", "1", "1")
    p0, s0 = gate_passes(ins, ops0, items0)
    p1, s1 = gate_passes(ins, ops1, items1)
    print(f"{c}: gate passes {p0} -> {p1}, gate stages {s0} -> {s1}")
    assert p1 <= bound
    if stage_bound:
        assert s1 <= stage_bound


# scheduling time of the commit before the search on the machine that recorded the fixture,
# through the same wrapper: the search may take ten times that
PARENT_SCHED_S = {"c2": 0.023, "c5_33": 0.21}


@pytest.mark.parametrize("c", list(PARENT_SCHED_S))
def test_search_scheduling_time(c):
    circuit(c)
    best = {}
    for search in ("0", "1"):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            run(c, 1, "1", "1", search)
            ts.append(time.perf_counter() - t0)
        best[search] = min(ts)
    print(f"{c}: schedule {best['0']:.3f} s (scan) -> {best['1']:.3f} s (search)")
    assert best["1"] <= 10 * max(PARENT_SCHED_S[c], best["0"])


def _record():
    out = {}
    for c, mode, rq, mir in GRID:
        for prec in precisions(c):
            _, ins, _, ops, items = run(c, mode, rq, mir, "0", prec)
            out[case_id(c, mode, rq, mir, prec)] = {
                "counts": [len(items), *gate_passes(ins, ops, items)], "sha256": digest(items)}
    rows = ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(out.items()))
    GOLDEN.write_text("{\n" + rows + "\n}\n")
    print(f"{len(out)} schedules -> {GOLDEN}")


if __name__ == "__main__":
    if "--record" in sys.argv:
        _record()

#!/usr/bin/env python3
"""Device time of the two-state reading calls and their injections (include/qdc/overlap.h) beside
the one-state calls that read or write the same states.

At n = 28 in f32 and n = 27 in f64 (one state S: 2 GiB), on the primitives' stream with per-launch
events (primitives_profile), two different dense states, one warm-up and then `--reps` timed
calls per row; a call's time is the sum over its kernels (its finalize launches included):

  overlap            <a|b>, 2 S read, beside the one-state norm pass (norm_sq: sample_sums, S)
                     and a read-only two-state reduction of the same bytes (get_q1_grad on qubit 0)
  pauli_overlap      <a|H|b> beside pauli_energy of the same H on one state, for the Ising chain
                     (one window pass and one pass per far bond and site) and a far-only sum
  overlap_inject     conj(g H src) with a complex g beside pauli_inject with a real weight, same H,
                     storing (2 S per pass) and accumulating (3 S)

Each row: launches, ms per call, algorithmic bytes over time as a fraction of 8 TB/s, and the ratio
to the one-state call of the same run.  Then, at n = 24, the wall time of one overlap call against
the host route (two get_cpu_state_copy and np.vdot).

usage: overlap_probe.py [--precision both] [--qubits N] [--reps 3]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "differentiable-quantum-circuit-cuda_amd")]

HBM = 8e12  # bytes / s


def timed(q, prec, reps, fn):
    """(ms per call, launches per call, algorithmic bytes per call) of fn over `reps` calls after
    one warm-up, summed over its kernels."""
    fn()
    q.primitives_profile(True, prec)
    try:
        for _ in range(reps):
            fn()
        stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    return (sum(s["total_ms"] for s in stats.values()) / reps,
            sum(s["launches"] for k, s in stats.items() if k != "finalize") / reps,
            sum(s["algo_bytes"] for s in stats.values()) / reps)


def two_states(q, prec, n):
    """Two different dense states: |+>^n under two different rotations."""
    dt = np.complex64 if prec == "f32" else np.complex128
    had = (np.array([1, 1, 1, -1]) / np.sqrt(2)).astype(dt)
    a = q.QuantizedTensor.new_standard(n, precision=prec)
    for p in range(n):
        a.apply_q1_gate(had, p)
    b = a.clone()
    a.apply_pauli_rotation(f"Z0 Y{n - 1}", 0.7)
    b.apply_pauli_rotation(f"Y1 Z{n - 2}", -1.3)
    return a, b


def row(label, t, ref=None):
    ms, launches, nbytes = t
    tail = f" {ms / ref[0]:7.2f}" if ref else ""
    print(f"{label:34s} {launches:8.0f} {ms:9.3f} {nbytes / (ms * 1e-3) / HBM:9.3f}{tail}",
          flush=True)


def probe(q, prec, n, reps):
    from quantum_differentiable_circuit import PauliSum
    a, b = two_states(q, prec, n)
    out = q.QuantizedTensor(n, prec)
    w = q.observable.plan(PauliSum(1, [(1.0, "Z0")]), prec)["W"]
    s = (8.0 if prec == "f32" else 16.0) * 2.0 ** n
    print(f"# n = {n} {prec}, state S = {s / 2 ** 30:.2f} GiB, {reps} timed calls after one "
          f"warm-up, fractions of {HBM / 1e12:.0f} TB/s; ratio: to the row above")
    print(f"{'call':34s} {'launches':>8s} {'ms':>9s} {'of 8 TB/s':>9s} {'ratio':>7s}")
    norm = timed(q, prec, reps, a.norm_sq)
    row("norm_sq (S)", norm)
    grad = timed(q, prec, reps, lambda: q.get_q1_grad(a, b, 0))
    row("get_q1_grad qubit 0 (2 S)", (grad[0], grad[1], 2 * s))
    row("overlap (2 S)", timed(q, prec, reps, lambda: a.overlap(b)), grad)
    chain = PauliSum(n, [(1.0, f"Z{k} Z{k + 1}") for k in range(n - 1)]
                     + [(0.8, f"X{k}") for k in range(n)])
    far = PauliSum(n, [(0.9, f"X{n - 1}"), (-0.4, f"Y{w} Z3"), (0.6, f"X{w + 1} X0"),
                       (1.1, f"X{n - 1} Z{w}")])
    for name, obs in (("Ising chain", chain), ("far only", far)):
        p = q.observable.plan(obs, prec)
        print(f"# {name}: {len(obs)} terms, {p['window_groups']} window groups in one pass, "
              f"{p['far_groups']} far groups")
        e = timed(q, prec, reps, lambda: a.pauli_energy(obs))
        row(f"pauli_energy {name}", e)
        row(f"pauli_overlap {name}", timed(q, prec, reps, lambda: a.pauli_overlap(b, obs)), e)
        for acc in (False, True):
            word = "accumulating" if acc else "storing"
            i1 = timed(q, prec, reps, lambda: q.pauli_inject(a, out, obs, 0.6, accumulate=acc))
            row(f"pauli_inject {name} {word}", i1)
            i2 = timed(q, prec, reps,
                       lambda: q.overlap_inject(a, out, 0.6 - 1.1j, obs, accumulate=acc))
            row(f"overlap_inject {name} {word}", i2, i1)
    for acc in (False, True):
        word = "accumulating" if acc else "storing"
        row(f"overlap_inject H = I {word}",
            timed(q, prec, reps, lambda: q.overlap_inject(a, out, 0.6 - 1.1j, accumulate=acc)))


def host_route(q, prec, n, reps):
    a, b = two_states(q, prec, n)
    a.overlap(b)
    q.primitives_sync(prec)
    t0 = time.perf_counter()
    for _ in range(reps):
        o = a.overlap(b)
    dev = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        h = np.vdot(a.get_cpu_state_copy(), b.get_cpu_state_copy())
    host = (time.perf_counter() - t0) / reps
    # (np.vdot sums in the arrays' own precision: both against the sum in complex128)
    ref = np.vdot(a.get_cpu_state_copy().astype(np.complex128),
                  b.get_cpu_state_copy().astype(np.complex128))
    print(f"end to end n = {n} {prec}: overlap() {dev * 1e3:9.3f} ms, two copies + np.vdot "
          f"{host * 1e3:9.3f} ms, ratio {host / dev:7.1f}  (error against complex128: overlap() "
          f"{abs(o - ref):.1e}, np.vdot {abs(h - ref):.1e})", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", choices=["f32", "f64", "both"], default="both")
    ap.add_argument("--qubits", type=int, default=0, help="default: 28 (f32) / 27 (f64)")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import quantum_differentiable_circuit as q
    precs = ["f32", "f64"] if a.precision == "both" else [a.precision]
    for prec in precs:
        probe(q, prec, a.qubits or (28 if prec == "f32" else 27), a.reps)
    for prec in precs:
        host_route(q, prec, min(24, a.qubits or 24), a.reps)


if __name__ == "__main__":
    main()

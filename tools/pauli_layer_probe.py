#!/usr/bin/env python3
"""Device time of the diagonal Pauli layers against the route of one rotation per string.

At n = 28 in f32 and n = 27 in f64 (one state: 2 GiB), on the primitives' stream with per-launch
events (primitives_profile), on a uniform superposition state, one warm-up and then `--reps`
timed passes per row, for three layers of ZZ strings: the open chain (n - 1 bonds), the ring
(n bonds) and all-to-all pairs (n (n - 1) / 2):

  (a) pauli_layer (apply_pauli_layer) and pauli_layer_rev (pauli_layer_reverse with its
      gradients; the finalize launches of the reduction are counted with it);
  (b) in the same process and run, the route a user had before: K apply_pauli_rotation calls
      forward and K pauli_rot_reverse calls with their gradients back.

Each row: the layer's launches, device ms per call (the sum over its kernels), algorithmic bytes
over time as a fraction of 8 TB/s, the sequential route's ms, and the ratio of the two.

usage: pauli_layer_probe.py [--precision both] [--qubits N] [--reps 2]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "differentiable-quantum-circuit-cuda_amd")]

HBM = 8e12  # bytes / s


def timed(q, prec, reps, fn):
    """{kernel name: (ms per call, launches per call)} of fn over `reps` calls after one warm-up."""
    fn()
    q.primitives_profile(True, prec)
    try:
        for _ in range(reps):
            fn()
        stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    return {k: (s["total_ms"] / reps, s["launches"] / reps) for k, s in stats.items()}


def probe(q, prec, n, reps):
    dt = np.complex64 if prec == "f32" else np.complex128
    fwd = q.QuantizedTensor.new_standard(n, precision=prec)
    had = (np.array([1, 1, 1, -1]) / np.sqrt(2)).astype(dt)
    for p in range(n):
        fwd.apply_q1_gate(had, p)
    bwd = fwd.conj_and_double()
    s = float(np.dtype(dt).itemsize) * 2.0 ** n
    chain = [f"Z{i} Z{i + 1}" for i in range(n - 1)]
    layers = [("chain", chain), ("ring", chain + [f"Z0 Z{n - 1}"]),
              ("all pairs", [f"Z{j} Z{i}" for i in range(n) for j in range(i)])]
    rng = np.random.default_rng(5)
    print(f"# n = {n} {prec}, state S = {s / 2 ** 30:.2f} GiB, {reps} timed passes after one "
          f"warm-up, fractions of {HBM / 1e12:.0f} TB/s")
    print(f"{'layer':10s} {'K':>4s} {'groups':>6s} | {'launches':>8s} {'layer ms':>9s} "
          f"{'of 8 TB/s':>9s} {'K rot ms':>9s} {'ratio':>7s} | {'launches':>8s} {'rev ms':>9s} "
          f"{'of 8 TB/s':>9s} {'K rev ms':>9s} {'ratio':>7s}")
    for label, strings in layers:
        th = rng.uniform(-np.pi, np.pi, len(strings))
        plan = q.pauli_layer_plan(n, strings, prec)

        def layer():
            fwd.apply_pauli_layer(strings, th)
            q.pauli_layer_reverse(fwd, bwd, strings, th)

        def sequential():
            for ops, t in zip(strings, th):
                fwd.apply_pauli_rotation(ops, t)
            for ops, t in zip(reversed(strings), th[::-1]):
                q.pauli_rot_reverse(fwd, bwd, ops, t)

        st = timed(q, prec, reps, layer)
        lf, nf = st["pauli_layer"]
        lr = sum(ms for k, (ms, _) in st.items() if k != "pauli_layer")  # with its finalize
        nr = st["pauli_layer_rev"][1]
        sq = timed(q, prec, reps, sequential)
        sf = sq["pauli_rot"][0]
        sr = sum(ms for k, (ms, _) in sq.items() if k != "pauli_rot")
        print(f"{label:10s} {len(strings):4d} {plan['groups']:6d} | {nf:8.0f} {lf:9.3f} "
              f"{2 * s * nf / (lf * 1e-3) / HBM:9.3f} {sf:9.3f} {sf / lf:7.1f} | {nr:8.0f} "
              f"{lr:9.3f} {4 * s * nr / (lr * 1e-3) / HBM:9.3f} {sr:9.3f} {sr / lr:7.1f}",
              flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", choices=["f32", "f64", "both"], default="both")
    ap.add_argument("--qubits", type=int, default=0, help="default: 28 (f32) / 27 (f64)")
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    import quantum_differentiable_circuit as q
    for prec in (["f32", "f64"] if a.precision == "both" else [a.precision]):
        probe(q, prec, a.qubits or (28 if prec == "f32" else 27), a.reps)


if __name__ == "__main__":
    main()

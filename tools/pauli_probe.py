#!/usr/bin/env python3
"""Device time of the Pauli-sum observable kernels against the density route.

For n qubits in one precision, on the primitives' stream with per-launch events
(primitives_profile), on a uniform superposition state:

  (a) pauli_energy and pauli_inject (accumulating) for the open transverse-field Ising chain
      sum Z_k Z_{k+1} + g sum X_k, and for a Hamiltonian of n random weight-8 strings;
  (b) the density route for the Ising chain with the primitives that predate the observables:
      forward 2n - 1 densities (n - 1 get_q2density, n get_q1density), backward 2n - 1 times
      conj_and_double / the transposed cotangent as a gate / add.

Each row: device ms per call (the sum over its kernels, finalize launches included), launches
per call, algorithmic bytes over time as a fraction of 8 TB/s.  Then the same per kernel name.

usage: pauli_probe.py --qubits 26 --precision f64 [--reps 3]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "differentiable-quantum-circuit-cuda_amd")]

HBM = 8e12  # bytes / s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--qubits", type=int, default=26)
    ap.add_argument("--precision", choices=["f32", "f64"], default="f64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--field", type=float, default=1.0)
    a = ap.parse_args()
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import PauliSum, observable
    from quantum_differentiable_circuit._native import ptr

    n, prec = a.qubits, a.precision
    dt = np.complex64 if prec == "f32" else np.complex128
    fwd = q.QuantizedTensor.new_standard(n, precision=prec)
    had = (np.array([1, 1, 1, -1]) / np.sqrt(2)).astype(dt)
    for p in range(n):
        fwd.apply_q1_gate(had, p)
    bwd = fwd.conj_and_double()
    tmp = q.QuantizedTensor(n, prec)
    lib = fwd._lib

    ising = PauliSum(n, [(1.0, f"Z{k} Z{k + 1}") for k in range(n - 1)]
                     + [(a.field, f"X{k}") for k in range(n)])
    rng = np.random.default_rng(0)
    weight8 = PauliSum(n, [(float(rng.standard_normal()),
                            [(int(p), "XYZ"[int(rng.integers(3))])
                             for p in rng.permutation(n)[:min(8, n)]]) for _ in range(n)])
    zz = np.ascontiguousarray(np.diag([1.0, -1.0, -1.0, 1.0]).astype(dt).T).reshape(-1)
    xg = np.ascontiguousarray((a.field * np.array([[0, 1], [1, 0]])).astype(dt).T).reshape(-1)

    def density_forward():
        e = 0.0
        for k in range(n - 1):
            e += float(np.dot(fwd.get_q2_density(k + 1, k), zz).real)
        for k in range(n):
            e += float(np.dot(fwd.get_q1_density(k), xg).real)
        return e

    def density_backward():
        for k in range(n - 1):
            lib.conj_and_double(fwd._p, tmp._p, n)
            q.check(lib.q2gate(tmp._p, ptr(zz), k + 1, k, n))
            lib.add(tmp._p, bwd._p, n)
        for k in range(n):
            lib.conj_and_double(fwd._p, tmp._p, n)
            q.check(lib.q1gate(tmp._p, ptr(xg), k, n))
            lib.add(tmp._p, bwd._p, n)

    sections = [
        ("ising pauli_energy", lambda: fwd.pauli_energy(ising)),
        ("ising pauli_inject", lambda: q.pauli_inject(fwd, bwd, ising, 1e-3)),
        ("ising density route fwd", density_forward),
        ("ising density route bwd", density_backward),
        ("weight-8 pauli_energy", lambda: fwd.pauli_energy(weight8)),
        ("weight-8 pauli_inject", lambda: q.pauli_inject(fwd, bwd, weight8, 1e-3)),
    ]
    for name, obs in (("ising", ising), ("weight-8", weight8)):
        p = observable.plan(obs, prec)
        print(f"# plan {name}: W {p['W']}, {p['merged']} terms, {p['window_groups']} window + "
              f"{p['far_groups']} far groups, {p['energy_launches']} launches")
    print(f"# n = {n} {prec}, state {np.dtype(dt).itemsize * 2.0 ** n / 2 ** 30:.2f} GiB, "
          f"{a.reps} repetitions, fractions of {HBM / 1e12:.0f} TB/s")
    rows, kernels = [], {}
    for name, fn in sections:
        fn()  # warm-up (allocations, first launches)
        q.primitives_profile(True, prec)
        try:
            for _ in range(a.reps):
                fn()
            stats = q.primitives_profile_collect(prec)
        finally:
            q.primitives_profile(False, prec)
        ms = sum(s["total_ms"] for s in stats.values()) / a.reps
        launches = sum(s["launches"] for s in stats.values()) / a.reps
        gb = sum(s["algo_bytes"] for s in stats.values()) / a.reps
        rows.append((name, ms, launches, gb))
        for k, s in stats.items():
            if s["algo_bytes"] > 0:
                kernels[(name, k)] = (s["total_ms"] / s["launches"], s["launches"] / a.reps,
                                      s["algo_bytes"] / s["launches"])
    print(f"{'section':28s} {'ms':>10s} {'launches':>9s} {'of 8 TB/s':>10s}")
    for name, ms, launches, b in rows:
        print(f"{name:28s} {ms:10.3f} {launches:9.0f} {b / (ms * 1e-3) / HBM:10.3f}")
    by = dict((r[0], r[1]) for r in rows)
    print(f"# ising energy: density route / pauli = "
          f"{by['ising density route fwd'] / by['ising pauli_energy']:.1f}x; injection: "
          f"{by['ising density route bwd'] / by['ising pauli_inject']:.1f}x")
    print(f"{'section / kernel':44s} {'ms each':>10s} {'launches':>9s} {'of 8 TB/s':>10s}")
    for (name, k), (ms, launches, b) in kernels.items():
        print(f"{name + ' / ' + k:44s} {ms:10.3f} {launches:9.0f} {b / (ms * 1e-3) / HBM:10.3f}")


if __name__ == "__main__":
    main()

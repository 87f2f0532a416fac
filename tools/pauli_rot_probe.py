#!/usr/bin/env python3
"""Device time of the Pauli-rotation kernels against the dense route.

At n = 28 in f32 and n = 27 in f64 (one state: 2 GiB), on the primitives' stream with per-launch
events (primitives_profile), on a uniform superposition state, one warm-up and then `--reps`
timed passes per row, for the strings X0, Z0 Z1, X0 X(n-1), Y3 Z9 X20 and one of weight n:

  (a) pauli_rot (apply_pauli_rotation, 2 S bytes) and pauli_rot_rev (pauli_rot_reverse with its
      gradient, 4 S; the finalize launch of the reduction is counted with it);
  (b) for the strings on at most 5 qubits, in the same run, the route a user had before: the
      rotation's 2^k x 2^k matrix through apply_qk_gate_conj_tr (fwd), get_qk_grad and
      apply_qk_gate_tr (bwd): three calls, 6 S.

Each row: device ms per call (the sum over its kernels), algorithmic bytes over time as a
fraction of 8 TB/s, and the ratio of the three-call route's time to the fused reverse's.

usage: pauli_rot_probe.py [--precision both] [--qubits N] [--reps 3]
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
    from quantum_differentiable_circuit import PauliSum
    dt = np.complex64 if prec == "f32" else np.complex128
    fwd = q.QuantizedTensor.new_standard(n, precision=prec)
    had = (np.array([1, 1, 1, -1]) / np.sqrt(2)).astype(dt)
    for p in range(n):
        fwd.apply_q1_gate(had, p)
    bwd = fwd.conj_and_double()
    s = float(np.dtype(dt).itemsize) * 2.0 ** n
    theta = 0.7
    hi, mid = min(20, n - 2), min(9, n - 3)  # (a smaller --qubits: the same shape of string)
    cases = [[(0, "X")], [(1, "Z"), (0, "Z")], [(n - 1, "X"), (0, "X")],
             [(hi, "X"), (mid, "Z"), (3, "Y")], [(p, "XYZ"[p % 3]) for p in range(n - 1, -1, -1)]]
    print(f"# n = {n} {prec}, state S = {s / 2 ** 30:.2f} GiB, {reps} timed passes after one "
          f"warm-up, fractions of {HBM / 1e12:.0f} TB/s")
    print(f"{'string':16s} {'pauli_rot ms':>13s} {'of 8 TB/s':>10s} {'pauli_rot_rev ms':>17s} "
          f"{'of 8 TB/s':>10s} {'three calls ms':>15s} {'of 8 TB/s':>10s} {'ratio':>6s}")
    for ops in cases:
        label = " ".join(f"{l}{p}" for p, l in reversed(ops)) if len(ops) <= 5 else f"weight {n}"

        def fused():
            fwd.apply_pauli_rotation(ops, theta)
            q.pauli_rot_reverse(fwd, bwd, ops, theta)

        st = timed(q, prec, reps, fused)
        rot = st["pauli_rot"][0]
        rev = sum(ms for k, (ms, _) in st.items() if k != "pauli_rot")  # with its finalize
        row = (f"{label:16s} {rot:13.3f} {2 * s / (rot * 1e-3) / HBM:10.3f} {rev:17.3f} "
               f"{4 * s / (rev * 1e-3) / HBM:10.3f}")
        if len(ops) <= 5:
            pos = [p for p, _ in ops]  # most to least significant: local bit k-1-b is pos[b]
            k = len(pos)
            pk = PauliSum(k, [(1.0, [(k - 1 - i, l) for i, (_, l) in enumerate(ops)])]).to_matrix()
            u = (np.cos(theta / 2) * np.eye(1 << k) - 1j * np.sin(theta / 2) * pk).astype(dt)
            u = np.ascontiguousarray(u.reshape(-1))

            def three_calls():
                fwd.apply_qk_gate_conj_tr(u, pos)
                q.get_qk_grad(fwd, bwd, pos)
                bwd.apply_qk_gate_tr(u, pos)

            st3 = timed(q, prec, reps, three_calls)
            ms3 = sum(ms for ms, _ in st3.values())
            row += f" {ms3:15.3f} {6 * s / (ms3 * 1e-3) / HBM:10.3f} {ms3 / rev:6.2f}"
            row += "   # " + ", ".join(f"{k} {ms:.3f}" for k, (ms, _) in st3.items())
        print(row, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", choices=["f32", "f64", "both"], default="both")
    ap.add_argument("--qubits", type=int, default=0, help="default: 28 (f32) / 27 (f64)")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import quantum_differentiable_circuit as q
    for prec in (["f32", "f64"] if a.precision == "both" else [a.precision]):
        probe(q, prec, a.qubits or (28 if prec == "f32" else 27), a.reps)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the shared-footprint Pauli layers against the route of one rotation per string.

At n = 28 in f32 and n = 27 in f64 (one state: 2 GiB), on the primitives' stream with per-launch
events (primitives_profile), on a uniform superposition state, one warm-up and then `--reps`
timed passes per row.  The layers are the Jordan-Wigner excitations of `excitation(n, occ, virt)`:
a single (K = 2 strings), a double (K = 8) and a triple (K = 32), once on the lowest qubits (the
highest bit of the footprint inside a span) and once on the highest.  Per row, in the same
process and run:

  (a) pauli_xlayer forward, pauli_xlayer_rev without gradients (a constant layer) and with
      gradients (the finalize launches of the reduction are counted with it);
  (b) the route a user had before: the same K strings as K apply_pauli_rotation calls forward
      and K pauli_rot_reverse calls back, without and with gradients.  Their time over K is the
      reference row of one rotation of the footprint (`rot/1`).

Each time is device ms per call (the sum over its kernels); `frac` is algorithmic bytes (2 S
forward, 4 S reverse) over time as a fraction of 8 TB/s; `x` is K rotations over the layer.

usage: pauli_xlayer_probe.py [--precision both] [--qubits N] [--reps 2]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "differentiable-quantum-circuit-cuda_amd")]

HBM = 8e12  # bytes / s


def timed(q, prec, reps, fn):
    """Device ms per call of fn (every kernel it launches) over `reps` calls after one warm-up."""
    fn()
    q.primitives_profile(True, prec)
    try:
        for _ in range(reps):
            fn()
        stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    return sum(s["total_ms"] for s in stats.values()) / reps


def ops_of(n, x, z):
    return [(b, "Y" if z >> b & 1 else "X") if x >> b & 1 else (b, "Z")
            for b in range(n) if (x | z) >> b & 1]


def probe(q, prec, n, reps):
    dt = np.complex64 if prec == "f32" else np.complex128
    fwd = q.QuantizedTensor.new_standard(n, precision=prec)
    had = (np.array([1, 1, 1, -1]) / np.sqrt(2)).astype(dt)
    for p in range(n):
        fwd.apply_q1_gate(had, p)
    bwd = fwd.conj_and_double()
    s = float(np.dtype(dt).itemsize) * 2.0 ** n
    print(f"# n = {n} {prec}, state S = {s / 2 ** 30:.2f} GiB, {reps} timed passes after one "
          f"warm-up, frac = fractions of {HBM / 1e12:.0f} TB/s, x = K rotations / layer")
    print(f"{'footprint':9s} {'K':>3s} | {'fwd ms':>7s} {'frac':>5s} {'K rot':>7s} {'rot/1':>6s} "
          f"{'frac':>5s} {'x':>5s} | {'rev ms':>7s} {'frac':>5s} {'K rev':>7s} {'rev/1':>6s} "
          f"{'frac':>5s} {'x':>5s} | {'grad ms':>7s} {'frac':>5s} {'K grad':>7s} {'grd/1':>6s} "
          f"{'frac':>5s} {'x':>5s}")
    for place in ("low", "high"):
        for m in (1, 2, 3):
            base = 0 if place == "low" else n - 2 * m
            g = q.excitation(n, [base + i for i in range(m)], [base + m + i for i in range(m)])
            k = len(g)
            x = int(g.xmasks[0])
            masks = (x, g.zmasks.copy())
            th = 0.77 * g.coeffs
            rots = [(ops_of(n, x, int(z)), float(t)) for z, t in zip(g.zmasks, th)]
            row = []
            for per, layer, seq in (
                    (2, lambda: fwd.apply_pauli_xlayer(masks, th),
                     lambda: [fwd.apply_pauli_rotation(o, t) for o, t in rots]),
                    (4, lambda: q.pauli_xlayer_reverse(fwd, bwd, masks, th, want_grad=False),
                     lambda: [q.pauli_rot_reverse(fwd, bwd, o, t, want_grad=False) for o, t in rots]),
                    (4, lambda: q.pauli_xlayer_reverse(fwd, bwd, masks, th),
                     lambda: [q.pauli_rot_reverse(fwd, bwd, o, t) for o, t in rots])):
                tl, ts = timed(q, prec, reps, layer), timed(q, prec, reps, seq)
                row.append(f"{tl:7.3f} {per * s / (tl * 1e-3) / HBM:5.3f} {ts:7.3f} {ts / k:6.3f} "
                           f"{per * s * k / (ts * 1e-3) / HBM:5.3f} {ts / tl:5.1f}")
            print(f"{place + ' ' + str(2 * m) + 'q':9s} {k:3d} | " + " | ".join(row), flush=True)


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

#!/usr/bin/env python3
"""Variational quantum deflation on the critical transverse-field Ising ring: the ground state by
the VQE of examples/qaoa_pauli.py, then the first excited state by minimising

    E(theta) + beta |<psi_0|psi(theta)>|^2

with psi_0 the ground state found, held as a device state (DenseCircuit.get_fidelity_op_with_grad:
one overlap pass forward; one overlap pass and one injection backward).

  python examples/vqd_pauli.py [--qubits 8] [--layers 4] [--iters 300] [--beta 4] [--precision f64]

The Hamiltonian and the rotations are those of qaoa_pauli.py (|+>^n, per layer a ZZ rotation on
every bond of the ring and an X rotation on every qubit), with two changes the excited state
needs.  Those rotations all commute with the parity prod_i X_i, and the first excited state has
the other parity than |+>^n: one leading rotation about Z_0, which anticommutes with the parity,
lets the state change sector (phi = 0: even, phi = pi: odd).  And Z_0 singles out a site, so
every rotation has its own angle (1 + 2 n layers parameters) instead of one per layer and kind.
The second stage starts from the ground state's angles with phi = pi / 2, where the penalty's
gradient does not vanish (at phi = 0 it would: there |<psi_0|psi>|^2 is at its maximum).
L-BFGS-B, numpy seed 42.  At --qubits <= 12 both energies are printed next to
numpy.linalg.eigvalsh of PauliSum.to_matrix()."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "differentiable-quantum-circuit-cuda_amd"))

from quantum_differentiable_circuit import PauliSum  # noqa: E402
from quantum_differentiable_circuit.dense_circuit import DenseCircuit  # noqa: E402


def bonds(n):
    return [(i, i + 1) for i in range(n - 1)] + ([(0, n - 1)] if n > 2 else [])


def hamiltonian(n, field=1.0):
    """-sum over the ring's bonds of Z_i Z_j - field sum_i X_i."""
    return PauliSum(n, [(-1.0, f"Z{i} Z{j}") for i, j in bonds(n)]
                    + [(-field, f"X{i}") for i in range(n)])


def parameters(n, layers):
    return 1 + layers * (len(bonds(n)) + n)


def build(n, layers, precision, targets=()):
    """The ansatz, the energy, and one fidelity |<t|psi>|^2 per target state."""
    c = DenseCircuit(n, precision)
    c.set_state_from_vector(np.ones(1 << n, dtype=c.dtype) / np.sqrt(1 << n))
    c.add_var_pauli_rotation("Z0")
    for _ in range(layers):
        for i, j in bonds(n):
            c.add_var_pauli_rotation(f"Z{i} Z{j}")
        for i in range(n):
            c.add_var_pauli_rotation(f"X{i}")
    c.get_observable_op_with_grad(hamiltonian(n))
    for t in targets:
        c.get_fidelity_op_with_grad(t)
    return c


def loss_and_grad(c, angles, beta=0.0):
    """(E + beta sum_k F_k, its gradient in the angles, E, [F_k]): the cotangents are dL/dE = 1
    and dL/dF_k = beta."""
    angles = [float(a) for a in angles]
    energy, *fids = c.forward([], angles)
    grads = c.backward([1.0] + [beta] * len(fids), [], angles)
    return energy + beta * sum(fids), np.array(grads), energy, fids


def optimise(c, start, beta, iters):
    """L-BFGS-B from `start`: (angles, energy, fidelities, calls, seconds per call)."""
    from scipy.optimize import minimize
    calls = [0]

    def f(p):
        calls[0] += 1
        return loss_and_grad(c, p, beta)[:2]

    t0 = time.time()
    r = minimize(f, start, method="L-BFGS-B", jac=True, options={"maxiter": iters})
    per_call = (time.time() - t0) / calls[0]
    _, _, energy, fids = loss_and_grad(c, r.x, beta)
    return r.x, energy, fids, calls[0], per_call


def run(n, layers, iters, beta, precision, seed):
    """Both stages: ((E_0, E_1, |<psi_0|psi_1>|^2), (seconds per call of each stage))."""
    c0 = build(n, layers, precision)
    start = np.random.default_rng(seed).normal(size=parameters(n, layers))
    x0, e0, _, calls0, t0 = optimise(c0, start, 0.0, iters)
    c0.forward([], [float(a) for a in x0])
    psi0 = c0.state.clone()  # the ground state stays on the device
    c1 = build(n, layers, precision, targets=[psi0])
    start = x0.copy()
    start[0] = np.pi / 2
    _, e1, (f1,), calls1, t1 = optimise(c1, start, beta, iters)
    print(f"Number of loss value and gradient calls: {calls0} + {calls1}")
    print(f"Time per loss value and gradient call: {t0} (energy), {t1} (energy + penalty)")
    return (e0, e1, f1), (t0, t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=8)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--beta", type=float, default=4.0,
                    help="penalty weight: above the gap E_1 - E_0")
    ap.add_argument("--precision", default="f64", choices=["f32", "f64"])
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    n = args.qubits
    (e0, e1, f1), _ = run(n, args.layers, args.iters, args.beta, args.precision, args.seed)
    print(f"Ground state energy: {e0}")
    print(f"Excited state energy: {e1}")
    print(f"Overlap with the ground state |<psi_0|psi_1>|^2: {f1}")
    if n <= 12:
        ev = np.linalg.eigvalsh(hamiltonian(n).to_matrix())
        print(f"Exact energies: {ev[0]} {ev[1]}")
        print(f"Errors: {abs(e0 - ev[0])} {abs(e1 - ev[1])}")


if __name__ == "__main__":
    main()

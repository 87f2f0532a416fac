#!/usr/bin/env python3
"""VQE of the critical transverse-field Ising ring with the Hamiltonian given as a PauliSum: the
loop of examples/vqse_ising.py on DenseCircuit, with ONE differentiable observable
(get_observable_op_with_grad) in place of n differentiable densities.  The energy comes back as a
float and the backward takes the weight dL/dE = 1.

  python examples/vqe_pauli.py [--qubits 20] [--layers 10] [--iters 100] [--precision f64]

|+>^n initial state, field 1 (the phase transition), per layer a ZZ rotation on every bond of the
ring and an X rotation on every qubit (two real parameters per layer), L-BFGS-B, numpy seed 42."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
from scipy.optimize import minimize

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


def build(n, layers, precision):
    c = DenseCircuit(n, precision)
    c.set_state_from_vector(np.ones(1 << n, dtype=c.dtype) / np.sqrt(1 << n))
    for _ in range(layers):
        for b in bonds(n):
            c.add_var_gate(b)
        for i in range(n):
            c.add_var_gate([i])
    c.get_observable_op_with_grad(hamiltonian(n))
    return c


def gates_of(params, n, dtype):
    """(gates in instruction order, d gate / d parameter of each gate)."""
    nb = len(bonds(n))
    gates, dgates = [], []
    for layer in range(len(params) // 2):
        g, b = float(params[2 * layer]), float(params[2 * layer + 1])
        zz = np.diag([np.exp(-1j * g), np.exp(1j * g), np.exp(1j * g), np.exp(-1j * g)])
        dzz = np.diag([-1j * np.exp(-1j * g), 1j * np.exp(1j * g), 1j * np.exp(1j * g),
                       -1j * np.exp(-1j * g)])
        x = np.array([np.cos(b), -1j * np.sin(b), -1j * np.sin(b), np.cos(b)])
        dx = np.array([-np.sin(b), -1j * np.cos(b), -1j * np.cos(b), -np.sin(b)])
        gates += [zz.reshape(-1).astype(dtype)] * nb + [x.astype(dtype)] * n
        dgates += [dzz.reshape(-1)] * nb + [dx] * n
    return gates, dgates


def loss_and_grad(c, params, n):
    """E = <psi|H|psi> and its gradient in the real parameters: Re sum over a parameter's gates
    of (gate gradient . d gate / d parameter)."""
    nb = len(bonds(n))
    gates, dgates = gates_of(params, n, c.dtype)
    (energy,) = c.forward([], gates)
    grads = c.backward([1.0], [], gates)
    per_gate = [np.real(np.sum(np.asarray(g) * d)) for g, d in zip(grads, dgates)]
    grad = np.zeros(len(params))
    k = 0
    for layer in range(len(params) // 2):
        grad[2 * layer] = sum(per_gate[k:k + nb])
        grad[2 * layer + 1] = sum(per_gate[k + nb:k + nb + n])
        k += nb + n
    return energy, grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=20)
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--precision", default="f64", choices=["f32", "f64"])
    ap.add_argument("--seed", type=int, default=42)
    args = ap.parse_args()
    n = args.qubits
    c = build(n, args.layers, args.precision)
    params = np.random.default_rng(args.seed).normal(size=2 * args.layers)
    calls = [0]

    def loss_val_and_grad(p):
        calls[0] += 1
        return loss_and_grad(c, p, n)

    start = time.time()
    result = minimize(loss_val_and_grad, params, method="L-BFGS-B", jac=True,
                      options={"maxiter": args.iters})
    end = time.time()
    exact_e = -2 * (1 / np.sin(np.pi / (2 * n)))
    print(f"Exact energy: {exact_e}")
    print(f"Found energy: {result.fun}")
    print(f"Relative error: {abs(result.fun - exact_e) / abs(exact_e)}")
    print(f"Number of loss value and gradient calls: {calls[0]}")
    print(f"Time per loss value and gradient call: {(end - start) / calls[0]}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The VQE of examples/vqe_pauli.py with Pauli strings on both sides: the ansatz is made of
Pauli rotations exp(-i theta/2 P) (DenseCircuit.add_var_pauli_rotation) and the Hamiltonian is a
PauliSum.  Parameters go in as angles and gradients come back as floats: no gate matrices, no
d gate / d parameter chain on the host.

  python examples/qaoa_pauli.py [--qubits 20] [--layers 10] [--iters 100] [--precision f64]
                                [--cost-layer] [--shots K]

Per layer a ZZ rotation on every bond of the ring with theta = 2 g and an X rotation on every qubit
with theta = 2 b: the gates exp(-i g ZZ) and exp(-i b X) vqe_pauli.py writes as matrices, so the same
parameters give the same energy and the same gradient.  With --cost-layer each layer's bonds are
one diagonal Pauli layer exp(-i theta/2 sum ZZ) (DenseCircuit.add_var_pauli_evolution): one pass
over the state per layer and direction instead of one per bond.  With --shots K the optimised
state is sampled K times on the device (QuantizedTensor.sample): the five most frequent
bitstrings, and the sample mean of the cost -sum Z_i Z_j beside its expectation value."""
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


def build(n, layers, precision, cost_layer=False):
    c = DenseCircuit(n, precision)
    c.set_state_from_vector(np.ones(1 << n, dtype=c.dtype) / np.sqrt(1 << n))
    for _ in range(layers):
        if cost_layer:
            c.add_var_pauli_evolution(PauliSum(n, [(1.0, f"Z{i} Z{j}") for i, j in bonds(n)]))
        else:
            for i, j in bonds(n):
                c.add_var_pauli_rotation(f"Z{i} Z{j}")
        for i in range(n):
            c.add_var_pauli_rotation(f"X{i}")
    c.get_observable_op_with_grad(hamiltonian(n))
    return c


def angles_of(params, n, cost_layer=False):
    """The rotations' angles in instruction order: theta = 2 g on the bonds (once for a cost
    layer), 2 b on the sites."""
    nb = 1 if cost_layer else len(bonds(n))
    angles = []
    for layer in range(len(params) // 2):
        angles += [2.0 * float(params[2 * layer])] * nb + [2.0 * float(params[2 * layer + 1])] * n
    return angles


def loss_and_grad(c, params, n, cost_layer=False):
    """E = <psi|H|psi> and its gradient in the real parameters: d theta / d parameter = 2 times
    the sum of dE/dtheta over the parameter's rotations."""
    nb = 1 if cost_layer else len(bonds(n))
    angles = angles_of(params, n, cost_layer)
    (energy,) = c.forward([], angles)
    dtheta = c.backward([1.0], [], angles)
    grad = np.zeros(len(params))
    k = 0
    for layer in range(len(params) // 2):
        grad[2 * layer] = 2.0 * sum(dtheta[k:k + nb])
        grad[2 * layer + 1] = 2.0 * sum(dtheta[k + nb:k + nb + n])
        k += nb + n
    return energy, grad


def report_sample(c, params, n, shots, seed, cost_layer=False):
    """Sample the state the parameters prepare: the most frequent bitstrings (qubit 0 rightmost)
    and the sample mean of the cost -sum Z_i Z_j beside <psi| -sum Z_i Z_j |psi>."""
    c.forward([], angles_of(params, n, cost_layer))
    values, counts = c.state.sample_counts(shots, seed=seed)
    for k in np.argsort(-counts, kind="stable")[:5]:
        print(f"Sampled {int(values[k]):0{n}b}: {int(counts[k])} of {shots}")
    cost = np.zeros(values.size)
    for i, j in bonds(n):
        zz = ((values >> np.uint64(i)) ^ (values >> np.uint64(j))) & np.uint64(1)
        cost -= 1.0 - 2.0 * zz.astype(np.float64)
    mean = float(np.dot(cost, counts)) / shots
    zpart = PauliSum(n, [(-1.0, f"Z{i} Z{j}") for i, j in bonds(n)])
    print(f"Sample mean of -sum ZZ: {mean}")
    print(f"Expectation of -sum ZZ: {c.state.pauli_energy(zpart)}")


def main():
    from scipy.optimize import minimize
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=20)
    ap.add_argument("--layers", type=int, default=10)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--precision", default="f64", choices=["f32", "f64"])
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--cost-layer", action="store_true",
                    help="one diagonal Pauli layer per layer of bonds")
    ap.add_argument("--shots", type=int, default=0,
                    help="bitstrings to sample from the optimised state (0: none)")
    args = ap.parse_args()
    n = args.qubits
    c = build(n, args.layers, args.precision, args.cost_layer)
    params = np.random.default_rng(args.seed).normal(size=2 * args.layers)
    calls = [0]

    def loss_val_and_grad(p):
        calls[0] += 1
        return loss_and_grad(c, p, n, args.cost_layer)

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
    if args.shots > 0:
        report_sample(c, result.x, n, args.shots, args.seed, args.cost_layer)


if __name__ == "__main__":
    main()

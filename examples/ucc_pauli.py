#!/usr/bin/env python3
"""VQE of a small Fermi-Hubbard chain with a singles-and-doubles excitation ansatz, Pauli strings
on both sides: every excitation exp(theta/2 (tau - tau^dagger)) is one shared-footprint Pauli layer
(DenseCircuit.add_var_excitation: 2 strings for a single, 8 for a double, one pass over the state
each), and the Hamiltonian is a PauliSum.  No gate matrices, no JAX.

  python examples/ucc_pauli.py [--qubits 12] [--layers 2] [--steps 40] [--precision f64]
                               [--per-string]

Qubit 2 s + sigma is the spin orbital (site s, spin sigma) under Jordan-Wigner, value 1 = occupied.
H = -t sum_{<s,s'>,sigma} (a^dagger_{s sigma} a_{s' sigma} + h.c.) + U sum_s n_{s up} n_{s down}
on an open chain of qubits / 2 sites, built from the ladder operators of
quantum_differentiable_circuit.ladder_terms.  The reference state is the half-filled product state
with alternating spins.  Per layer: a single excitation of every electron to each neighbouring
site, then a double excitation on every bond (the two electrons of the bond exchange their
sites).  Every excitation conserves the particle number, which is printed beside the energy of
each gradient-descent step.  With --per-string every string of an excitation is its own
add_var_pauli_rotation with the angle theta c_k: the same unitary, one pass per string."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "differentiable-quantum-circuit-cuda_amd"))

from quantum_differentiable_circuit import PauliSum, excitation, ladder_terms  # noqa: E402
from quantum_differentiable_circuit.dense_circuit import DenseCircuit  # noqa: E402


def mode(site, spin):
    return 2 * site + spin


def hermitian_sum(n, weighted):
    """PauliSum of sum_w w * (product of ladder operators), which must come out Hermitian."""
    total = {}
    for w, ops in weighted:
        for key, c in ladder_terms(n, ops).items():
            total[key] = total.get(key, 0.0) + w * c
    assert all(abs(c.imag) < 1e-12 for c in total.values())
    keys = [k for k, c in total.items() if abs(c.real) > 1e-12]
    return PauliSum.from_masks(n, [total[k].real for k in keys], [k[0] for k in keys],
                               [k[1] for k in keys])


def hamiltonian(n, t=1.0, u=2.0):
    sites = n // 2
    terms = []
    for s in range(sites - 1):
        for spin in (0, 1):
            p, q = mode(s, spin), mode(s + 1, spin)
            terms += [(-t, [(p, True), (q, False)]), (-t, [(q, True), (p, False)])]
    for s in range(sites):
        up, dn = mode(s, 0), mode(s, 1)
        terms.append((u, [(up, True), (up, False), (dn, True), (dn, False)]))
    return hermitian_sum(n, terms)


def number_operator(n):
    return hermitian_sum(n, [(1.0, [(q, True), (q, False)]) for q in range(n)])


def reference_index(n):
    """Site s holds one electron of spin s mod 2."""
    return sum(1 << mode(s, s % 2) for s in range(n // 2))


def excitations(n):
    """(occ, virt) of one layer, relative to the reference state."""
    sites = n // 2
    out = []
    for s in range(sites):
        for nb in (s - 1, s + 1):
            if 0 <= nb < sites:
                out.append(([mode(s, s % 2)], [mode(nb, s % 2)]))
    for s in range(sites - 1):
        a, b = s % 2, (s + 1) % 2
        out.append(([mode(s, a), mode(s + 1, b)], [mode(s + 1, a), mode(s, b)]))
    return out


def build(n, layers, precision, per_string=False):
    """(circuit, generators): one generator (a PauliSum) per variational angle."""
    c = DenseCircuit(n, precision)
    psi = np.zeros(1 << n, dtype=c.dtype)
    psi[reference_index(n)] = 1
    c.set_state_from_vector(psi)
    gens = []
    for _ in range(layers):
        for occ, virt in excitations(n):
            g = excitation(n, occ, virt)
            gens.append(g)
            if per_string:
                for _, x, z in g.terms():
                    ops = [(q, "Y" if z >> q & 1 else "X") if x >> q & 1 else (q, "Z")
                           for q in range(n) if (x | z) >> q & 1]
                    c.add_var_pauli_rotation(ops)
            else:
                c.add_var_excitation(occ, virt)
    c.get_observable_op_with_grad(hamiltonian(n))
    return c, gens


def loss_and_grad(c, gens, params, per_string=False, number=None):
    """(E, dE/dtheta per excitation, <N>): E = <psi|H|psi>; per string theta_k = theta c_k and the
    gradient is sum_k c_k dE/dtheta_k; <N> the expectation of ``number`` in the prepared state
    (None without it)."""
    if not per_string:
        angles = [float(p) for p in params]
        (energy,) = c.forward([], angles)
        particles = c.state.pauli_energy(number) if number is not None else None
        return energy, np.array(c.backward([1.0], [], angles)), particles
    angles = [float(p) * ck for p, g in zip(params, gens) for ck in g.coeffs]
    (energy,) = c.forward([], angles)
    particles = c.state.pauli_energy(number) if number is not None else None
    d = c.backward([1.0], [], angles)
    grad, k = np.zeros(len(gens)), 0
    for i, g in enumerate(gens):
        grad[i] = float(np.dot(g.coeffs, d[k:k + len(g)]))
        k += len(g)
    return energy, grad, particles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qubits", type=int, default=12, help="spin orbitals (even): 2 per site")
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--precision", default="f64", choices=["f32", "f64"])
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--per-string", action="store_true",
                    help="one Pauli rotation per string in place of one layer per excitation")
    args = ap.parse_args()
    n = args.qubits
    if n < 4 or n % 2:
        ap.error("--qubits must be even and at least 4")
    c, gens = build(n, args.layers, args.precision, args.per_string)
    number = number_operator(n)
    params = 0.1 * np.random.default_rng(args.seed).normal(size=len(gens))
    print(f"{n // 2} sites, {len(gens)} excitations, "
          f"{sum(len(g) for g in gens)} Pauli strings, {len(c.instructions) - 1} passes forward")
    start = time.time()
    for step in range(args.steps):
        energy, grad, particles = loss_and_grad(c, gens, params, args.per_string, number)
        print(f"Step {step}: energy {energy:.10f}  particles {particles:.10f}")
        params = params - args.rate * grad
    print(f"Time per step: {(time.time() - start) / max(1, args.steps)}")


if __name__ == "__main__":
    main()

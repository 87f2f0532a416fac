"""A differentiable circuit of dense gates and densities on 1..5 qubits.

``DenseCircuit`` has the shape and the call order of ``AbiCircuit`` (``abi_circuit.py``, which
restates ``src/circuit.rs:164-429``), over the dense k-qubit primitives of ``include/qdc/dense.h``
in place of the q1 / q2 ones:

* forward: one ``qdc_qkgate`` per gate, ``qdc_qkdensity`` (a host sync each) per density;
* backward, walking the instructions in reverse, per gate: ``apply_qk_gate_conj_tr`` on fwd (the
  uncompute), then, once a cotangent has been injected, ``get_qk_grad(fwd, bwd, positions)`` for
  a variable gate and ``apply_qk_gate_tr`` on bwd; per differentiable density:
  ``conj_and_double`` into a new state, ``apply_qk_gate_tr(cotangent)`` on it, then ``add`` into
  bwd (the first one becomes bwd); per differentiable observable (a ``PauliSum``, its cotangent
  a real weight dL/dE): one ``pauli_inject(fwd, bwd, obs, weight)``, with ``accumulate=False``
  into a newly allocated bwd when it is the first cotangent, ``accumulate=True`` otherwise.
  Variable gates met before the first cotangent get zero gradients.

An observable's forward value is ``state.pauli_energy(obs)``, a Python float, at its place in
instruction order among the densities.

A Pauli rotation ``exp(-i theta/2 P)`` (``add_const_pauli_rotation`` / ``add_var_pauli_rotation``)
takes its angle, a real scalar, from the same FIFO as the gates of its class: forward is one
``apply_pauli_rotation``, backward one ``pauli_rot_reverse(fwd, bwd, ops, theta)`` (``bwd=None``
before the first cotangent), and a variable rotation's gradient is dL/dtheta, a Python float at
its place among the variable gates' gradients (0.0 before the first cotangent).

A diagonal Pauli layer ``exp(-i/2 sum_k theta_k P_k)`` of Z-only strings
(``add_const_pauli_layer`` / ``add_var_pauli_layer``) takes one FIFO entry of its class, the real
array of its K angles: forward is one ``apply_pauli_layer``, backward one ``pauli_layer_reverse``,
and a variable layer's gradient is a float64 array of K (zeros before the first cotangent).
``add_const_pauli_evolution(H)`` / ``add_var_pauli_evolution(H)`` is the same layer with one real
scalar theta for a ``PauliSum`` H of Z strings, ``U = exp(-i theta/2 H)`` (theta_k = theta c_k,
the QAOA cost layer); its gradient is the float ``sum_k c_k dtheta_k``.

``add_const_pauli_xlayer`` / ``add_var_pauli_xlayer``, ``add_const_pauli_xevolution`` /
``add_var_pauli_xevolution`` are the same two instructions for commuting strings that share their
X/Y positions (``apply_pauli_xlayer`` / ``pauli_xlayer_reverse``), and
``add_const_excitation(occ, virt)`` / ``add_var_excitation(occ, virt)`` is the xevolution of
``excitation(n, occ, virt)``: ``exp(theta/2 (tau - tau^dagger))``, a fermionic excitation under
Jordan-Wigner in one pass.

``get_sample_op(shots, seed, qubits)`` draws bitstrings from the state at its place
(``state.sample``): not differentiable, like ``get_dens_op``.  ``run`` returns its uint64 array at
its place among the outputs; ``forward`` and ``backward`` skip it.  An int seed gives the same
sample on every ``run``, ``seed=None`` a fresh one.

``get_overlap_op(target, obs=None)`` / ``get_overlap_op_with_grad`` read the transition element
o = <target|H|psi> of the state at their place against a constant ``target`` (``obs=None``: H = I,
the plain overlap; ``include/qdc/overlap.h``), a Python ``complex`` at its place among the outputs.
``target`` is a ``QuantizedTensor`` of the circuit's size and precision, held by reference (the
caller may refill it between calls), or a host vector, uploaded once when the op is added.  The
differentiable op's cotangent in ``grads_wrt_density`` is the complex g = dL/dRe o + i dL/dIm o of
a real loss L; backward is one ``overlap_inject(target, bwd, g, obs)``: bwd (+)= conj(g H target),
into a newly allocated bwd when it is the first cotangent.  ``get_fidelity_op(target)`` /
``get_fidelity_op_with_grad`` yield the float F = |<target|psi>|^2; the cotangent is a real weight
w, and backward recomputes o on the uncomputed forward state (one overlap pass; nothing is cached
from forward, as for an observable) and injects with g = 2 w o.  ``run`` yields both kinds of op,
``forward`` only the differentiable ones.  The target is a constant: nothing is differentiated
through it.

Gates are 1-D arrays of 4^k values (2^k x 2^k row-major, local index bit (k-1-b) = qubit
positions[b]); densities come back as (2^k, 2^k) arrays and gradients as 1-D arrays in forward
order.  At k = 1, 2 every call lands on the q1 / q2 kernels, so a circuit of 1- and 2-qubit
instructions computes what ``AbiCircuit`` computes, bit for bit.

Gates are assumed unitary: the uncompute applies the conjugate transpose.  Non-unitary dense
gates would need a 2^k x 2^k LU inverse on the host and are out of scope.  No fusion: every
instruction is one primitive call (the fused runtime, ``Circuit``, has no dense instruction
kinds).
"""
from __future__ import annotations

from collections import deque
from typing import List

import numpy as np

from . import (PanicException, PauliSum, QuantizedTensor, _real_angle, data_transfer, excitation,
               get_qk_grad, layer_angles, layer_masks, overlap_inject, pauli_inject,
               pauli_layer_reverse, pauli_masks, pauli_rot_reverse, pauli_xlayer_reverse,
               xevolution_masks, xlayer_masks)
from .abi_circuit import _slice

(CONST_GATE, VAR_GATE, DENSITY, DIFF_DENSITY, OBSERVABLE, DIFF_OBSERVABLE, CONST_ROT,
 VAR_ROT, CONST_LAYER, VAR_LAYER, CONST_EVOL, VAR_EVOL, SAMPLE, CONST_XLAYER, VAR_XLAYER,
 CONST_XEVOL, VAR_XEVOL, OVERLAP, DIFF_OVERLAP, FIDELITY, DIFF_FIDELITY) = range(21)
_CONST_KINDS = (CONST_GATE, CONST_ROT, CONST_LAYER, CONST_EVOL, CONST_XLAYER, CONST_XEVOL)
_XLAYER_KINDS = (CONST_XLAYER, VAR_XLAYER, CONST_XEVOL, VAR_XEVOL)



class DenseCircuit:
    def __init__(self, qubits_number: int, precision: str | None = None):
        self.initial_state = QuantizedTensor.new_standard(qubits_number, precision)
        self.state = self.initial_state.clone()
        self.instructions = []
        self.dtype = self.initial_state.dtype
        self.bwd = None

    def set_state_from_vector(self, vector):
        self.initial_state.set_from_host(np.asarray(vector, dtype=self.dtype))

    # --- builders -------------------------------------------------------------------------
    def _push(self, kind, positions):
        pos = tuple(int(p) for p in positions)
        if not 1 <= len(pos) <= 5:
            raise PanicException("k must be in 1..5.")
        if len(set(pos)) != len(pos):
            raise PanicException("positions must be different.")
        if max(pos) >= self.state.qubits_number:
            raise PanicException("pos is out of the bound.")
        self.instructions.append((kind, pos))

    def add_const_gate(self, positions): self._push(CONST_GATE, positions)
    def add_var_gate(self, positions): self._push(VAR_GATE, positions)
    def get_dens_op(self, positions): self._push(DENSITY, positions)
    def get_dens_op_with_grad(self, positions): self._push(DIFF_DENSITY, positions)

    def _push_observable(self, kind, obs):
        if not isinstance(obs, PauliSum):
            raise TypeError("argument 'obs': expected a PauliSum")
        if obs.qubits_number != self.state.qubits_number:
            raise PanicException("The observable and the tensor have different sizes.")
        if len(obs) == 0:
            raise PanicException("The observable has no terms.")
        self.instructions.append((kind, obs))

    def get_observable_op(self, obs): self._push_observable(OBSERVABLE, obs)
    def get_observable_op_with_grad(self, obs): self._push_observable(DIFF_OBSERVABLE, obs)

    def _push_overlap(self, kind, target, obs):
        s = self.state
        if isinstance(target, QuantizedTensor):  # held by reference: the caller may refill it
            s._same_shape(target)
        else:  # a host vector, uploaded once
            v = np.asarray(target).reshape(-1)
            if v.size != 1 << s.qubits_number:
                raise PanicException("The two tensors have different sizes.")
            target = QuantizedTensor.new_from_host(v, s._precision)
        if obs is not None:
            if not isinstance(obs, PauliSum):
                raise TypeError("argument 'obs': expected a PauliSum")
            if obs.qubits_number != s.qubits_number:
                raise PanicException("The observable and the tensor have different sizes.")
            if len(obs) == 0:
                raise PanicException("The observable has no terms.")
        self.instructions.append((kind, (target, obs)))

    def get_overlap_op(self, target, obs=None): self._push_overlap(OVERLAP, target, obs)

    def get_overlap_op_with_grad(self, target, obs=None):
        self._push_overlap(DIFF_OVERLAP, target, obs)

    def get_fidelity_op(self, target): self._push_overlap(FIDELITY, target, None)
    def get_fidelity_op_with_grad(self, target): self._push_overlap(DIFF_FIDELITY, target, None)

    @staticmethod
    def _overlap(target, obs, s) -> complex:
        """<target|H|s> (H = I when obs is None)."""
        return target.overlap(s) if obs is None else target.pauli_overlap(s, obs)

    def _push_rotation(self, kind, ops):
        ops = ops if isinstance(ops, str) else tuple(ops)
        pauli_masks(self.state.qubits_number, ops)  # its panics, when the circuit is built
        self.instructions.append((kind, ops))

    def add_const_pauli_rotation(self, ops): self._push_rotation(CONST_ROT, ops)
    def add_var_pauli_rotation(self, ops): self._push_rotation(VAR_ROT, ops)

    def _push_layer(self, kind, strings):
        strings = tuple(s if isinstance(s, str) else tuple(s) for s in strings)
        if not strings:
            raise PanicException("The layer has no terms.")
        # (the parser's panics when the circuit is built; the masks are kept, not the strings)
        self.instructions.append((kind, (layer_masks(self.state.qubits_number, strings), None)))

    def add_const_pauli_layer(self, strings): self._push_layer(CONST_LAYER, strings)
    def add_var_pauli_layer(self, strings): self._push_layer(VAR_LAYER, strings)

    def _push_evolution(self, kind, h):
        if not isinstance(h, PauliSum):
            raise TypeError("argument 'H': expected a PauliSum")
        if h.qubits_number != self.state.qubits_number:
            raise PanicException("The observable and the tensor have different sizes.")
        if len(h) == 0:
            raise PanicException("The layer has no terms.")
        if np.any(h.xmasks != 0):
            raise PanicException("a Pauli layer takes Z strings only.")
        self.instructions.append((kind, (h.zmasks.copy(), h.coeffs.copy())))

    def add_const_pauli_evolution(self, h): self._push_evolution(CONST_EVOL, h)
    def add_var_pauli_evolution(self, h): self._push_evolution(VAR_EVOL, h)

    def _push_xlayer(self, kind, strings):
        if not (isinstance(strings, tuple) and len(strings) == 2
                and isinstance(strings[1], np.ndarray)):
            strings = tuple(s if isinstance(s, str) else tuple(s) for s in strings)
        if len(strings) == 0:
            raise PanicException("The layer has no terms.")
        x, zmasks = xlayer_masks(self.state.qubits_number, strings)
        if zmasks.size == 0:
            raise PanicException("The layer has no terms.")
        self.instructions.append((kind, ((x, zmasks), None)))

    def add_const_pauli_xlayer(self, strings): self._push_xlayer(CONST_XLAYER, strings)
    def add_var_pauli_xlayer(self, strings): self._push_xlayer(VAR_XLAYER, strings)

    def _push_xevolution(self, kind, h):
        if not isinstance(h, PauliSum):
            raise TypeError("argument 'H': expected a PauliSum")
        if h.qubits_number != self.state.qubits_number:
            raise PanicException("The observable and the tensor have different sizes.")
        if len(h) == 0:
            raise PanicException("The layer has no terms.")
        x, zmasks, coeffs = xevolution_masks(h)
        self.instructions.append((kind, ((x, zmasks), coeffs)))

    def add_const_pauli_xevolution(self, h): self._push_xevolution(CONST_XEVOL, h)
    def add_var_pauli_xevolution(self, h): self._push_xevolution(VAR_XEVOL, h)

    def add_const_excitation(self, occ, virt):
        self._push_xevolution(CONST_XEVOL, excitation(self.state.qubits_number, occ, virt))

    def add_var_excitation(self, occ, virt):
        self._push_xevolution(VAR_XEVOL, excitation(self.state.qubits_number, occ, virt))

    def get_sample_op(self, shots, seed=None, qubits=None):
        shots = int(shots)
        if shots < 0:
            raise ValueError("shots must be >= 0")
        if qubits is not None:
            qubits = tuple(int(q) for q in qubits)
            if len(set(qubits)) != len(qubits) or \
                    any(q < 0 or q >= self.state.qubits_number for q in qubits):
                raise PanicException("pos is out of the bound.")
        self.instructions.append((SAMPLE, (shots, seed, qubits)))

    @staticmethod
    def _layer_angles(kind, pos, entry):
        """The K angles of a layer instruction from its FIFO entry."""
        masks, coeffs = pos
        if coeffs is not None:
            return _real_angle(entry) * coeffs
        return layer_angles(entry, (masks[1] if kind in _XLAYER_KINDS else masks).size)

    # --- forward --------------------------------------------------------------------------
    def _forward(self, const_gates, var_gates, all_densities) -> List[np.ndarray]:
        if not self.instructions:
            raise PanicException("The circuit is empty.")
        out = []
        cg, vg = deque(const_gates), deque(var_gates)
        data_transfer(self.initial_state, self.state)
        s = self.state
        for kind, pos in self.instructions:
            if kind in (CONST_GATE, VAR_GATE):
                pool = cg if kind == CONST_GATE else vg
                if not pool:
                    word = "constant" if kind == CONST_GATE else "variable"
                    raise PanicException(f"The number of {word} gates is less than required.")
                s.apply_qk_gate(_slice(pool.popleft()), pos)
            elif kind in (CONST_ROT, VAR_ROT):
                pool = cg if kind == CONST_ROT else vg
                if not pool:
                    word = "constant" if kind == CONST_ROT else "variable"
                    raise PanicException(f"The number of {word} gates is less than required.")
                s.apply_pauli_rotation(pos, _real_angle(pool.popleft()))
            elif kind in (CONST_LAYER, VAR_LAYER, CONST_EVOL, VAR_EVOL):
                pool = cg if kind in _CONST_KINDS else vg
                if not pool:
                    word = "constant" if kind in _CONST_KINDS else "variable"
                    raise PanicException(f"The number of {word} gates is less than required.")
                s.apply_pauli_layer(pos[0], self._layer_angles(kind, pos, pool.popleft()))
            elif kind in _XLAYER_KINDS:
                pool = cg if kind in _CONST_KINDS else vg
                if not pool:
                    word = "constant" if kind in _CONST_KINDS else "variable"
                    raise PanicException(f"The number of {word} gates is less than required.")
                s.apply_pauli_xlayer(pos[0], self._layer_angles(kind, pos, pool.popleft()))
            elif kind in (OBSERVABLE, DIFF_OBSERVABLE):
                if kind == DIFF_OBSERVABLE or all_densities:
                    out.append(s.pauli_energy(pos))
            elif kind in (OVERLAP, DIFF_OVERLAP):
                if kind == DIFF_OVERLAP or all_densities:
                    out.append(self._overlap(*pos, s))
            elif kind in (FIDELITY, DIFF_FIDELITY):
                if kind == DIFF_FIDELITY or all_densities:
                    out.append(abs(self._overlap(*pos, s)) ** 2)
            elif kind == SAMPLE:
                if all_densities:
                    shots, seed, qubits = pos
                    out.append(s.sample(shots, seed, qubits=qubits))
            elif kind == DIFF_DENSITY or all_densities:
                c = 1 << len(pos)
                out.append(s.get_qk_density(pos).reshape(c, c))
        if cg:
            raise PanicException("Number of constant gates is more than required.")
        if vg:
            raise PanicException("Number of variable gates is more than required.")
        return out

    def run(self, const_gates, var_gates):
        """Every density matrix, every observable's energy, every overlap and fidelity and every
        sample, in instruction order."""
        return self._forward(const_gates, var_gates, True)

    def forward(self, const_gates, var_gates):
        """The differentiable density matrices, energies, overlaps and fidelities, in instruction
        order."""
        return self._forward(const_gates, var_gates, False)

    # --- backward -------------------------------------------------------------------------
    def backward(self, grads_wrt_density, const_gates, var_gates) -> List[np.ndarray]:
        """Gradients of the variable gates, forward order; call after ``forward`` with the same
        gates.  ``grads_wrt_density`` holds, in the order of ``forward``'s outputs, a cotangent
        matrix per differentiable density, a real weight per differentiable observable or
        fidelity and a complex g = dL/dRe o + i dL/dIm o per differentiable overlap.
        Leaves the forward state uncomputed back to the initial state."""
        if not self.instructions:
            raise PanicException("The circuit is empty.")
        dens, cg, vg = list(grads_wrt_density), list(const_gates), list(var_gates)
        fwd = self.state
        bwd = None
        grads = deque()
        for kind, pos in reversed(self.instructions):
            if kind in (CONST_GATE, VAR_GATE):
                pool = cg if kind == CONST_GATE else vg
                if not pool:
                    raise PanicException("The number of gates is less than required.")
                g = _slice(pool.pop())
                fwd.apply_qk_gate_conj_tr(g, pos)
                if bwd is not None:
                    if kind == VAR_GATE:
                        grads.appendleft(get_qk_grad(fwd, bwd, pos))
                    bwd.apply_qk_gate_tr(g, pos)
                elif kind == VAR_GATE:
                    grads.appendleft(np.zeros(1 << (2 * len(pos)), self.dtype))
            elif kind in (CONST_ROT, VAR_ROT):
                pool = cg if kind == CONST_ROT else vg
                if not pool:
                    raise PanicException("The number of gates is less than required.")
                d = pauli_rot_reverse(fwd, bwd, pos, _real_angle(pool.pop()),
                                      want_grad=kind == VAR_ROT)
                if kind == VAR_ROT:
                    grads.appendleft(d)
            elif kind in (CONST_LAYER, VAR_LAYER, CONST_EVOL, VAR_EVOL):
                pool = cg if kind in _CONST_KINDS else vg
                if not pool:
                    raise PanicException("The number of gates is less than required.")
                d = pauli_layer_reverse(fwd, bwd, pos[0], self._layer_angles(kind, pos, pool.pop()),
                                        want_grad=kind in (VAR_LAYER, VAR_EVOL))
                if kind == VAR_LAYER:
                    grads.appendleft(d)
                elif kind == VAR_EVOL:
                    grads.appendleft(float(np.dot(pos[1], d)))
            elif kind in _XLAYER_KINDS:
                pool = cg if kind in _CONST_KINDS else vg
                if not pool:
                    raise PanicException("The number of gates is less than required.")
                d = pauli_xlayer_reverse(fwd, bwd, pos[0],
                                         self._layer_angles(kind, pos, pool.pop()),
                                         want_grad=kind in (VAR_XLAYER, VAR_XEVOL))
                if kind == VAR_XLAYER:
                    grads.appendleft(d)
                elif kind == VAR_XEVOL:
                    grads.appendleft(float(np.dot(pos[1], d)))
            elif kind == DIFF_DENSITY:
                if not dens:
                    raise PanicException(
                        "The number of gradients wrt density matrices is less than required.")
                gd = _slice(dens.pop(), "Gradient is not contiguous.")
                addition = fwd.conj_and_double()
                addition.apply_qk_gate_tr(gd, pos)
                if bwd is None:
                    bwd = addition
                else:
                    bwd.add(addition)
                    del addition
            elif kind == DIFF_OBSERVABLE:
                if not dens:
                    raise PanicException(
                        "The number of gradients wrt density matrices is less than required.")
                w = complex(np.asarray(dens.pop()).reshape(()))
                if w.imag != 0.0:
                    raise PanicException("Pauli coefficients must be real.")
                if bwd is None:
                    bwd = QuantizedTensor(fwd.qubits_number, fwd._precision)
                    pauli_inject(fwd, bwd, pos, w.real, accumulate=False)
                else:
                    pauli_inject(fwd, bwd, pos, w.real, accumulate=True)
            elif kind in (DIFF_OVERLAP, DIFF_FIDELITY):
                if not dens:
                    raise PanicException(
                        "The number of gradients wrt density matrices is less than required.")
                g = complex(np.asarray(dens.pop()).reshape(()))
                target, obs = pos
                if kind == DIFF_FIDELITY:  # F = |o|^2: g = 2 w o, o recomputed on the uncomputed fwd
                    if g.imag != 0.0:
                        raise PanicException("Pauli coefficients must be real.")
                    g = 2.0 * g.real * self._overlap(target, obs, fwd)
                first = bwd is None
                if first:
                    bwd = QuantizedTensor(fwd.qubits_number, fwd._precision)
                overlap_inject(target, bwd, g, obs, accumulate=not first)
        if cg:
            raise PanicException("Number of constant gates is more than required.")
        if vg:  # circuit.rs:426 words it this way
            raise PanicException("Number of constant gates is more than required.")
        if dens:
            raise PanicException("Number of gradients wrt density matrices is more than required.")
        self.bwd = bwd
        return list(grads)

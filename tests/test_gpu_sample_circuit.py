"""Sampling inside a circuit (DenseCircuit.get_sample_op, dense_circuit.py, over
QuantizedTensor.sample) and in examples/qaoa_pauli.py --shots."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
N = 6


def build(prec, with_sample):
    from quantum_differentiable_circuit import PauliSum
    from quantum_differentiable_circuit.dense_circuit import DenseCircuit
    c = DenseCircuit(N, prec)
    cost = PauliSum(N, [(1.0, f"Z{i} Z{(i + 1) % N}") for i in range(N)])
    for q in range(N):
        c.add_var_pauli_rotation(f"X{q}")
    c.add_var_gate([4, 1])
    c.get_observable_op_with_grad(PauliSum(N, [(0.5, "Z0 Z3"), (-1.0, "X2")]))
    c.add_var_pauli_evolution(cost)
    if with_sample:
        c.get_sample_op(5000, seed=3)
    c.add_var_pauli_rotation("Y1 Z5")
    c.get_dens_op_with_grad([2, 0])
    return c


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_sample_op_in_a_circuit(prec):
    """Rotations, a dense gate, a cost layer and get_sample_op(5000, seed=3) between two
    observables: run returns the sample at its place, equal to state.sample by hand with the
    same seed, the same on every run; forward and backward give, bit for bit, the outputs and
    gradients of the circuit without the sample op."""
    import quantum_differentiable_circuit as q
    rng = np.random.default_rng(21)
    dt = np.complex64 if prec == "f32" else np.complex128
    var = [float(a) for a in rng.uniform(-2, 2, N)]
    var += [O.haar_unitary(rng, 4).astype(dt).reshape(-1), 0.7, -0.4]
    c, plain = build(prec, True), build(prec, False)
    out = c.run([], var)
    assert len(out) == 3
    energy, sample, dens = out
    assert isinstance(energy, float) and dens.shape == (4, 4)
    assert sample.dtype == np.uint64 and sample.shape == (5000,) and np.all(sample < (1 << N))
    assert len(np.unique(sample)) > 8
    # by hand: the state at the sample's place
    s = q.QuantizedTensor.new_standard(N, prec)
    for k in range(N):
        s.apply_pauli_rotation(f"X{k}", var[k])
    s.apply_qk_gate(var[N], [4, 1])
    cost = q.PauliSum(N, [(1.0, f"Z{i} Z{(i + 1) % N}") for i in range(N)])
    s.apply_pauli_layer(cost.zmasks, var[N + 1] * cost.coeffs)
    assert np.array_equal(sample, s.sample(5000, seed=3))
    again = c.run([], var)
    assert np.array_equal(again[1], sample) and again[0] == energy
    assert np.array_equal(again[2], dens)
    # forward / backward skip it
    f1, f0 = c.forward([], var), plain.forward([], var)
    assert len(f1) == len(f0) == 2 and f1[0] == f0[0] == energy
    assert np.array_equal(f1[1], f0[1]) and np.array_equal(f1[1], dens)
    cot = [0.8, (rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))).astype(dt)]
    g1, g0 = c.backward(cot, [], var), plain.backward(cot, [], var)
    assert len(g1) == len(g0) == len(var)
    for a, b in zip(g1, g0):
        assert type(a) is type(b) and np.array_equal(a, b)
    assert any(np.any(np.asarray(a) != 0) for a in g1)
    assert np.array_equal(c.state.get_cpu_state_copy(), plain.state.get_cpu_state_copy())
    # a marginal sample; its panics when the circuit is built
    c.get_sample_op(100, seed=3, qubits=[5, 0])
    m = c.run([], var)[-1]
    assert m.shape == (100,) and np.all(m < 4)
    for qs in ([0, 0], [N]):
        with pytest.raises(q.PanicException, match="pos is out of the bound."):
            c.get_sample_op(10, qubits=qs)


def test_qaoa_example_samples():
    """examples/qaoa_pauli.py --shots in a child process: five bitstring lines whose counts are
    at most the shots, the sample mean of -sum ZZ within 6 standard errors of its expectation
    (|cost| <= n per shot)."""
    n, shots = 8, 2000
    r = subprocess.run([sys.executable, str(ROOT / "examples" / "qaoa_pauli.py"), "--qubits", str(n),
                        "--layers", "2", "--iters", "3", "--shots", str(shots)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = re.findall(r"^Sampled ([01]{%d}): (\d+) of %d$" % (n, shots), r.stdout, re.M)
    assert len(lines) == 5, r.stdout
    counts = [int(c) for _, c in lines]
    assert counts == sorted(counts, reverse=True) and 0 < sum(counts) <= shots
    mean = float(re.search(r"^Sample mean of -sum ZZ: (\S+)$", r.stdout, re.M).group(1))
    want = float(re.search(r"^Expectation of -sum ZZ: (\S+)$", r.stdout, re.M).group(1))
    assert -n <= want <= n and abs(mean - want) <= 6.0 * n / np.sqrt(shots)
    assert "Found energy" in r.stdout

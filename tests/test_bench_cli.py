"""bench.py's command line: a plain run times its steps and nothing else (what takes runs of its
own sits behind --full), and --dump-outputs writes what the last timed step returned.

The host-side checks need no GPU; the end-to-end case runs the benchmark itself, at a size where
a step takes milliseconds (n = 10, 2 layers: the single-gate and small fused kernels)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as O

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def _complex(a):
    return a[:, 0] + 1j * a[:, 1]


def test_plain_run_is_the_default():
    args = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.steps, args.warmup) == (7, 2)
    assert not args.full and args.dump_outputs is None
    assert bench.parse(["--full"]).full
    assert bench.parse(["--dump-outputs", "x"]).dump_outputs == "x"


@pytest.mark.parametrize("dt,real", [(np.complex64, np.float32), (np.complex128, np.float64)])
def test_dump_outputs_layout(tmp_path, dt, real):
    """Matrices of different sizes, row-major one after the other, (re, im) columns, in the
    real type of the precision; an existing directory is reused."""
    rng = np.random.default_rng(3)

    def rand(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dt)

    dens = [rand(2, 2), rand(4, 4)]
    grads = [rand(2, 2), rand(4), rand(4, 4).T]  # a diagonal; a non-contiguous view
    for _ in range(2):
        bench.dump_outputs(tmp_path / "a" / "b", dens, grads)
    for name, arrs in (("densities", dens), ("gradients", grads)):
        got = np.load(tmp_path / "a" / "b" / f"{name}.npy")
        want = np.concatenate([np.array(a).reshape(-1) for a in arrs])
        assert got.dtype == real and got.shape == (want.size, 2)
        assert np.array_equal(_complex(got), want)


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last(tmp_path):
    """bench.py --steps 3 on a small C2 circuit: the line holds the headline's fields, 3 timed
    steps with value = gates / ms_per_step, and null for every block that --full measures; the
    dumped densities and gradients are those of the oracle on the same seeded circuit.  Bound
    1e-5, the suite's f32 tolerance for single primitives: an amplitude passes 6 gates in 2
    layers, so the rounding is a few 6e-8 steps (smoke() measures 1e-7 .. 3e-7 here)."""
    n, layers = 10, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--qubits", str(n), "--layers", str(layers),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "gate-applications/sec (fwd+bwd) at n qubits"
    assert line["unit"] == "gate-applications/s" and line["higher_is_better"] is True
    assert line["dtype"] == "c64 (f32)" and line["steps"] == 3 and line["ms_per_step"] > 0
    gates = line["config"]["gates_per_step"]
    assert line["value"] == pytest.approx(gates / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("micro_min", "gate_kernels", "dense_gate_kernels", "vqse_c3", "vqse_c3_f32",
              "abi_unfused", "cpu_baseline"):
        assert line[k] is None, k

    wl = bench.WORKLOADS["c2"]
    ins, var = O.layered_circuit(n, layers, wl["seed"])
    assert len(var) == gates
    vg = [np.ascontiguousarray(g, dtype=np.complex64) for g in var]
    o = O.OracleCircuit(n, np.complex128)
    for kind, pos in ins:
        o.add(kind, *pos)
    vg128 = [g.astype(np.complex128) for g in vg]
    dens = o.forward([], vg128)
    grads = o.backward(bench.sigma_z_cotangents(len(dens), np.complex128), [], vg128)
    for name, want in (("densities", dens), ("gradients", grads)):
        got = np.load(out / f"{name}.npy")
        want = np.concatenate([np.asarray(a).reshape(-1) for a in want])
        assert got.dtype == np.float32 and got.shape == (want.size, 2)
        err = np.abs(_complex(got) - want).max() / np.abs(want).max()
        print(f"[bench dump] {name}: {want.size} elements, max error {err:.2e}")
        assert err < 1e-5, (name, err)

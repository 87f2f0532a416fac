#!/usr/bin/env python3
"""Gradient and density kernels of dense k-qubit gates (csrc/qdc_qkgrad.hpp): GB/s and fraction
of 8 TB/s of grad_qk{3,4,5} and density_qk{3,4,5} at n = 28 (f32) and n = 27 (f64), with the
yardsticks of the same library in the same run: grad_q2 / density_q2 (same traffic, VALU path)
and qk{3,4,5} (same k, MFMA path).  Two placement classes, each its own profiled session:
"mixed" = bench.py's dense_gate_sample placements (8 random per k; the q2 yardsticks on their
first two qubits), "low" = targets 1..k (q2: 2, 1).  Per-launch HIP events on the primitives'
stream; one warm-up pass, then REPS timed passes (timing probe)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "differentiable-quantum-circuit-cuda_amd")]
import quantum_differentiable_circuit as q  # noqa: E402
from quantum_differentiable_circuit.workloads import haar_unitary  # noqa: E402

HBM_PEAK_GBS = 8000.0
REPS = 3
NAMES = [f"{p}_qk{k}" for k in (3, 4, 5) for p in ("grad", "density")] + \
        ["qk3", "qk4", "qk5", "grad_q2", "density_q2"]


def session(prec, fwd, bwd, poss, mats):
    def one_pass():
        for k in (3, 4, 5):
            for pos, u in zip(poss[k], mats[k]):
                q.get_qk_grad(fwd, bwd, pos)
                fwd.get_qk_density(pos)
                q.get_q2_grad(fwd, bwd, pos[0], pos[1])
                fwd.get_q2_density(pos[0], pos[1])
                bwd.apply_qk_gate(u, pos)
    one_pass()  # warm-up (scratch allocation, clocks, caches)
    q.primitives_sync(prec)
    q.primitives_profile(True, prec)
    for _ in range(REPS):
        one_pass()
    stats = q.primitives_profile_collect(prec)
    q.primitives_profile(False, prec)
    out = {}
    for name in NAMES:
        s = stats.get(name)
        if s and s["total_ms"] > 0:
            gbs = s["algo_bytes"] / (s["total_ms"] * 1e-3) / 1e9
            out[name] = {"GB/s": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
                         "TFLOP/s": round(s["algo_flops"] / (s["total_ms"] * 1e-3) / 1e12, 2),
                         "launches": s["launches"],
                         "avg_ms": round(s["total_ms"] / s["launches"], 4)}
    return out


def main():
    info = q._native.load("f32").qdc_build_info().decode()
    print("# library:", info, flush=True)
    for prec, n in (("f32", 28), ("f64", 27)):
        dt = np.complex64 if prec == "f32" else np.complex128
        rng = np.random.default_rng(2)  # bench.py dense_gate_sample's stream
        mats = {k: [np.ascontiguousarray(haar_unitary(rng, 1 << k), dtype=dt) for _ in range(8)]
                for k in (3, 4, 5)}
        mixed = {k: [[int(p) for p in rng.permutation(n)[:k]] for _ in range(8)]
                 for k in (3, 4, 5)}
        low = {k: [list(range(k, 0, -1))] * 2 for k in (3, 4, 5)}
        fwd = q.QuantizedTensor.new_standard(n, precision=prec)
        h = (np.array([[1, 1], [1, -1]]) / np.sqrt(2)).astype(dt).reshape(-1)
        for p in range(n):  # every amplitude nonzero
            fwd.apply_q1_gate(h, p)
        bwd = fwd.clone()
        for cls, poss in (("mixed", mixed), ("low", low)):
            res = session(prec, fwd, bwd, poss, mats)
            print(json.dumps({"precision": prec, "n": n, "placements": cls, "kernels": res}),
                  flush=True)
            g2, d2 = res["grad_q2"]["GB/s"], res["density_q2"]["GB/s"]
            print(f"# {prec} n={n} {cls}: kernel GB/s frac-of-8TB/s x(q2 yardstick) x(qk same k)")
            for k in (3, 4, 5):
                for p, y in (("grad", g2), ("density", d2)):
                    r = res[f"{p}_qk{k}"]
                    print(f"#   {p}_qk{k:<2} {r['GB/s']:8.1f} {r['frac']:.3f} "
                          f"{r['GB/s'] / y:5.2f} {r['GB/s'] / res[f'qk{k}']['GB/s']:5.2f}")
            print(f"#   grad_q2 {g2:.1f} density_q2 {d2:.1f} " +
                  " ".join(f"qk{k} {res[f'qk{k}']['GB/s']:.1f}" for k in (3, 4, 5)), flush=True)
        del fwd, bwd


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of sampling (QuantizedTensor.sample: k_sample_sums, k_sample_locate) and the
host time of the step between the two passes.

At n = 28 in f32 and n = 27 in f64 (one state: 2 GiB), on the primitives' stream with per-launch
events (primitives_profile), one warm-up and then `--reps` timed calls per row, for 10^3 and 10^6
shots on the uniform superposition (the shots spread over every segment) and on a basis state
(every shot in one segment, one block doing all the searches):

  (a) per kernel: device ms, algorithmic bytes (pass A: the state; pass B: hit segments x 2^G
      amplitudes, against its bound, the state) and bytes over time as a fraction of 8 TB/s;
  (b) the yardstick of pass A, in the same process and run: the device ms of
      state.pauli_energy(PauliSum(n, [(1.0, "Z0")])), the one-pass read-only reduction over the
      same bytes, and the ratio of the two;
  (c) host ms of sample_assign on the same segment sums and uniforms, and the whole call (a host
      clock around sample(), which ends in a stream synchronisation).

Then, at n = 24, the whole call against the route it replaces: get_cpu_state_copy() and numpy's
cumsum and searchsorted on the host (median of `--reps` runs each).

usage: sample_probe.py [--precision both] [--qubits N] [--reps 3]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "differentiable-quantum-circuit-cuda_amd")]

HBM = 8e12  # bytes / s


def timed(q, prec, reps, fn):
    """{kernel name: (ms per call, launches per call, bytes per call)} of fn over `reps` calls
    after one warm-up."""
    fn()
    q.primitives_profile(True, prec)
    try:
        for _ in range(reps):
            fn()
        stats = q.primitives_profile_collect(prec)
    finally:
        q.primitives_profile(False, prec)
    return {k: (s["total_ms"] / reps, s["launches"] / reps, s["algo_bytes"] / reps)
            for k, s in stats.items()}


def wall_ms(reps, fn):
    """median host ms of fn (which must end in a synchronisation)"""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def states(q, prec, n):
    dt = np.complex64 if prec == "f32" else np.complex128
    uni = q.QuantizedTensor.new_standard(n, precision=prec)
    had = (np.array([1, 1, 1, -1]) / np.sqrt(2)).astype(dt)
    for p in range(n):
        uni.apply_q1_gate(had, p)
    yield "uniform", uni
    del uni
    yield "basis", q.QuantizedTensor.new_standard(n, precision=prec)


def probe(q, prec, n, reps):
    plan = q.sample_plan(n, prec)
    segs, seg_amps = plan["segments"], 1 << min(plan["G"], n)
    item = 8 if prec == "f32" else 16
    s = float(item) * 2.0 ** n
    print(f"# n = {n} {prec}, state S = {s / 2 ** 30:.2f} GiB, G = {plan['G']}, {segs} segments, "
          f"{reps} timed calls after one warm-up, fractions of {HBM / 1e12:.0f} TB/s")
    print(f"{'state':8s} {'shots':>8s} | {'sums ms':>8s} {'of 8TB/s':>8s} {'Z0 ms':>8s} {'ratio':>6s} | "
          f"{'locate ms':>9s} {'blocks':>6s} {'read MiB':>9s} {'of S':>7s} {'of 8TB/s':>8s} | "
          f"{'assign ms':>9s} {'call ms':>8s}")
    obs = q.PauliSum(n, [(1.0, "Z0")])
    for label, t in states(q, prec, n):
        for shots in (1000, 1_000_000):
            u = np.random.default_rng(9).random(shots)
            st = timed(q, prec, reps, lambda: t.sample(shots, uniforms=u))
            a_ms = st["sample_sums"][0]
            b_ms, _, b_bytes = st["sample_locate"]
            en = timed(q, prec, reps, lambda: t.pauli_energy(obs))
            z_ms = sum(ms for ms, _, _ in en.values())  # with its finalize
            sums = np.full(segs, seg_amps / 2.0 ** n) if label == "uniform" else \
                np.concatenate([[1.0], np.zeros(segs - 1)])
            h_ms = wall_ms(reps, lambda: q.sample_assign(sums, u, prec))
            c_ms = wall_ms(reps, lambda: t.sample(shots, uniforms=u))
            print(f"{label:8s} {shots:8d} | {a_ms:8.3f} {s / (a_ms * 1e-3) / HBM:8.3f} {z_ms:8.3f} "
                  f"{a_ms / z_ms:6.2f} | {b_ms:9.3f} {b_bytes / (seg_amps * item):6.0f} "
                  f"{b_bytes / 2 ** 20:9.1f} {b_bytes / s:7.4f} {b_bytes / (b_ms * 1e-3) / HBM:8.4f} | "
                  f"{h_ms:9.3f} {c_ms:8.3f}", flush=True)
        del t


def end_to_end(q, prec, n, reps):
    """sample() against copy-to-host + cumsum + searchsorted, the uniform state"""
    for label, t in states(q, prec, n):
        if label != "uniform":
            continue
        for shots in (1000, 1_000_000):
            u = np.random.default_rng(9).random(shots)
            t.sample(shots, uniforms=u)

            def host_route():
                psi = t.get_cpu_state_copy()
                c = np.cumsum(psi.real.astype(np.float64) ** 2 + psi.imag.astype(np.float64) ** 2)
                return np.searchsorted(c, u * c[-1], side="right")

            dev = wall_ms(reps, lambda: t.sample(shots, uniforms=u))
            host = wall_ms(reps, host_route)
            print(f"end to end n = {n} {prec} {shots:8d} shots: sample() {dev:9.3f} ms, copy + cumsum + "
                  f"searchsorted {host:9.3f} ms, ratio {host / dev:7.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--precision", choices=["f32", "f64", "both"], default="both")
    ap.add_argument("--qubits", type=int, default=0, help="default: 28 (f32) / 27 (f64)")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import quantum_differentiable_circuit as q
    precs = ["f32", "f64"] if a.precision == "both" else [a.precision]
    for prec in precs:
        probe(q, prec, a.qubits or (28 if prec == "f32" else 27), a.reps)
    for prec in precs:
        end_to_end(q, prec, 24, a.reps)


if __name__ == "__main__":
    main()

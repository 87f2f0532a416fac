"""The Gamma cap of two-state register-resident passes as a value (QDC_RQ_GCAP in the runtime,
QDC_SCHED_GCAP in the qdc_fusion_schedule hook; storage bound FMAX_GRAD_RQ = 32), on CPU.

1. With the hook's cap at 24 and 32 (48 / 64 gates per pass) the schedules keep the invariants of
   tests/test_fusion_schedule.py in both directions, mirrored forwards reverse into valid
   sweeps, and no pass exceeds the cap in Gamma stages or 64 gates.
2. A layered circuit at n = 12 scheduled at cap 32 — with a pass of more than 16 Gamma stages —
   replayed with the oracle's primitives equals the sequential oracle.
3. What the cap is worth on C2 and C4, and that the hook's defaults are still the schedules of
   tests/golden/fusion_search_parent.json.
4. The largest C2 reverse pass of more than 16 Gamma stages and its forward mirror compile for
   gfx950 within the resources tests/test_spec_cpu.py asks of their kinds.
"""
import json
import os
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_fusion_schedule import DENS, T, check_invariants, mirrored, replay  # noqa: E402
from test_fusion_search_cpu import (GOLDEN, case_id, circuit, digest, gamma_stages,  # noqa: E402
                                    gate_passes, precisions)
from test_fusion_search_cpu import run as run_default  # noqa: E402

from oracle import oracle as O  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "differentiable-quantum-circuit-cuda_amd"
ENV = ("QDC_FUSE_SEARCH", "QDC_SCHED_RQ", "QDC_SCHED_MIRROR", "QDC_SCHED_GCAP")
CAPS = (24, 32)
CIRCUITS = ("c2", "c4", "make_14_1", "make_17_2", "make_24_3")


def run(name, mode, mir, cap, prec="f32"):
    """One schedule of the hook with the runtime's register-resident settings, the search on,
    Gamma cap `cap` and 2 * cap gates per pass (the environment restored afterwards)."""
    import quantum_differentiable_circuit as q
    n, ins, sens = circuit(name)
    old = {k: os.environ.get(k) for k in ENV}
    os.environ.update(QDC_FUSE_SEARCH="1", QDC_SCHED_RQ="1", QDC_SCHED_MIRROR=mir,
                      QDC_SCHED_GCAP=str(cap))
    try:
        ops, items = q.fusion_schedule(n, [(k, *p) for k, p in ins], mode, fwd_sens=sens,
                                       precision=prec, max_ops=2 * cap)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return n, ins, sens, ops, items


def within_caps(ins, ops, items, cap):
    for it in items:
        if it["type"] == 2:
            assert gamma_stages(ins, ops, it) <= cap
            assert sum(len(st) for st in it["stages"]) <= 64


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("mir", ["0", "1"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("c", CIRCUITS)
def test_invariants_at_higher_caps(c, mode, mir, cap):
    for prec in precisions(c):
        n, ins, sens, ops, items = run(c, mode, mir, cap, prec)
        two = mode == 2 or mir == "1"
        check_invariants(n, ins, sens, mode, prec, ops, items, permuted=True,
                         tbits=T[2] if two else None)
        if two:
            within_caps(ins, ops, items, cap)
        if mir == "1" and mode == 1:
            ops_b, items_b = mirrored(ops, items, ins)
            check_invariants(n, ins, sens, 2, prec, ops_b, items_b, permuted=True, tbits=T[2])
            within_caps(ins, ops_b, items_b, cap)
            for it in items:
                if it["type"] == 2:
                    meas = [ins[ops[st[0]]["instr"]][0] in DENS for st in it["stages"]]
                    assert meas == sorted(meas)  # gate stages, then densities


@pytest.mark.parametrize("mirror", ["0", "1"])
def test_replay_at_cap_32_matches_sequential_oracle(monkeypatch, mirror):
    """test_search_replay_matches_sequential_oracle's construction on a layered circuit at
    n = 12 (12 layers: the 11-bit two-state tile holds all but one qubit, so passes run to the
    cap) with the cap at 32; a pass of more than 16 Gamma stages must be among them."""
    import quantum_differentiable_circuit as q
    from quantum_differentiable_circuit import workloads as W
    monkeypatch.setenv("QDC_FUSE_SEARCH", "1")
    monkeypatch.setenv("QDC_SCHED_RQ", "1")
    monkeypatch.setenv("QDC_SCHED_MIRROR", mirror)
    monkeypatch.setenv("QDC_SCHED_GCAP", "32")
    n = 12
    ins, var = W.layered_circuit(n, 12, 5)
    var = [np.asarray(g, np.complex128) for g in var]
    gates = dict(zip([i for i, (k, _) in enumerate(ins) if k not in DENS], var))
    sens = [0] * len(ins)
    instr = [(k, *p) for k, p in ins]

    def sched(mode):
        return q.fusion_schedule(n, instr, mode, fwd_sens=sens, precision="f32", max_ops=64)

    ops, items = {}, {}
    ops["fwd"], items["fwd"] = sched(1)
    if mirror == "1":
        ops["bwd"], items["bwd"] = mirrored(ops["fwd"], items["fwd"], ins)
    else:
        ops["bwd"], items["bwd"] = sched(2)
    widest = max(gamma_stages(ins, ops["bwd"], it) for it in items["bwd"] if it["type"] == 2)
    print(f"mirror {mirror}: widest reverse pass {widest} Gamma stages")
    assert 16 < widest <= 32
    within_caps(ins, ops["bwd"], items["bwd"], 32)
    psi0 = O.random_state(np.random.default_rng(4), n)
    o = O.OracleCircuit(n)
    for k, p in ins:
        o.add(k, *p)
    o.set_state_from_vector(psi0)
    want_d = o.forward([], var)

    def cot_fn(d):
        return [c.conj() for c in O.tsallis_loss_and_cotangents(d)[1]]

    want_g = o.backward(cot_fn(want_d), [], var)
    got_d, got_g, final = replay(n, ins, ops, items, gates, psi0, cot_fn)
    assert len(got_d) == len(want_d) and len(got_g) == len(want_g)
    for a, b in zip(got_d, want_d):
        assert np.abs(a - b).max() < 1e-12
    ga, gb = np.concatenate(got_g), np.concatenate(want_g)
    assert np.abs(ga - gb).max() < 1e-11 * np.abs(gb).max()
    assert np.abs(final - o.state).max() < 1e-11


# gate passes (and stages) of the mirrored forward at cap 32 / 64 gates.  Recorded: C2 25 passes
# of 539 stages, C4 56 passes; two passes of margin for tie-breaks.
PASS_BOUNDS_32 = {"c2": (27, 542), "c4": (58, None)}


@pytest.mark.parametrize("c", list(PASS_BOUNDS_32))
def test_cap_32_saves_passes(c):
    bound, stage_bound = PASS_BOUNDS_32[c]
    _, ins, _, ops, items = run(c, 1, "1", 32)
    p, s = gate_passes(ins, ops, items)
    print(f"{c}: cap 32: {p} gate passes, {s} gate stages")
    assert p <= bound
    if stage_bound:
        assert s <= stage_bound
    assert max(gamma_stages(ins, ops, it) for it in items if it["type"] == 2) > 16


@pytest.mark.parametrize("c,mode,rq,mir", [("c2", 1, "1", "1"), ("c2", 2, "1", "0"),
                                           ("c4", 1, "1", "1"), ("make_17_2", 2, "1", "0")])
def test_hook_defaults_are_the_golden_schedules(monkeypatch, c, mode, rq, mir):
    """Without QDC_SCHED_GCAP and with max_ops = 0 the hook plans cap 16 and 32 gates: the scan's
    digests of tests/golden/fusion_search_parent.json, and passes of at most 16 Gamma stages
    with the search on."""
    monkeypatch.delenv("QDC_SCHED_GCAP", raising=False)
    golden = json.loads(GOLDEN.read_text())
    for prec in precisions(c):
        _, ins, _, ops, items = run_default(c, mode, rq, mir, "0", prec)
        want = golden[case_id(c, mode, rq, mir, prec)]
        assert [len(items), *gate_passes(ins, ops, items)] == want["counts"]
        assert digest(items) == want["sha256"]
        _, ins, _, ops, items = run_default(c, mode, rq, mir, "1", prec)
        for it in items:
            if it["type"] == 2:
                assert gamma_stages(ins, ops, it) <= 16
                assert sum(len(st) for st in it["stages"]) <= 32


def test_knob_rows():
    import quantum_differentiable_circuit as q
    for prec, cap in (("f32", "32"), ("f64", "16")):
        val = {r[0]: (r[1], r[3]) for r in q.knob_table(prec)}
        assert val["QDC_RQ_GCAP"] == ("Circuit", cap)
        assert val["QDC_FUSE_MAX_OPS"] == ("Circuit", str(2 * int(cap)))
        assert val["QDC_SCHED_GCAP"][0] == "Hook"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_largest_c2_passes_compile_within_their_kinds_resources(tmp_path):
    """The C2 step's specialized kernels as the runtime generates them (a dry run): the reverse
    pass with the most Gamma stages (more than 16: the instance with 32 accumulators) keeps the
    generic two-state kernel's budget — two waves per SIMD, <= 256 VGPRs, no scratch — on the
    half buffer plus 4 KiB of accumulators; its forward mirror, the one-state pass with the most
    stages, keeps its kind's (tests/test_spec_cpu.py test_spec_half_buffer_relayouts)."""
    dump = tmp_path / "dump"
    dump.mkdir()
    code = f"""
        import sys
        sys.path[:0] = [{str(ROOT)!r}, {str(PKG)!r}]
        import numpy as np
        import quantum_differentiable_circuit as q
        from quantum_differentiable_circuit import workloads as W
        ins, var = W.layered_circuit(28, 20, 24)
        cots = [np.diag([1.0, -1.0]).astype(np.complex64) for k, _ in ins if k == W.DIFF_Q1_DENSITY]
        q.precompile(28, [(k, *p) for k, p in ins], [], [np.ascontiguousarray(g, dtype=np.complex64)
                     for g in var], cots, world=1, precision="f32")
        """
    env = dict(os.environ, QDC_PRECOMPILE_DUMP=str(dump), QDC_PRECOMPILE_COUNT="1",
               QDC_JIT_DIR=str(tmp_path / "jit"))
    for k in [k for k in env if k.startswith("QDC_") and k not in
              ("QDC_PRECOMPILE_DUMP", "QDC_PRECOMPILE_COUNT", "QDC_JIT_DIR")]:
        del env[k]
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

    def largest(prefix, mark):
        best = max(dump.glob(prefix + "*.hip"), key=lambda f: f.read_text().count(mark))
        return best, best.read_text().count(mark)

    rev, ngamma = largest("qdc_spec_", "true, &E.accw[")
    fwd, nstage = largest("qdc_specf_", "false, nullptr);")
    print(f"largest reverse pass: {ngamma} Gamma stages; largest forward pass: {nstage} stages")
    assert 16 < ngamma <= 32 and nstage == ngamma
    assert "Prog, true, 32>" in rev.read_text() or "Prog, false, 32>" in rev.read_text()
    csrc, inc = PKG / "csrc", ROOT / "include"
    meta = {}
    for src in (rev, fwd):
        asm = tmp_path / (src.stem + ".s")
        c = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950",
                            f"-I{inc}", f"-I{csrc}", "-S", "--cuda-device-only", "-o", str(asm),
                            str(src)], capture_output=True, text=True)
        assert c.returncode == 0, c.stderr
        text = asm.read_text()
        m = text[text.index(".amdhsa_kernel " + src.stem):]
        meta[src] = {k: int(m.split(".amdhsa_" + k)[1].split()[0]) for k in
                     ("next_free_vgpr", "private_segment_fixed_size", "group_segment_fixed_size")}
        body = text[text.index(src.stem + ":"):text.index(".Lfunc_end0")]
        meta[src]["code_lines"] = body.count("\n")
        print(src.stem, meta[src])
    half = "Prog, true, 32>" in rev.read_text()
    assert meta[rev]["private_segment_fixed_size"] == 0
    assert meta[rev]["next_free_vgpr"] <= 256
    assert meta[rev]["group_segment_fixed_size"] == (8192 if half else 16384) + 4096
    # (the one-state half-buffer kind: 5 waves per SIMD, a few spilled registers)
    assert meta[fwd]["private_segment_fixed_size"] <= 128 and meta[fwd]["next_free_vgpr"] <= 102
    assert meta[fwd]["group_segment_fixed_size"] in (8192, 16384)

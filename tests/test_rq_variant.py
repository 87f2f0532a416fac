"""The register-resident kernel variants (csrc/qdc_variant.hpp) on CPU: the table of the kernels
the runtime can launch and the one selector that maps a pass (state count, tile size) and the
QDC_RW / QDC_RQ_PF / QDC_RQ_SLOTS5 / QDC_MIRROR knobs to a row.  emit_rq_pass plans and
specializes a pass from its row and launch_rq launches it with the row's block size, so a wrong
row is a kernel started with the wrong number of threads for its LDS and register layout: the
rows and the selection rules are written out here, independently of the code.  The hook
(qdc_rq_variant) builds a dry circuit, which reads the knobs from the environment like a real
one; every environment runs in a fresh process.  Parity of the variants on the GPU:
tests/test_gpu_fusion.py (RQ_VARIANTS)."""
import itertools
import re

import pytest

from test_spec_cpu import _run

# kernel -> (two-state, tile bits, block threads, register slots, dynamic tail allowed,
#            specialized pass, has a half-buffer form, specialized grid from its own occupancy)
F32_ROWS = {
    "k_rw<true, 2, false, 1, true>":
        (True, 11, 64, 5, True, "qdc::rw_pass<true, 2, false, 1, true, Prog>", True, True),
    "k_rw<true, 2, false, 1>": (True, 11, 64, 4, True, "", False, False),
    "k_rw<true, 2, true, 1>": (True, 11, 64, 4, False, "", False, False),
    "k_rq<true, 128, false>": (True, 11, 128, 4, False, "", False, False),
    "k_rw<false, 2, false, 1, true>":
        (False, 11, 64, 5, True, "qdc::rw_pass<false, 2, false, 1, true, Prog>", True, True),
    "k_rw<false, 2, true, 1, true>":
        (False, 11, 64, 5, True, "qdc::rw_pass<false, 2, true, 1, true, Prog>", False, False),
    "k_rw<false, 2, false, 1>": (False, 11, 64, 4, True, "", False, False),
    "k_rq<false, 128, true>": (False, 11, 128, 4, True, "", False, False),
    "k_rq<false, 128, false>": (False, 11, 128, 4, False, "", False, False),
    "k_rw<false, 2, false, 2>": (False, 12, 128, 4, False, "", False, False),
    "k_rq<false, 256, true>":
        (False, 12, 256, 4, True, "qdc::rq_pass<false, 256, true, Prog>", False, False),
    "k_rq<false, 256, false>": (False, 12, 256, 4, False, "", False, False),
}
F64_ROWS = {
    "k_rw<true, 1, false, 1>":
        (True, 10, 64, 4, True, "qdc::rw_pass<true, 1, false, 1, false, Prog>", False, False),
    "k_rw<false, 1, false, 1>":
        (False, 10, 64, 4, True, "qdc::rw_pass<false, 1, false, 1, false, Prog>", False, False),
    "k_rw<false, 1, false, 2>":
        (False, 11, 128, 4, False, "qdc::rw_pass<false, 1, false, 2, false, Prog>", False, False),
}
# (two-state, tile bits) asked of each precision: every supported pair, and tiles no kernel runs
PAIRS = {"f32": [(1, 11), (0, 11), (0, 12), (1, 12), (0, 10), (1, 10), (0, 13)],
         "f64": [(1, 10), (0, 10), (0, 11), (1, 11), (0, 12), (0, 9)]}


def expected_f32(two, tile, rw, pf, s5, mirror):
    """today's rules; None: refused"""
    w0, w1, w2, w3 = rw & 1, rw & 2, rw & 4, rw & 8
    if two and tile == 11:
        if not w0:
            return "k_rq<true, 128, false>"
        if w2:
            return "k_rw<true, 2, true, 1>"
        return "k_rw<true, 2, false, 1, true>" if s5 else "k_rw<true, 2, false, 1>"
    if not two and tile == 11:
        if w1 or mirror:
            if s5:
                return "k_rw<false, 2, true, 1, true>" if w3 and pf else "k_rw<false, 2, false, 1, true>"
            return "k_rw<false, 2, false, 1>"
        return "k_rq<false, 128, true>" if pf else "k_rq<false, 128, false>"
    if not two and tile == 12:
        if w1:
            return "k_rw<false, 2, false, 2>"
        return "k_rq<false, 256, true>" if pf else "k_rq<false, 256, false>"
    return None


def expected_f64(two, tile):
    return {(1, 10): "k_rw<true, 1, false, 1>", (0, 10): "k_rw<false, 1, false, 1>",
            (0, 11): "k_rw<false, 1, false, 2>"}.get((two, tile))


QUERY = f"""
    import quantum_differentiable_circuit as q
    out = {{}}
    for prec, pairs in {PAIRS!r}.items():
        for two, tile in pairs:
            try:
                out[f"{{prec}} {{two}} {{tile}}"] = q.rq_variant(two, tile, precision=prec)
            except RuntimeError as e:
                out[f"{{prec}} {{two}} {{tile}}"] = "refused: " + str(e)
    print(json.dumps(out))
    """


def query(env):
    out, _ = _run(QUERY, {k: str(v) for k, v in env.items()})
    return out


def check_row(got, rows, kernel, what, spec_half=True):
    two, tile, threads, slots, dyn, spec, half, own = rows[kernel]
    assert got["kernel"] == kernel, what
    assert (got["threads"], got["slots"], got["dyn"]) == (threads, slots, dyn), (what, got)
    assert got["spec"] == spec and got["own_grid"] == own, (what, got)
    assert got["spec_half"] == (spec.replace("Prog>", "Prog, true>") if half else ""), (what, got)
    # the five-slot rows (all on 2^11 tiles) are planned for half buffers when QDC_SPEC_HALF is on
    assert got["keep"] == (spec_half and slots == 5), (what, got)


def test_rows_are_launchable():
    """Each row's block size is what its kernel defines for the row's tile: 16 amplitudes per
    lane and register group, so k_rq<TWO, NT, PF> runs NT = 2^tile / 16 threads and k_rw<TWO,
    NE, PF, W[, S5]>, whose lanes hold NE register groups, 64 W = 2^tile / 16 / NE; five slots
    only where the kernel takes them (the S5 argument)."""
    for rows in (F32_ROWS, F64_ROWS):
        for kernel, (two, tile, threads, slots, dyn, spec, half, own) in rows.items():
            name, args = re.fullmatch(r"(k_r[qw])<(.*)>", kernel).groups()
            args = [a.strip() for a in args.split(",")]
            assert args[0] == ("true" if two else "false"), kernel
            if name == "k_rq":
                assert threads == int(args[1]) == (1 << tile) // 16, kernel
                assert slots == 4
            else:
                ne, w = int(args[1]), int(args[3])
                assert threads == 64 * w == (1 << tile) // 16 // ne, kernel
                assert slots == (5 if len(args) > 4 and args[4] == "true" else 4), kernel
            if spec:  # the specialized pass is the same instance (S5 spelled out) with the program
                a = args + (["false"] if name == "k_rw" and len(args) == 4 else [])
                assert spec == f"qdc::{name[2:]}_pass<{', '.join(a)}, Prog>", kernel
            assert not (own or half) or spec, kernel


@pytest.mark.parametrize("rw", [0, 1, 2, 3, 5, 9, 11])
def test_selected_variant(rw):
    """QDC_RW x QDC_RQ_PF x QDC_RQ_SLOTS5 x QDC_MIRROR, every supported (state, tile) pair in both
    precisions: the selected row is the one today's rules name, with the table's columns; tiles no
    kernel runs (two-state 2^12 in f32 among them) are refused with the launch's message."""
    for pf, s5, mirror in itertools.product((0, 1), repeat=3):
        got = query({"QDC_RW": rw, "QDC_RQ_PF": pf, "QDC_RQ_SLOTS5": s5, "QDC_MIRROR": mirror})
        for prec, pairs in PAIRS.items():
            for two, tile in pairs:
                what = f"{prec} two={two} tile={tile} RW={rw} PF={pf} S5={s5} MIRROR={mirror}"
                g = got[f"{prec} {two} {tile}"]
                want = expected_f32(two, tile, rw, pf, s5, mirror) if prec == "f32" \
                    else expected_f64(two, tile)
                if want is None:
                    assert g == (f"refused: no register-resident kernel for a {1 << tile}-amplitude "
                                 f"{'two' if two else 'one'}-state tile"), what
                else:
                    assert not isinstance(g, str), (what, g)
                    check_row(g, F32_ROWS if prec == "f32" else F64_ROWS, want, what)
    assert expected_f32(1, 12, rw, 1, 1, 1) is None  # (two-state 2^12: refused above)


def test_defaults_and_half_buffer_planning():
    """With no knob set: the benchmark's kernels.  QDC_SPEC_HALF=0: no pass is planned for half
    buffers."""
    got = query({})
    check_row(got["f32 1 11"], F32_ROWS, "k_rw<true, 2, false, 1, true>", "default reverse")
    check_row(got["f32 0 11"], F32_ROWS, "k_rw<false, 2, false, 1, true>", "default mirrored forward")
    check_row(got["f32 0 12"], F32_ROWS, "k_rq<false, 256, true>", "default 2^12 forward")
    got = query({"QDC_SPEC_HALF": 0})
    check_row(got["f32 1 11"], F32_ROWS, "k_rw<true, 2, false, 1, true>", "no half", spec_half=False)
    check_row(got["f32 0 11"], F32_ROWS, "k_rw<false, 2, false, 1, true>", "no half", spec_half=False)

"""The QDC_* runtime knobs (csrc/qdc_knobs.hpp) on CPU: the table, the code that reads it and
INTEGRATION.md §7 say the same.  qdc_knob_table reports each Context / Circuit row with the value
a default-constructed Ctx::Knobs / Circuit::Knobs holds after read() under the current
environment (no device), so a default, a name or a clamp that drifts from its row shows here.
A new knob is a row, a typed read and a doc row; one of the tests below fails otherwise."""
import os
import re
from pathlib import Path

import pytest

import quantum_differentiable_circuit as q

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "differentiable-quantum-circuit-cuda_amd" / "csrc"
SCOPES = ("Process", "Context", "Circuit", "Call", "Hook")
PRECISIONS = ("f32", "f64")

# The value a knob is set to when the rule "0 where the default is non-zero, 1 where it is 0"
# gives no legal value: the other legal tile size, and a granule that is a power of two.
OTHER = {"QDC_TILE1_CHUNKS": "1024", "QDC_DYN_GRAN": "2"}
# What read() makes of that value where it clamps (qdc_device.hpp, qdc_circuit.hpp): grids and
# pass sizes are at least 1, the interleave block at least 2^4 chunks.
CLAMPED = {"QDC_GRID_CAP": 1, "QDC_RED_CAP": 1, "QDC_REV_RED": 1, "QDC_DIAG_RED": 1,
           "QDC_FUSE_MAX_OPS": 1, "QDC_FUSE_LCMIN": 1, "QDC_STATE_ILV_BITS": 4}


def as_int(text):
    """The value of an integer literal (decimal or 0x...), else None."""
    try:
        return int(text, 0)
    except ValueError:
        return None


@pytest.fixture
def clean_env(monkeypatch):
    for name in [n for n in os.environ if n.startswith("QDC_")]:
        monkeypatch.delenv(name)
    return monkeypatch


def valued_rows(table):
    """The Context / Circuit rows whose default text is an integer literal."""
    return [r for r in table if r[1] in ("Context", "Circuit") and as_int(r[2]) is not None]


@pytest.mark.parametrize("prec", PRECISIONS)
def test_table_shape(prec):
    table = q.knob_table(prec)
    assert all(len(r) == 5 for r in table)
    names = [r[0] for r in table]
    assert len(set(names)) == len(names)
    assert all(re.fullmatch(r"QDC_[A-Z0-9_]+", n) for n in names)
    assert all(r[1] in SCOPES for r in table)
    assert {r[1] for r in table} == set(SCOPES)
    assert all(r[2] and r[4] for r in table)
    # a value for the two scopes with state, none for the others
    assert all(bool(r[3]) == (r[1] in ("Context", "Circuit")) for r in table)


def test_tables_of_both_precisions_agree():
    a, b = (q.knob_table(p) for p in PRECISIONS)
    assert [(r[0], r[1], r[2], r[4]) for r in a] == [(r[0], r[1], r[2], r[4]) for r in b]


@pytest.mark.parametrize("prec", PRECISIONS)
def test_default_matches_code(clean_env, prec):
    rows = valued_rows(q.knob_table(prec))
    assert len(rows) >= 50
    wrong = [(r[0], r[2], r[3]) for r in rows if as_int(r[3]) != as_int(r[2])]
    assert not wrong, f"(knob, default in the table, value the code holds): {wrong}"
    # the one default that depends on the precision
    val = {r[0]: r[3] for r in q.knob_table(prec)}
    assert val["QDC_SPEC_ASYNC"] == ("1" if prec == "f32" else "0")
    assert val["QDC_LANE_U"] == "8,1,4"


@pytest.mark.parametrize("prec", PRECISIONS)
def test_each_knob_is_wired_to_its_own_name(clean_env, prec):
    base = {r[0]: r[3] for r in q.knob_table(prec)}
    for name, _, dflt, _, _ in valued_rows(q.knob_table(prec)):
        text = OTHER.get(name, "0" if as_int(dflt) != 0 else "1")
        want = CLAMPED.get(name, int(text))
        assert want != as_int(dflt), name
        with clean_env.context() as m:
            m.setenv(name, text)
            got = {r[0]: r[3] for r in q.knob_table(prec)}
        assert as_int(got[name]) == want, (name, text, got[name])
        others = {n: (base[n], got[n]) for n in base if n != name and got[n] != base[n]}
        assert not others, (name, others)
    assert {r[0]: r[3] for r in q.knob_table(prec)} == base


def test_invalid_tile_is_refused(clean_env):
    """QDC_TILE1_CHUNKS keeps its validation: no value is reported for a circuit that would not
    be created (the Context rows are unaffected)."""
    clean_env.setenv("QDC_TILE1_CHUNKS", "512")
    for r in q.knob_table("f32"):
        assert bool(r[3]) == (r[1] == "Context"), r


def doc_rows():
    """`QDC_X` [default] of the scope tables of INTEGRATION.md §7, per scope heading."""
    text = (ROOT / "INTEGRATION.md").read_text()
    sec = text[text.index("## 7. Profiling and runtime knobs"):]
    rows = []
    for scope in SCOPES:
        head = f"### {scope} knobs\n"
        assert sec.count(head) == 1, scope
        body = sec[sec.index(head) + len(head):]
        body = body[:body.index("\n### ")]
        assert body.strip().startswith("Read "), f"{scope}: no sentence saying when it is read"
        for m in re.finditer(r"^\| `(QDC_[A-Z0-9_]+)` \[(.*?)\] \|", body, re.M):
            rows.append((m.group(1), scope, m.group(2)))
    return rows


def test_documentation_lists_the_table():
    table = q.knob_table("f32")
    doc = doc_rows()
    assert len(doc) == len({d[0] for d in doc}), "a knob documented twice"
    assert {(d[0], d[1]) for d in doc} == {(r[0], r[1]) for r in table}
    dflt = {r[0]: r[2] for r in table}
    wrong = [(n, d, dflt[n]) for n, _, d in doc
             if as_int(dflt[n]) is not None and as_int(d) != as_int(dflt[n])]
    assert not wrong, f"(knob, default in INTEGRATION.md, default in the table): {wrong}"


# The one "QDC_..." literal of csrc/ that is no environment name: the amdgpu_waves_per_eu text of
# a specialized kernel (qdc_variant.hpp), a compile-time macro's name spliced into generated
# kernel source.  (Its neighbours, such as "QDC_RW_WAVES, QDC_RW_WAVES", do not match the pattern.)
SOURCE_TEXT = ['"QDC_RQ_PF_WAVES"']


def test_one_reader():
    """Outside qdc_knobs.hpp, csrc/ calls getenv only for HOME, XDG_CACHE_HOME and ROCM_PATH and
    holds no "QDC_..." string literal (but SOURCE_TEXT); qdc_knobs.hpp calls it once."""
    files = sorted(CSRC.glob("*.hpp")) + [CSRC / "qdc.hip"]
    assert CSRC / "qdc_knobs.hpp" in files
    for f in files:
        src = f.read_text()
        if f.name == "qdc_knobs.hpp":
            assert len(re.findall(r"getenv\(", src)) == 1
            continue
        calls = re.findall(r"getenv\(\s*([^)]*)\)", src)
        assert all(c in ('"HOME"', '"XDG_CACHE_HOME"', '"ROCM_PATH"') for c in calls), (f.name, calls)
        lits = re.findall(r'"QDC_[A-Z0-9_]+"', src)
        assert lits == (SOURCE_TEXT if f.name == "qdc_variant.hpp" else []), (f.name, lits)
    assert SOURCE_TEXT[0].strip('"') not in [r[0] for r in q.knob_table("f32")]

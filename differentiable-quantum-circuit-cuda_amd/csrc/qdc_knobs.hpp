// The QDC_* runtime knobs: one table, one reader.
//
// Every environment variable the library reads is one row of QDC_KNOBS below: its name (QDC_ +
// the id), its scope (when it is read), its default as display text and a one-line effect.  The
// row's id is the only way to read it (knob_text, the one getenv of a QDC_* name in csrc/), so a
// name that is not in the table does not compile.  INTEGRATION.md §7 documents the same rows
// and qdc_knob_table exports them; tests/test_knobs_cpu.py holds table, code and document
// together.  A new knob is a row here, a typed read where it acts and a row in INTEGRATION.md.
//
// Plain C++17, no HIP: the defaults that depend on kernel constants (NBMAX, FMAX_OPS,
// TILE_CHUNKS_*) live with the values, in Ctx::Knobs (qdc_device.hpp) and Circuit::Knobs
// (qdc_circuit.hpp).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace qdc {

// When a knob is read.  Process: once per process (a function-local static, or the kernel
// cache's one initialisation).  Context: when a Ctx is created (Ctx::Knobs::read).  Circuit:
// when a circuit is created, dry circuits included (Circuit::Knobs::read).  Call: on every call
// of the function it acts in.  Hook: only by a host-only test hook (qdc.hip).
enum class KnobScope { Process, Context, Circuit, Call, Hook };

// X(id, scope, default, effect)
#define QDC_KNOBS(X)                                                                               \
  /* ---- Ctx::Knobs (qdc_device.hpp) ---- */                                                      \
  X(DYN, Context, "35",                                                                            \
    "static share (% of the fair share) of a dynamic-tail pass; 100: static only")                 \
  X(DYN_GRAN, Context, "1",                                                                        \
    "smallest granule (tiles per grab, a power of two <= 32) of a reducing dynamic tail")          \
  X(EVENT_FENCE, Context, "0",                                                                     \
    "1: the profiler's HIP events are default events (system-scope fence per record)")             \
  X(GRID_CAP, Context, "1048576", "grid cap of the single-gate streaming kernels")                 \
  X(RED_CAP, Context, "2048", "grid of the single-gate reduction kernels (<= 4096)")               \
  X(REV_RED, Context, "4096",                                                                      \
    "grid of the single-gate reverse launches with a gradient (<= 4096)")                          \
  X(DIRECT_IT, Context, "0", "minimum items per thread of streaming direct launches")              \
  X(TILE_FAR, Context, "3",                                                                        \
    "far-target single-gate ops on the tile family, bits: 1 reverse, 2 one-state, 4 inject / "     \
    "grad")                                                                                        \
  X(XCD_MAP, Context, "1",                                                                         \
    "XCD-aware block order, bits: 1 streaming, 2 reducing, 4 diagonal launches")                   \
  X(TILE2_WIDE, Context, "2", "two-state tile-family launches on 2^(9 + w)-chunk tiles")           \
  X(TILE1_WIDE, Context, "2", "one-state tile-family launches on 2^(10 + w)-chunk tiles")          \
  X(LANE, Context, "2",                                                                            \
    "single-gate ops on the LANE family, bits: 1 reverse, 2 streaming one-state, 4 densities "     \
    "/ gradients")                                                                                 \
  X(DIAG_RU, Context, "16",                                                                        \
    "chunks per state in flight per thread of the diagonal reverse kernels")                       \
  X(DIAG_Q, Context, "1", "0: diagonal reverse launches on k_diag instead of k_diag_q")            \
  X(DIAG_RED, Context, "4096", "grid of the diagonal reverse's reducing launches (<= 4096)")       \
  X(TILE_PF, Context, "1", "0: tile-family blocks of several tiles do not prefetch the next tile") \
  X(LANE_BLK, Context, "1",                                                                        \
    "0: far-target streaming LANE launches stay on the wave variant, not k_lane_blk")              \
  X(LANE_TILE_BITS, Context, "0x8800000",                                                          \
    "mask of target byte strides 2^b whose one-state q1 applications run on the tile family")      \
  X(LANE_NOBLK_BITS, Context, "0x808000",                                                          \
    "mask of target byte strides 2^b whose far LANE applications run on the wave variant")         \
  X(LANE_U, Context, "8,1,4",                                                                      \
    "units in flight per wave of LANE launches, \"u0,u1,u2\" per op class as QDC_LANE")            \
  /* ---- Circuit::Knobs (qdc_circuit.hpp) ---- */                                                 \
  X(FUSE, Circuit, "1", "0: one HBM pass per gate (single-gate kernels only)")                     \
  X(FUSE_MAX_OPS, Circuit, "f32: 64, f64: 32", "gates per fused pass (1 .. FMAX_OPS)")             \
  X(FUSE_MEAS, Circuit, "1", "0: densities / cotangent injections stay single passes")             \
  X(FUSE_LCMIN, Circuit, "3", "minimum contiguous chunk bits of a fused tile (1 .. 6)")            \
  X(FUSED_BLOCKS, Circuit, "0",                                                                    \
    "grid of fused passes (1 .. 4096); 0: as many blocks as are resident")                         \
  X(RQ, Circuit, "1", "0: gate passes on the LDS-tile kernel, not the register-resident ones")     \
  X(RQ64, Circuit, "1", "0: f64 gate passes stay on the LDS-tile kernel")                          \
  X(RQ_STATS, Circuit, "0",                                                                        \
    "1: print each register-resident pass's counts to stderr; 2: its stages too")                  \
  X(RW, Circuit, "1", "register-resident kernel choice, a bit mask (qdc_variant.hpp)")             \
  X(RQ_PF, Circuit, "1", "0: one-state register-resident passes do not prefetch the next tile")    \
  X(RQ_SLOTS5, Circuit, "1", "0: f32 one-wave passes plan four register slots, not five")          \
  X(RQ_ORDER, Circuit, "2",                                                                        \
    "register-resident tile order: 0 block-contiguous, 1 grid-strided, 2 XCD-aware")               \
  X(RQ_PERM, Circuit, "1", "0: gate-only passes keep the qubit layout (no in-store permutation)")  \
  X(RQ_PERM_SHARD, Circuit, "1", "0: no permuting passes on sharded circuits")                     \
  X(RQ_PERM_LOW, Circuit, "0", "low positions a permuting pass fills; 0: the planner's default")   \
  X(RQ_GRAD32, Circuit, "1",                                                                       \
    "0: two-state passes hold FMAX_GRAD instead of QDC_RQ_GCAP Gamma stages")                      \
  X(RQ_GCAP, Circuit, "f32: 32, f64: 16",                                                          \
    "Gamma stages a two-state register-resident pass holds (1 .. FMAX_GRAD_RQ)")                   \
  X(RQ_MAXCL, Circuit, "1", "0: relayouts chosen greedily instead of by max closure")              \
  X(RQ_GSTAGE, Circuit, "1",                                                                       \
    "0: two-state passes capped by variable gates instead of Gamma stages")                        \
  X(TILE1_CHUNKS, Circuit, "2048", "one-state fused tile in chunks: 2048 or 1024")                 \
  X(DIAG_INJECT, Circuit, "1",                                                                     \
    "0: runs of diagonal cotangent injections stay fused injection passes")                        \
  X(EARLY_INJECT, Circuit, "1",                                                                    \
    "0: the backward's leading diagonal injection waits for its program")                          \
  X(DENS1, Circuit, "1", "0: read-only one-qubit density passes on k_fused instead of k_dens1")    \
  X(DENS_SPLIT, Circuit, "1", "0: a forward pass may hold gates and densities together")           \
  X(MIRROR, Circuit, "1",                                                                          \
    "mirrored reverse sweeps; 0: the backward schedules itself; 2: failing to mirror is an "       \
    "error")                                                                                       \
  X(DEFER_Q1, Circuit, "1", "0: trailing one-qubit stages of a pass stay there")                   \
  X(FUSE_SEARCH, Circuit, "1",                                                                     \
    "0: a pass's qubits are whatever the scan meets first, not chosen by search")                  \
  X(SCHED_CACHE, Circuit, "1",                                                                     \
    "0: schedule every call instead of reusing the last call's schedule")                          \
  X(SPEC, Circuit, "1",                                                                            \
    "specialized passes: 0 off, 1 from QDC_SPEC_MIN_QUBITS local qubits, 2 always")                \
  X(SPEC_MIN_QUBITS, Circuit, "22", "local qubits from which QDC_SPEC=1 specializes")              \
  X(SPEC_MAX, Circuit, "160", "distinct specialized kernels a call compiles in line")              \
  X(SPEC_FWD, Circuit, "1", "0: only the two-state reverse passes are specialized")                \
  X(SPEC_ASYNC, Circuit, "f32: 1, f64: 0",                                                         \
    "programs above QDC_SPEC_MAX compile in the background; 0: they stay generic")                 \
  X(SPEC_HALF, Circuit, "1",                                                                       \
    "0: five-slot specialized passes relayout through the full LDS buffer")                        \
  X(STATE_ILV, Circuit, "1", "0: separate fwd / bwd allocations instead of the interleaved pair")  \
  X(STATE_ILV_BITS, Circuit, "12", "block size of the interleaved pair, 2^b chunks (4 .. 24)")     \
  /* ---- once per process ---- */                                                                 \
  X(SPEC_IMM, Process, "0", "1: specialized relayouts address LDS by immediate offsets")           \
  X(RQ_SWZ, Process, "1", "0: register-resident relayouts use the k_fused LDS swizzle")            \
  X(PACK_TILE, Process, "1", "0: remap packing on the direct kernel instead of LDS tiles")         \
  X(JIT_DIR, Process, "$XDG_CACHE_HOME/qdc_jit, $HOME/.cache/qdc_jit or /tmp/qdc_jit_<uid>",       \
    "code-object cache of the specialized kernels")                                                \
  X(JIT_PREBUILT, Process, "<lib>/../jit-prebuilt",                                                \
    "directory of kernels compiled ahead of time; 0: none")                                        \
  X(SRC_DIR, Process, "<lib>/../csrc", "kernel headers the specialized passes compile against")    \
  X(HIPCC, Process, "$ROCM_PATH/bin/hipcc", "compiler of the specialized passes")                  \
  /* ---- every call ---- */                                                                       \
  X(JIT_JOBS, Call, "min(hardware threads, 16) / ranks", "parallel hipcc processes (<= 16)")       \
  X(JIT_ASYNC_JOBS, Call, "as QDC_JIT_JOBS", "kernels per batch of the background compiler")       \
  X(JIT_WAIT_S, Call, "900", "seconds to wait for a kernel another process compiles")              \
  X(JIT_KEEP, Call, "0", "1: keep the sources and logs of successful compiles")                    \
  X(QK_PAIR, Call, "1", "dense k-qubit kernel: 0 no paired 16-B accesses, 2 paired at k = 4 too")  \
  X(QK_WIDE, Call, "k >= 4: 1, else 0",                                                            \
    "dense k-qubit kernel: doubled batches per wave iteration")                                    \
  X(QK_PF, Call, "k = 3: 2, k = 5: 1, else 0",                                                     \
    "dense k-qubit kernel: 1 software-pipelined batches, 2 doubled too")                           \
  X(QK_GRID, Call, "4096", "block cap of the dense k-qubit kernels' grids")                        \
  X(QK_LDS, Call, "k = 3: 2, else 1",                                                              \
    "low targets from which a dense gate runs as LDS-staged tiles; 0: never")                      \
  X(QKL_VAR, Call, "1", "k_qkl variant: 0 not pipelined, 1 pipelined, 2 half the tiles at k = 5")  \
  X(QKG_GRID, Call, "resident blocks", "block cap of the dense gradient / density kernel")         \
  X(PAULI_GRID, Call, "per kernel", "block cap of the Pauli-sum kernels")                          \
  /* ---- host-only test hooks (qdc.hip) ---- */                                                   \
  X(SCHED_RQ, Hook, "0",                                                                           \
    "qdc_fusion_schedule: permuting passes and the register-resident Gamma cap")                   \
  X(SCHED_PERM, Hook, "as QDC_SCHED_RQ", "qdc_fusion_schedule: permuting passes alone")            \
  X(SCHED_MIRROR, Hook, "0", "qdc_fusion_schedule: the mirrored forward schedule")                 \
  X(SCHED_GCAP, Hook, "16",                                                                        \
    "qdc_fusion_schedule: Gamma stages of a two-state pass (1 .. FMAX_GRAD_RQ)")                   \
  X(TILE2_CHUNKS, Hook, "1024", "qdc_fusion_schedule: two-state fused tile in chunks")             \
  X(RQ_KEEP, Hook, "0", "qdc_rq_plan: every relayout keeps a register slot (half buffers)")        \
  X(PRECOMPILE_DUMP, Hook, "unset",                                                                \
    "qdc_precompile: directory that receives each kernel's source")                                \
  X(PRECOMPILE_COUNT, Hook, "0", "qdc_precompile: 1 counts the kernels without compiling them")

enum class Knob : int {
#define QDC_KNOB_ID(id, scope, dflt, effect) id,
  QDC_KNOBS(QDC_KNOB_ID)
#undef QDC_KNOB_ID
};

struct KnobRow {
  const char* name;
  KnobScope scope;
  const char* dflt;
  const char* effect;
};
inline constexpr KnobRow KNOB_TABLE[] = {
#define QDC_KNOB_ROW(id, scope, dflt, effect) {"QDC_" #id, KnobScope::scope, dflt, effect},
    QDC_KNOBS(QDC_KNOB_ROW)
#undef QDC_KNOB_ROW
};
constexpr size_t KNOB_COUNT = sizeof(KNOB_TABLE) / sizeof(KNOB_TABLE[0]);

inline const char* knob_scope_name(KnobScope s) {
  constexpr const char* names[] = {"Process", "Context", "Circuit", "Call", "Hook"};
  return names[(int)s];
}

// ---- the reader: a knob's text (nullptr: unset), and the typed forms over it.  Parsing is
// atoi / atol / atof / strtoull(base 0): malformed text is accepted silently, as ever. ----
inline const char* knob_text(Knob k) { return std::getenv(KNOB_TABLE[(int)k].name); }
inline int knob_int(Knob k, int dflt) {
  const char* e = knob_text(k);
  return e ? atoi(e) : dflt;
}
// (a set value is clamped to [lo, hi]; the default is returned as it is)
inline int knob_int(Knob k, int dflt, int lo, int hi) {
  const char* e = knob_text(k);
  return e ? std::max(lo, std::min(atoi(e), hi)) : dflt;
}
inline long knob_long(Knob k, long dflt, long lo, long hi) {
  const char* e = knob_text(k);
  return e ? std::min(std::max(lo, atol(e)), hi) : dflt;
}
inline uint32_t knob_uint(Knob k, uint32_t dflt) {
  const char* e = knob_text(k);
  return e ? (uint32_t)atoi(e) : dflt;
}
inline uint64_t knob_mask(Knob k, uint64_t dflt) {
  const char* e = knob_text(k);
  return e ? strtoull(e, nullptr, 0) : dflt;
}
inline double knob_double(Knob k, double dflt) {
  const char* e = knob_text(k);
  return e ? atof(e) : dflt;
}
// "u0,u1,u2" (QDC_LANE_U): all three or none
inline void knob_triple(Knob k, uint32_t (&u)[3]) {
  unsigned v[3] = {0, 0, 0};
  const char* e = knob_text(k);
  if (e && sscanf(e, "%u,%u,%u", &v[0], &v[1], &v[2]) == 3)
    for (int i = 0; i < 3; ++i) u[i] = v[i];
}

// ---- the two knob structs list their members once, as f(Knob::X, member[, lo, hi]) (their
// each()): KnobRead fills them from the environment, KnobShow prints them (qdc_knob_table) ----
struct KnobRead {
  void operator()(Knob k, int& v) const { v = knob_int(k, v); }
  void operator()(Knob k, uint32_t& v) const { v = knob_uint(k, v); }
  void operator()(Knob k, uint32_t& v, int lo, int hi) const {
    v = (uint32_t)knob_int(k, (int)v, lo, hi);
  }
  void operator()(Knob k, uint64_t& v) const { v = knob_mask(k, v); }
  void operator()(Knob k, uint32_t (&v)[3]) const { knob_triple(k, v); }
};
struct KnobShow {
  std::string* out;  // [KNOB_COUNT]
  void operator()(Knob k, int v, int = 0, int = 0) const { out[(int)k] = std::to_string(v); }
  void operator()(Knob k, uint32_t v, int = 0, int = 0) const { out[(int)k] = std::to_string(v); }
  void operator()(Knob k, uint64_t v) const {
    char b[32];
    snprintf(b, sizeof b, "0x%llx", (unsigned long long)v);
    out[(int)k] = b;
  }
  void operator()(Knob k, const uint32_t (&v)[3]) const {
    out[(int)k] = std::to_string(v[0]) + "," + std::to_string(v[1]) + "," + std::to_string(v[2]);
  }
};

}  // namespace qdc

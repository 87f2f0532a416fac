// qdc_circuit.hpp — the circuit interpreter (src/circuit.rs:53-430 and the QuantizedTensor
// methods it calls, src/quantized_tensor.rs:54-238) as a native C++ runtime.
//
// Device state per circuit: `initial` (set_state_from_vector target), `state` (the forward
// state; the reverse sweep uncomputes it in place, exactly as circuit.rs:275 borrows
// self.state), `bwd` (the cotangent state, allocated on the first backward and kept), a
// gradient buffer and a density buffer.  That is 3 full states, never the reference's
// transient 4th (`conj_and_double` allocation per density injection, quantized_tensor.rs:81-86).
#pragma once

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include <rccl/rccl.h>

#include "qdc/circuit.h"
#include "qdc_device.hpp"
#include "qdc_shard.hpp"
#include "qdc_stage.hpp"
#include "qdc_fusion.hpp"
#include "qdc_spec.hpp"

namespace qdc {

// A flattened list of host buffers (gate matrices or density cotangents).
struct Flat {
  const qdc_complex* data;
  std::vector<size_t> off;
  std::vector<size_t> len;
  Flat(const qdc_complex* d, const size_t* lens, size_t n) : data(d), off(n), len(n) {
    size_t o = 0;
    for (size_t i = 0; i < n; ++i) {
      off[i] = o;
      len[i] = lens[i];
      o += lens[i];
    }
  }
  size_t size() const { return len.size(); }
  size_t total() const { return len.empty() ? 0 : off.back() + len.back(); }  // values in all
  const qdc_complex* at(size_t i) const { return data + off[i]; }
};

// a physical position after a pass's swaps, applied in order (qdc_fusion.hpp FusionItem::swaps)
inline uint32_t apply_swaps(const std::vector<std::pair<uint32_t, uint32_t>>& swaps, uint32_t p) {
  for (const auto& sw : swaps) {
    if (p == sw.first) p = sw.second;
    else if (p == sw.second) p = sw.first;
  }
  return p;
}
// the applied matrix and the pull-back of a gate of this kind (qdc_device.hpp GateMats)
inline const char* gate_mats(int kind, const qdc_complex* g, bool uncompute, GateMats& m) {
  return gate_mats(g, is_diag(kind), is_q1_gate(kind), is_nonu(kind), uncompute, m);
}

// The assertion sequence of QuantizedTensor::apply_* (quantized_tensor.rs:100-152).
inline const char* check_density_pos(const Instr& in, uint32_t n) {
  if (is_q1_gate(in.kind) || is_q1_density(in.kind)) {
    if (in.a >= n) return fail("pos is out of the bound.");
  } else {
    if (in.a == in.b) return fail("pos1 and pos2 must be different.");
    if (in.b >= n) return fail("pos1 is out of the bound.");
    if (in.a >= n) return fail("pos2 is out of the bound.");
  }
  return nullptr;
}
inline const char* check_gate(const Instr& in, size_t len, uint32_t n) {
  if (len != (size_t)gate_len(in.kind)) return fail("Incorrect len of the gate's buffer.");
  return check_density_pos(in, n);
}

#define QDC_NCCL(call)                                                                   \
  do {                                                                                   \
    ncclResult_t qdc_r_ = (call);                                                        \
    if (qdc_r_ != ncclSuccess)                                                           \
      return ::qdc::fail("RCCL ERROR: call of a function \"%s\" in line %d of file %s "  \
                         "failed with %s.",                                              \
                         #call, __LINE__, __FILE__, ncclGetErrorString(qdc_r_));          \
  } while (0)

// Per-device resources of a circuit: a context (stream, reduction arena, profiling) and the
// device copy of the fused-pass program.  One per shard when the shards run on their own
// streams (single-process multi-GPU, or the multi-stream rehearsal on one GPU), else one shared
// by every local shard.
struct DevRes {
  Ctx ctx;
  unsigned char* prog_dev = nullptr;
};

struct Shard {
  cx* initial = nullptr;
  cx* state = nullptr;
  cx* bwd = nullptr;
  bool bwd_live = false;  // bwd holds a cotangent (written by a backward): readable
  cx* scratch = nullptr;  // all-to-all staging (allocated when world > 1)
  std::vector<void*> owned;  // state allocations (remaps swap the pointers above among them)
  cx* dens = nullptr;
  cx* grads = nullptr;
  DevRes* d = nullptr;  // the shard's device resources
  Ctx& c() const { return d->ctx; }
};

// The shard exchange.  Transports:
//   * RCCL, one shard per process (one rank per GPU, xGMI): `comm`;
//   * RCCL, every shard of the job in this process, one per GPU (ncclCommInitAll): `comms`,
//     one collective per shard inside ncclGroupStart/End, each on its shard's stream;
//   * loopback, every shard on this process's one GPU: device-to-device copies — on one shared
//     stream, or (`multi_stream`) on the shards' own streams ordered by events.
struct Exchange {
  int world = 1;   // total shards
  int rank0 = 0;   // global index of this process's first shard
  int nlocal = 1;  // shards held by this process
  ncclComm_t comm = nullptr;
  std::vector<ncclComm_t> comms;
  bool multi_stream = false;
  std::vector<hipEvent_t> ev;  // multi_stream: one per shard

  static ncclDataType_t type() { return sizeof(real) == 4 ? ncclFloat : ncclDouble; }
  const char* events(size_t n) {
    while (ev.size() < n) {
      hipEvent_t e;
      QDC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      ev.push_back(e);
    }
    return nullptr;
  }
  // every shard stream waits for every other shard stream's work so far
  const char* join(std::vector<Shard>& sh) {
    QDC_TRY(events(sh.size()));
    for (size_t s = 0; s < sh.size(); ++s) {
      QDC_TRY(sh[s].c().use());
      QDC_HIP(hipEventRecord(ev[s], sh[s].c().stream));
    }
    for (size_t d = 0; d < sh.size(); ++d)
      for (size_t s = 0; s < sh.size(); ++s)
        if (s != d) QDC_HIP(hipStreamWaitEvent(sh[d].c().stream, ev[s], 0));
    return nullptr;
  }

  // Block j of send[s] (chunk amplitudes) goes to shard j and lands as block s of recv[j].
  const char* alltoall(std::vector<Shard>& sh, std::vector<cx*>& send, std::vector<cx*>& recv,
                       size_t chunk) {
    if (world == 1) return nullptr;
    const double bytes = (double)chunk * sizeof(cx) * (world - 1);  // per shard
    std::vector<ProfSpan> span(sh.size());
    for (size_t s = 0; s < sh.size(); ++s) span[s] = sh[s].c().prof_begin();
    if (comm) {
      QDC_NCCL(ncclAllToAll(send[0], recv[0], chunk * 2, type(), comm, sh[0].c().stream));
    } else if (!comms.empty()) {
      QDC_NCCL(ncclGroupStart());
      for (size_t s = 0; s < sh.size(); ++s)
        QDC_NCCL(ncclAllToAll(send[s], recv[s], chunk * 2, type(), comms[s], sh[s].c().stream));
      QDC_NCCL(ncclGroupEnd());
    } else {
      if (multi_stream) QDC_TRY(join(sh));  // sources written, destinations free
      for (int d = 0; d < nlocal; ++d)
        for (int s = 0; s < nlocal; ++s)
          QDC_HIP(hipMemcpyAsync(recv[d] + (size_t)s * chunk, send[s] + (size_t)d * chunk,
                                 chunk * sizeof(cx), hipMemcpyDeviceToDevice, sh[d].c().stream));
      if (multi_stream) QDC_TRY(join(sh));  // no source is rewritten before every copy is done
    }
    for (size_t s = 0; s < sh.size(); ++s)
      sh[s].c().prof_end(span[s], "alltoall", bytes, 0.0);  // link bytes, not HBM bytes
    return nullptr;
  }
  // in-place sum over all shards of `count` complex values (every shard's buffer holds the sum)
  const char* allreduce(std::vector<Shard>& sh, std::vector<cx*>& bufs, size_t count) {
    if (world == 1 || count == 0) return nullptr;
    if (comm) {
      QDC_NCCL(ncclAllReduce(bufs[0], bufs[0], count * 2, type(), ncclSum, comm, sh[0].c().stream));
      return nullptr;
    }
    if (!comms.empty()) {
      QDC_NCCL(ncclGroupStart());
      for (size_t s = 0; s < sh.size(); ++s)
        QDC_NCCL(ncclAllReduce(bufs[s], bufs[s], count * 2, type(), ncclSum, comms[s],
                               sh[s].c().stream));
      QDC_NCCL(ncclGroupEnd());
      return nullptr;
    }
    if (multi_stream) QDC_TRY(join(sh));
    Ctx& c0 = sh[0].c();
    QDC_TRY(c0.use());
    for (int s = 1; s < nlocal; ++s) QDC_TRY(elementwise_count<2>(c0, bufs[s], bufs[0], count));
    for (int s = 1; s < nlocal; ++s)
      QDC_HIP(hipMemcpyAsync(bufs[s], bufs[0], count * sizeof(cx), hipMemcpyDeviceToDevice,
                             c0.stream));
    if (multi_stream) QDC_TRY(join(sh));
    return nullptr;
  }
  void destroy() {
    for (auto e : ev) (void)hipEventDestroy(e);
    ev.clear();
    for (auto c : comms) (void)ncclCommDestroy(c);
    comms.clear();
  }
};

struct Circuit {
  uint32_t n = 0;   // logical qubits
  uint32_t g = 0;   // rank bits
  uint32_t nl = 0;  // local qubits of a shard
  // interleaved state pair (unsharded): fwd and bwd alternate in 2^gap_bits-chunk blocks of one
  // allocation; chunk c of either state at c + (c & gm), bwd = fwd + 2^gap_bits chunks
  uint32_t gap_bits = 0;
  uint64_t gm = 0;
  std::vector<std::unique_ptr<DevRes>> devs;  // per-device resources (sh[s].d points here)
  Exchange ex;
  std::vector<Shard> sh;
  QubitMap layout;  // physical layout of every shard's `state` (identity until a remap)
  size_t dens_cap = 0, grads_cap = 0;
  cx* host_out = nullptr;  // pinned
  size_t host_cap = 0;
  std::vector<Instr> ins;
  // The circuit's QDC_* knobs (qdc_knobs.hpp, scope Circuit): read() fills them from the
  // environment when a circuit is created, dry circuits included; host only.
  struct Knobs {
    // fused multi-gate passes
    int fuse = 1;             // 0: one HBM pass per gate
    // gates per fused pass: twice the Gamma cap (a brickwork stage holds two gates and more)
    uint32_t fuse_max_ops = 2 * RQ_GCAP_DEFAULT;
    uint32_t fuse_lcmin = 3;  // min contiguous chunk bits of a fused tile (128-B rows)
    int fuse_meas = 1;        // densities / cotangent injections join fused passes
    int use_rq = 1;           // f32 gate passes run register-resident (qdc_rq.hpp)
    int rq_stats = 0;
    // which register-resident kernel variant runs a pass (QDC_RW, QDC_RQ_PF, QDC_RQ_SLOTS5): read
    // by rq_variant() below and nowhere else
    RqKnobs rqk;
    int rq64 = 1;  // f64 gate passes register-resident too (k_rw; QDC_RQ64)
    // register-resident tile order: 0 block-contiguous, 1 grid-strided, 2 block-contiguous in
    // XCD-aware block order (QDC_RQ_ORDER).  C2 n = 28, same box (profiles/r5/r5q_*): 2 is
    // +0.4-0.6 % over 0, 1 (concurrent tiles neighbours in memory) -6.5 %
    int rq_order = 2;
    // register-resident passes as straight-line kernels specialized per pass program
    // (qdc_spec.hpp, qdc_jit.hpp; QDC_SPEC): 0 off, 1 for states of >= spec_min_qubits local
    // qubits, 2 always; a call whose program needs more than spec_max distinct kernels runs generic
    int spec_mode = 1;
    uint32_t spec_min_qubits = 22;
    uint32_t spec_max = 160;
    int spec_fwd = 1;  // forward (one-state) passes too (QDC_SPEC_FWD)
    // a program with more than spec_max distinct kernels: its missing kernels are compiled by the
    // JIT's background thread while the generic kernels run its passes, later calls launch the
    // specialized ones as their objects appear (QDC_SPEC_ASYNC=0: such programs stay generic).
    // f32 only by default: f32 specialized and generic passes are bit-identical, so a result never
    // depends on how far the background compiler has got; f64 ones differ in the last bits (the
    // compiler contracts the scalar complex arithmetic differently), so a deep f64 program stays
    // generic — reproducible from call to call — unless QDC_SPEC_ASYNC=1 opts in
    int spec_async = sizeof(real) == 4 ? 1 : 0;
    int rq_permute = 1;      // gate-only passes permute their tile's qubits (QDC_RQ_PERM)
    int rq_perm_shard = 1;    // ... on sharded circuits too (QDC_RQ_PERM_SHARD)
    int rq_grad32 = 1;        // two-state passes hold up to rq_gcap Gamma stages (QDC_RQ_GRAD32)
    // Gamma stages a two-state register-resident pass holds (QDC_RQ_GCAP, 1 .. FMAX_GRAD_RQ;
    // FusionPlanner::gamma_cap).  The defaults were measured: DESIGN.md "Fewer, fuller passes"
    uint32_t rq_gcap = RQ_GCAP_DEFAULT;
    int rq_maxcl = 1;         // relayouts chosen by max closure, else greedily (QDC_RQ_MAXCL)
    uint32_t rq_perm_low = 0;  // low positions a permuting pass fills, 0: default (QDC_RQ_PERM_LOW)
    int rq_gstage = 1;  // two-state passes capped by Gamma stages, not variable gates (QDC_RQ_GSTAGE)
    // one-state fused tile in chunks (QDC_TILE1_CHUNKS): TILE_CHUNKS_1, or TILE_CHUNKS_2 (f32:
    // 2^11 amplitudes; the kernels of either size: qdc_variant.hpp)
    uint32_t tile1_chunks = FusionPlanner::TILE_CHUNKS_1;
    // runs of cotangent injections whose cotangents are all diagonal become one elementwise pass
    // (k_diag_inject; QDC_DIAG_INJECT)
    int diag_inject = 1;
    // the backward's leading diagonal-injection passes launched before its program is built
    // (QDC_EARLY_INJECT)
    int early_inject = 1;
    // read-only passes of one-qubit densities on k_dens1 (register partial sums across a block's
    // tiles, one reduction per block; QDC_DENS1=0: k_fused's per-tile reductions)
    int dens1_kernel = 1;
    int dens_split = 1;  // forward passes hold gates or densities, not both (qdc_fusion.hpp split_dens)
    // Mirrored schedules (QDC_MIRROR): the forward is scheduled on the two-state tile under both
    // directions' rules (qdc_fusion.hpp FusionPlanner::mirror) and the backward runs its passes in
    // reverse, uncomputing each stage with exactly the adjoint of the matrix the forward applied —
    // the O(1)-memory uncompute then drifts like the reference's gate-by-gate U, U^dagger sequence
    // instead of accumulating the rounding of independently formed stage products.  Sharded
    // circuits too (round 5): the forward's remap plan keeps both directions' order relations and
    // the backward undoes its remaps in reverse (remap, inverse).  The backward must follow a forward call
    // with the same gates (else the backward schedules itself as usual).  On by default (round
    // 4: C5 n = 14 f32 uncompute 4.85x -> 1.4x the reference's floor; C2 n = 28 f32 ~3.5 %
    // slower, DESIGN.md "Uncompute drift").
    int mirror = 1;
    // one-state one-wave specialized passes relayout through half the LDS buffer when every
    // relayout keeps a register slot (QDC_SPEC_HALF; twice the resident waves)
    int spec_half = 1;
    // trailing one-qubit stages of a pass join their qubit's next two-qubit stage in a later pass
    // (qdc_fusion.hpp defer_trailing_q1; QDC_DEFER_Q1)
    int defer_q1 = 1;
    // each pass's tile chosen by search instead of by scan order (qdc_fusion.hpp search_pass;
    // QDC_FUSE_SEARCH)
    int fuse_search = 1;
    // grid of fused passes (QDC_FUSED_BLOCKS); 0: as many blocks as are resident at once
    // (occupancy query)
    uint32_t fused_blocks = 0;
    // the pass schedule of a call is reused by the next call with the same plan (sched_cache;
    // QDC_SCHED_CACHE)
    int sched_cache_on = 1;
    // the forward and cotangent states interleaved in one allocation, in blocks of
    // 2^state_ilv_bits chunks (alloc_pair; QDC_STATE_ILV, QDC_STATE_ILV_BITS)
    int state_ilv = 1;
    uint32_t state_ilv_bits = 12;

    template <class K, class F>
    static void each(K& k, F&& f) {
      f(Knob::FUSE, k.fuse);
      f(Knob::FUSE_MAX_OPS, k.fuse_max_ops, 1, FMAX_OPS);
      f(Knob::FUSE_MEAS, k.fuse_meas);
      f(Knob::FUSE_LCMIN, k.fuse_lcmin, 1, LOWBITS);
      f(Knob::FUSED_BLOCKS, k.fused_blocks, 1, (int)NBMAX);
      f(Knob::RQ, k.use_rq);
      f(Knob::RQ64, k.rq64);
      f(Knob::RQ_STATS, k.rq_stats);
      f(Knob::RW, k.rqk.rq_wave);
      f(Knob::RQ_PF, k.rqk.rq_prefetch);
      f(Knob::RQ_SLOTS5, k.rqk.rq_slots5);
      f(Knob::RQ_ORDER, k.rq_order);
      f(Knob::RQ_PERM, k.rq_permute);
      f(Knob::RQ_PERM_SHARD, k.rq_perm_shard);
      f(Knob::RQ_PERM_LOW, k.rq_perm_low);
      f(Knob::RQ_GRAD32, k.rq_grad32);
      f(Knob::RQ_GCAP, k.rq_gcap, 1, FMAX_GRAD_RQ);
      f(Knob::RQ_MAXCL, k.rq_maxcl);
      f(Knob::RQ_GSTAGE, k.rq_gstage);
      f(Knob::TILE1_CHUNKS, k.tile1_chunks);
      f(Knob::DIAG_INJECT, k.diag_inject);
      f(Knob::EARLY_INJECT, k.early_inject);
      f(Knob::DENS1, k.dens1_kernel);
      f(Knob::DENS_SPLIT, k.dens_split);
      f(Knob::MIRROR, k.mirror);
      f(Knob::DEFER_Q1, k.defer_q1);
      f(Knob::FUSE_SEARCH, k.fuse_search);
      f(Knob::SCHED_CACHE, k.sched_cache_on);
      f(Knob::SPEC, k.spec_mode);
      f(Knob::SPEC_MIN_QUBITS, k.spec_min_qubits);
      f(Knob::SPEC_MAX, k.spec_max);
      f(Knob::SPEC_FWD, k.spec_fwd);
      f(Knob::SPEC_ASYNC, k.spec_async);
      f(Knob::SPEC_HALF, k.spec_half);
      f(Knob::STATE_ILV, k.state_ilv);
      f(Knob::STATE_ILV_BITS, k.state_ilv_bits, 4, 24);
    }
    const char* read() {
      each(*this, KnobRead{});
      constexpr uint32_t T1 = FusionPlanner::TILE_CHUNKS_1, T2 = FusionPlanner::TILE_CHUNKS_2;
      if (tile1_chunks != T1 && tile1_chunks != T2)
        return fail("%s must be %u or %u", KNOB_TABLE[(int)Knob::TILE1_CHUNKS].name, T1, T2);
      return nullptr;
    }
  } k;
  // host time of the calls (qdc_circuit_host_times): per direction (0 run/forward, 1 backward)
  // the calls and the milliseconds of setup, scheduling, program build, launching and the
  // finish (stream sync and result copies), accumulated since the last reset
  double host_ms[2][6] = {};
  using hclock = std::chrono::steady_clock;
  static double ms_between(hclock::time_point a, hclock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  }
  void host_record(int dir, const hclock::time_point (&t)[6]) {
    host_ms[dir][0] += 1;
    for (int k = 1; k < 6; ++k) host_ms[dir][k] += ms_between(t[k - 1], t[k]);
  }
  // generated kernels by pass program (key: spec_entry), with their functions
  std::map<std::vector<uint32_t>, SpecEntry> spec_cache;
  uint64_t spec_epoch = 0;
  bool mirror_on() const {
    return k.mirror && k.fuse && k.fuse_max_ops >= 2 && k.use_rq && (sizeof(real) == 4 || k.rq64);
  }
  // The kernel variant (qdc_variant.hpp) of a register-resident pass on 2^tbits-amplitude tiles:
  // the one selection that planning (emit_rq_pass), specialization and launch (launch_rq) share
  const char* rq_variant(bool two, uint32_t tbits, const RqVariant*& V) const {
    V = rq_select(two, tbits, k.rqk, mirror_on());
    if (!V)
      return fail("no register-resident kernel for a %u-amplitude %s tile", 1u << tbits,
                  two ? "two-state" : "one-state");
    return nullptr;
  }

  // host-only dry run (init_dry): calls stop before their first launch; build_program writes
  // the pass program into dry_prog and collects the specialized kernels into dry_specs
  bool dry = false;
  std::vector<unsigned char> dry_prog;
  std::vector<SpecEntry*> dry_specs;
  // dry-run trace of the matrices a call applies to the forward state (qdc_trace_program, the
  // host emulation tools/drift_emu.py): per fused stage or single gate its logical qubits (row
  // index 2 bit(q2) + bit(q1); q2 == q1 for one qubit), the matrix as uploaded (working
  // precision, diagonals expanded) and whether it is the adjoint of a recorded forward matrix
  struct TraceOp {
    uint32_t dir, item, q2, q1, R, diag, mirrored, single;
    qdc_complex m[16];
  };
  bool tracing = false;
  std::vector<TraceOp> trace;
  std::vector<uint8_t> inexact;  // per instruction: gate not unitary to working precision
  std::vector<std::pair<const void*, uint32_t>> fused_resident_cache;
  unsigned char* prog_host = nullptr;  // pinned staging of the pass program (every device's copy)
  size_t prog_cap = 0;

  Ctx& ctx0() { return devs[0]->ctx; }
  const char* sync_all() {
    for (auto& d : devs) QDC_TRY(d->ctx.sync());
    return nullptr;
  }
  const char* flush_all() {  // pending reduction slots of every context
    for (auto& d : devs) {
      QDC_TRY(d->ctx.use());
      QDC_TRY(d->ctx.flush());
    }
    return nullptr;
  }

  // n qubits over `world` shards (a power of two): g rank bits, nl local qubits (init, init_dry)
  const char* set_size(uint32_t qubits, int world) {
    n = qubits;
    const uint32_t gg = log2_exact((size_t)world);
    if (gg == UINT32_MAX || gg > 8) return fail("the number of shards must be a power of two <= 256");
    g = gg;
    if (g > 0 && n < 2 * g + 3)
      return fail("%u qubits are too few to shard over %d ranks (need >= %u)", n, world, 2 * g + 3);
    nl = n - g;
    ex.world = world;
    return nullptr;
  }
  // world = total shards (power of two), nlocal = shards in this process.  devices: one device
  // per local shard, each shard on its own stream (nullptr: every local shard on the current
  // device and one stream).  comms: one RCCL communicator per local shard (ncclCommInitAll;
  // devices then distinct), or none (copies between the streams of one device).
  const char* init(uint32_t qubits, int world = 1, int rank0 = 0, int nlocal = 1,
                   ncclComm_t comm = nullptr, const std::vector<int>* devices = nullptr,
                   const std::vector<ncclComm_t>* comms = nullptr) {
    DeviceGuard keep;
    // the communicators are owned from here on (destroy() frees them, also on a failure below)
    if (comms) ex.comms = *comms;
    QDC_TRY(set_size(qubits, world));
    ex.rank0 = rank0;
    ex.nlocal = nlocal;
    ex.comm = comm;
    ex.multi_stream = devices != nullptr && ex.comms.empty() && nlocal > 1;
    layout.identity(n, g);
    QDC_TRY(read_knobs(world, nlocal));
    int cur = 0;
    QDC_HIP(hipGetDevice(&cur));
    const int ndev = devices ? nlocal : 1;
    for (int i = 0; i < ndev; ++i) {
      devs.push_back(std::make_unique<DevRes>());
      QDC_TRY(devs.back()->ctx.init(devices ? (*devices)[i] : cur));
    }
    const size_t bytes = ((size_t)1 << nl) * sizeof(cx);
    sh.resize(nlocal);
    for (int s = 0; s < nlocal; ++s) {
      sh[s].d = devs[devices ? s : 0].get();
      Ctx& c = sh[s].c();
      QDC_TRY(c.use());
      QDC_HIP(hipMalloc(&sh[s].initial, bytes));
      sh[s].owned.push_back(sh[s].initial);
      QDC_TRY(alloc_pair(sh[s], bytes));
      if (g > 0) {
        QDC_HIP(hipMalloc(&sh[s].scratch, bytes));
        sh[s].owned.push_back(sh[s].scratch);
      }
      // QuantizedTensor::new_standard + clone (circuit.rs:96-102): |0..0> lives on shard 0
      if (rank0 + s == 0)
        QDC_TRY(set_standard(c, sh[s].initial, nl));
      else
        QDC_HIP(hipMemsetAsync(sh[s].initial, 0, bytes, c.stream));
      QDC_TRY(copy_initial(sh[s]));
    }
    QDC_TRY(sync_all());
    return nullptr;
  }
  // the runtime's QDC_* knobs (environment, read once per circuit)
  const char* read_knobs(int world, int nlocal) {
    QDC_TRY(k.read());
    // the node's hipcc processes shared among the ranks of a multi-process job
    SpecJit::get().set_processes(std::max(1, world / std::max(1, nlocal)));
    return nullptr;
  }
  // A host-only circuit (no device, no state): plans, schedules and pass programs exactly as
  // execute() / backward() build them, for the specialized kernels compiled ahead of time
  // (qdc_precompile; dry-run calls return before their first launch).
  const char* init_dry(uint32_t qubits, int world) {
    dry = true;
    QDC_TRY(set_size(qubits, world));
    ex.nlocal = 1;
    layout.identity(n, g);
    return read_knobs(world, world);  // (compiles: this process's full parallelism)
  }
  void destroy() {
    DeviceGuard keep;
    (void)sync_all();
    for (auto& s : sh) {
      if (s.d) (void)s.d->ctx.use();
      for (void* p : s.owned) (void)hipFree(p);
      for (cx* p : {s.dens, s.grads})
        if (p) (void)hipFree(p);
    }
    sh.clear();
    if (host_out) (void)hipHostFree(host_out);
    host_out = nullptr;
    for (auto& d : devs) {
      (void)d->ctx.use();
      if (d->prog_dev) (void)hipFree(d->prog_dev);
      d->prog_dev = nullptr;
      d->ctx.destroy();
    }
    devs.clear();
    if (prog_host) (void)hipHostFree(prog_host);
    prog_host = nullptr;
    ex.destroy();
  }

  // The forward and cotangent states as one allocation, interleaved in 64 KiB blocks (chunk
  // bit 12 selects the state).  Two states streamed together then run at one steady rate
  // whatever the placement (6.5 TB/s for in-place fwd+bwd at n = 28), while two separate 2 GiB
  // allocations land on placements that stream at 5.0-6.5 TB/s and the single-gate reverse
  // kernels at 64 % or 79 % of 8 TB/s from one circuit to the next (tools/alloc_probe.hip,
  // tools/pair_probe.hip, profiles/r2e_*, r2f_*).  Unsharded circuits only (a remap swaps the
  // states with the scratch buffer); QDC_STATE_ILV=0 keeps the plain layout (bwd separate and
  // allocated on the first backward).  The initial copy, the bwd zeroing and every gate-shaped
  // kernel address the pair through Ctx::gm; readbacks copy block by block (read_state).
  const char* alloc_pair(Shard& s, size_t bytes) {
    // block size: 2^12 chunks (QDC_STATE_ILV_BITS); states of at least two blocks
    const uint32_t gb = k.state_ilv_bits;
    bool ilv = k.state_ilv != 0 && g == 0 && sh.size() == 1 &&
               nchunks_of(nl) >= ((uint64_t)2 << gb);
    if (ilv) {
      // the pair allocates bwd now, not on the first backward (circuit.rs:276 creates it
      // lazily): when the device cannot hold it beside `initial` plus 1 GiB of headroom, keep
      // the plain layout, so a run/forward-only circuit still needs only two states
      size_t free_b = 0, total_b = 0;
      QDC_HIP(hipMemGetInfo(&free_b, &total_b));
      if (free_b < 2 * bytes + ((size_t)1 << 30)) ilv = false;
    }
    if (ilv) {
      gap_bits = gb;
      gm = ~(((uint64_t)1 << gap_bits) - 1);
      char* blk = nullptr;
      QDC_HIP(hipMalloc(&blk, 2 * bytes));
      s.owned.push_back(blk);
      s.state = (cx*)blk;
      s.bwd = (cx*)blk + ((size_t)VEC << gap_bits);
      s.c().gm = gm;
    } else {
      QDC_HIP(hipMalloc(&s.state, bytes));
      s.owned.push_back(s.state);
    }
    return nullptr;
  }
  // (kernels: a 2-D hipMemset / hipMemcpy over the 64 KiB blocks runs at < 1 TB/s)
  // every call starts from `initial`; while that is the standard state (the reference's
  // new_standard, circuit.rs:96-102: no set_state_from_vector yet) the state is written directly
  // (|0..0> on shard 0, zeros elsewhere: one write of S instead of a copy's read and write)
  bool initial_standard = true;
  const char* copy_initial(Shard& s) {
    if (initial_standard) {
      const bool first = ex.rank0 + (int)(&s - sh.data()) == 0;
      return first ? elementwise<3>(s.c(), nullptr, s.state, nl, gm)
                   : elementwise<4>(s.c(), nullptr, s.state, nl, gm);
    }
    return elementwise<0>(s.c(), s.initial, s.state, nl, gm);
  }
  const char* zero_bwd(Shard& s) {
    if (gm) return elementwise<4>(s.c(), nullptr, s.bwd, nl, gm);
    QDC_HIP(hipMemsetAsync(s.bwd, 0, ((size_t)1 << nl) * sizeof(cx), s.c().stream));
    return nullptr;
  }
  // host copy of amplitudes [offset, offset + len) of a (possibly interleaved) state
  const char* read_state(const Shard& s, const cx* src, size_t offset, qdc_complex* host,
                         size_t len) {
    const hipStream_t st = s.c().stream;
    if (!gm || (src != s.state && src != s.bwd)) {
      QDC_HIP(hipMemcpyAsync(host, src + offset, len * sizeof(cx), hipMemcpyDeviceToHost, st));
      return nullptr;
    }
    const size_t row = (size_t)VEC << gap_bits;  // amplitudes per block
    size_t o = offset, done = 0;
    auto piece = [&](size_t cnt) -> const char* {  // within one block
      const size_t phys = (o / row) * 2 * row + o % row;
      QDC_HIP(hipMemcpyAsync(host + done, src + phys, cnt * sizeof(cx), hipMemcpyDeviceToHost, st));
      o += cnt;
      done += cnt;
      return nullptr;
    };
    if (o % row && done < len) QDC_TRY(piece(std::min(len - done, row - o % row)));
    const size_t full = (len - done) / row;
    if (full) {
      QDC_HIP(hipMemcpy2DAsync(host + done, row * sizeof(cx), src + (o / row) * 2 * row,
                               2 * row * sizeof(cx), row * sizeof(cx), full,
                               hipMemcpyDeviceToHost, st));
      o += full * row;
      done += full * row;
    }
    if (done < len) QDC_TRY(piece(len - done));
    return nullptr;
  }

  const char* ensure_out(bool dens, size_t count) {
    size_t& cap = dens ? dens_cap : grads_cap;
    if (count <= cap) return nullptr;
    QDC_TRY(sync_all());
    for (auto& s : sh) {
      QDC_TRY(s.c().use());
      cx*& p = dens ? s.dens : s.grads;
      if (p) QDC_HIP(hipFree(p));
      p = nullptr;
      QDC_HIP(hipMalloc(&p, sizeof(cx) * count));
    }
    cap = count;
    return nullptr;
  }
  const char* ensure_host(size_t count) {
    if (count <= host_cap) return nullptr;
    if (host_out) {
      QDC_TRY(sync_all());
      QDC_HIP(hipHostFree(host_out));
    }
    host_out = nullptr;
    QDC_HIP(hipHostMalloc(&host_out, sizeof(cx) * count));
    host_cap = count;
    return nullptr;
  }

  // the densities a call of this mode returns
  static bool is_output(int kind, int mode) {
    return is_diff_density(kind) || (mode == QDC_MODE_RUN && is_density(kind));
  }
  size_t output_size(int mode) const {
    size_t c = 0;
    for (auto& in : ins)
      if (is_output(in.kind, mode)) c += is_q1_density(in.kind) ? 4 : 16;
    return c;
  }
  // the output index of every instruction that has one, and the outputs' widths in order
  void outputs(int mode, std::vector<uint32_t>& out_idx, std::vector<int>& widths) const {
    out_idx.assign(ins.size(), 0);
    widths.clear();
    for (size_t k = 0; k < ins.size(); ++k)
      if (is_output(ins[k].kind, mode)) {
        out_idx[k] = (uint32_t)widths.size();
        widths.push_back(is_q1_density(ins[k].kind) ? 4 : 16);
      }
  }
  size_t grad_size() const {
    size_t c = 0;
    for (auto& in : ins)
      if (is_var(in.kind)) c += gate_len(in.kind);
    return c;
  }

  // --- validation: the reference's panic order (circuit.rs:170-211, 221-263, 274-428) --------
  const char* validate_forward(const Flat& cg, const Flat& vg, std::vector<size_t>& gidx) const {
    if (ins.empty()) return fail("The circuit is empty.");
    size_t ci = 0, vi = 0;
    gidx.assign(ins.size(), 0);
    for (size_t k = 0; k < ins.size(); ++k) {
      const Instr& in = ins[k];
      if (is_const(in.kind)) {
        if (ci >= cg.size()) return fail("The number of constant gates is less than required.");
        gidx[k] = ci;
        QDC_TRY(check_gate(in, cg.len[ci], n));
        ++ci;
      } else if (is_var(in.kind)) {
        if (vi >= vg.size()) {
          // circuit.rs:198 / :249 report the constant-gate message for VarQ2GateDiag
          if (in.kind == QDC_VAR_Q2_DIAG)
            return fail("The number of constant gates is less than required.");
          return fail("The number of variable gates is less than required.");
        }
        gidx[k] = vi;
        QDC_TRY(check_gate(in, vg.len[vi], n));
        ++vi;
      } else {
        QDC_TRY(check_density_pos(in, n));
      }
    }
    if (ci != cg.size()) return fail("Number of constant gates is more than required.");
    if (vi != vg.size()) return fail("Number of variable gates is more than required.");
    return nullptr;
  }

  const char* validate_backward(const Flat& dg, const Flat& cg, const Flat& vg,
                                std::vector<size_t>& gidx) const {
    if (ins.empty()) return fail("The circuit is empty.");
    size_t ci = cg.size(), vi = vg.size(), di = dg.size();
    gidx.assign(ins.size(), 0);
    for (size_t kk = ins.size(); kk-- > 0;) {
      const Instr& in = ins[kk];
      if (is_const(in.kind)) {
        if (ci == 0) return fail("The number of gates is less than required.");
        --ci;
        gidx[kk] = ci;
        QDC_TRY(check_gate(in, cg.len[ci], n));
      } else if (is_var(in.kind)) {
        if (vi == 0) return fail("The number of gates is less than required.");
        --vi;
        gidx[kk] = vi;
        QDC_TRY(check_gate(in, vg.len[vi], n));
      } else if (is_diff_density(in.kind)) {
        if (di == 0)
          return fail("The number of gradients wrt density matrices is less than required.");
        --di;
        gidx[kk] = di;
        const size_t want = is_q1_density(in.kind) ? 4 : 16;
        if (dg.len[di] != want) return fail("Incorrect len of the gate's buffer.");
        QDC_TRY(check_density_pos(in, n));
      }
    }
    if (ci != 0) return fail("Number of constant gates is more than required.");
    // circuit.rs:426 reports leftover variable gates with the constant-gate message
    if (vi != 0) return fail("Number of constant gates is more than required.");
    if (di != 0)
      return fail("Number of gradients wrt density matrices is more than required.");
    return nullptr;
  }

  // --- remap: one all-to-all per state (see qdc_shard.hpp) --------------------------------
  // remap(r), or (inverse) its undoing: the all-to-all first (its block exchange, block j of
  // shard s <-> block s of shard j, is its own inverse), then the pack's inverse permutation.  A
  // mirrored reverse sweep undoes the forward's remaps in reverse order, so each of its passes
  // finds the physical layout its forward pass ran in.  (The layout follows in step_layout.)
  const char* remap(const qdc_plan_op& r, bool inverse, bool with_bwd) {
    const uint32_t low = nl - g;              // amplitude bits of one all-to-all block
    const size_t chunk = (size_t)1 << low;    // amplitudes per block
    for (int which = 0; which < (with_bwd ? 2 : 1); ++which) {
      std::vector<cx*> send(sh.size()), recv(sh.size());
      for (size_t s = 0; s < sh.size(); ++s) {
        cx*& buf = which == 0 ? sh[s].state : sh[s].bwd;
        if (r.pack && !inverse) {
          QDC_TRY(sh[s].c().use());
          QDC_TRY(pack(sh[s].c(), buf, sh[s].scratch, r.victims, g, nl));
          send[s] = sh[s].scratch;
          recv[s] = buf;
        } else {
          send[s] = buf;
          recv[s] = sh[s].scratch;
        }
      }
      QDC_TRY(ex.alltoall(sh, send, recv, chunk));
      for (size_t s = 0; s < sh.size(); ++s) {
        cx*& buf = which == 0 ? sh[s].state : sh[s].bwd;
        if (!r.pack) {
          std::swap(buf, sh[s].scratch);
        } else if (inverse) {
          QDC_TRY(sh[s].c().use());
          QDC_TRY(pack(sh[s].c(), sh[s].scratch, buf, r.victims, g, nl, true));
        }
      }
    }
    return nullptr;
  }

  std::vector<qdc_plan_op> plan(int mode) const {
    std::vector<PlanIn> ops;
    std::vector<int> index;
    active_ops(ins, mode, ops, index);
    QubitMap m = layout;
    std::vector<qdc_plan_op> out;
    // a mirrored forward's remap plan keeps both directions' order relations (its reverse is
    // the backward's plan)
    plan_pass(ops, index, m, out, mode == QDC_PLAN_BACKWARD, &inexact,
              mode == QDC_PLAN_FORWARD && mirror_on());
    return out;
  }

  struct Item : FusionItem {
    std::vector<std::vector<uint32_t>> stages;  // fused pass: its stages (stage_partition)
    // a mirrored backward pass: per stage the forward (item, stage) it undoes
    std::vector<std::pair<uint32_t, uint32_t>> mirror_of;
    size_t fop_off = 0;  // byte offset of the group's fop array in the pass program
    uint32_t nstage = 0;  // fop count (stages) of the pass
    double flops_per_amp = 0;  // algorithmic real FLOPs per amplitude of the pass
    bool has_red = false;      // reduction ops (Gamma stages or densities)
    bool writes_f = false;     // gate stages (fwd changes; else fwd is only read)
    std::vector<uint32_t> grad_slots;  // reduction slot of each reduction op, in op order
    bool rq = false;   // register-resident pass (qdc_rq.hpp): ops include relayouts
    const RqVariant* var = nullptr;  // rq: the kernel variant that runs it (qdc_variant.hpp)
    bool inv = false;  // an ITEM_REMAP run backwards: a mirrored backward undoing the forward's remap
    bool dens1 = false;  // a read-only pass of one-qubit densities only: k_dens1
    uint32_t l0 = 0;   // rq: matrix-area offset (cx) of the L0 layout descriptor
    uint32_t tbits = 0;  // amplitude bits of the tile
    SpecEntry* spec = nullptr;  // specialized kernel of the pass (qdc_jit.hpp), or none
  };
  // what a mirrored backward needs from the forward call: its schedule (plan after the
  // permuting passes' rewrites, items with stages), each gate stage's forward matrix (double,
  // in the forward's frame) and the gates and inexact flags it was built from
  struct MirrorRec {
    bool valid = false;
    std::vector<qdc_plan_op> plan;
    std::vector<Item> items;
    std::vector<std::vector<SMat>> stage_mats;  // [item][stage] (gate stages; else unused)
    std::vector<qdc_complex> cgates, vgates;
    std::vector<uint8_t> inexact;
    std::vector<uint32_t> end_phys;  // the layout the forward left
    void capture(const Flat& cg, const Flat& vg, const std::vector<qdc_plan_op>& pl,
                 const std::vector<Item>& its, std::vector<std::vector<SMat>>&& mats,
                 const std::vector<uint8_t>& inex) {
      plan = pl;
      items = its;
      stage_mats = std::move(mats);
      cgates.assign(cg.data, cg.data + cg.total());
      vgates.assign(vg.data, vg.data + vg.total());
      inexact = inex;
    }
    static bool same(const Flat& f, const std::vector<qdc_complex>& v) {
      const size_t nf = f.total();
      return nf == v.size() && (nf == 0 || std::memcmp(f.data, v.data(), nf * sizeof(qdc_complex)) == 0);
    }
    bool same_gates(const Flat& cg, const Flat& vg) const { return same(cg, cgates) && same(vg, vgates); }
  } mrec;
  // One execute() / backward() call: its arguments and everything the call's steps hand each
  // other — validation's indices, the planner, the schedule, the program's layout, the sweep's
  // progress.  Built at the top of the call; the steps below take it instead of member state.
  struct Call {
    const bool backward;
    const int mode;  // QDC_MODE_RUN / QDC_MODE_FORWARD; a backward: QDC_PLAN_BACKWARD
    // the schedule is a mirrored forward's (forward calls only: a run call has no backward to
    // mirror and keeps the one-state schedule; a backward's own schedule never depends on it)
    const bool mirror_fwd;
    const FusionPlanner P;  // the call's planner (Circuit::planner)
    const Flat *cg, *vg, *dg;  // the gates; backward: the cotangents (a schedule-only call: none)
    std::vector<size_t> gidx;                 // per instruction: index into cg / vg / dg
    std::vector<uint32_t> var_idx, out_idx;   // ... gradient row (backward), density slot (forward)
    uint32_t nvar = 0;
    std::vector<qdc_plan_op> plan;
    std::vector<Item> items;
    size_t first_inject = SIZE_MAX;  // backward: plan index of the first cotangent injection
    size_t mats_off = 0;             // byte offset of the program's matrix area
    bool have_bwd = false;           // backward: bwd holds a cotangent by now
    // a mirrored forward records each gate stage's matrix for its backward (MirrorRec)
    bool record = false;
    std::vector<std::vector<SMat>> stage_mats;
    std::vector<StagePost> stage_post;  // gradient recipes of the backward's Gamma stages
    size_t trace_start = 0;             // the call's first entry of `trace`
    hclock::time_point ht[6];           // host_record's stamps
    Call(const Circuit& c, int mode_, bool backward_, bool mirror, const Flat* cg_ = nullptr,
         const Flat* vg_ = nullptr, const Flat* dg_ = nullptr)
        : backward(backward_), mode(mode_), mirror_fwd(mirror && !backward_), P(c.planner(mirror_fwd)),
          cg(cg_), vg(vg_), dg(dg_), trace_start(c.trace.size()) {
      ht[0] = hclock::now();
    }
    const qdc_complex* gate(const Instr& in, size_t instr) const {
      return (is_const(in.kind) ? cg : vg)->at(gidx[instr]);
    }
    // the pass runs on both states (a backward's passes from its first injection on)
    bool two_state(const Item& it) const { return backward && it.ops[0] >= first_inject; }
  };
  // How an item changes a qubit layout: a remap applied or undone, then the swaps of a permuting
  // pass (it stored its tile's qubits at new positions; later ops were planned so).  The one
  // statement of it: the sweeps (live and dry), trace_logical and qdc_check_schedule use it.
  static void step_layout(QubitMap& m, const Item& it, const std::vector<qdc_plan_op>& pl) {
    if (it.type == ITEM_REMAP) {
      if (it.inv)
        m.unapply(pl[it.ops[0]].victims);
      else
        m.apply(pl[it.ops[0]].victims);
    }
    for (const auto& sw : it.swaps) m.swap_phys(sw.first, sw.second);
  }
  // The backward schedule as the forward's passes run in reverse (mirror mode): op positions
  // mapped into the layout each reverse pass starts from (the forward pass's store layout),
  // stages and the ops in them reversed, the forward's swaps undone in reverse order.
  bool mirror_schedule(Call& c) const {
    std::vector<qdc_plan_op>& pl = c.plan;
    std::vector<Item>& items = c.items;
    auto is_meas = [&](const qdc_plan_op& op) { return c.P.is_meas(op); };
    pl.clear();
    items.clear();
    const std::vector<Item>& F = mrec.items;
    for (size_t k = F.size(); k-- > 0;) {
      const Item& f = F[k];
      if (f.type != ITEM_OP && f.type != ITEM_REMAP && f.type != ITEM_FUSED) return false;
      auto push = [&](uint32_t fi) {
        qdc_plan_op op = mrec.plan[fi];
        if (op.type == QDC_PLAN_OP) {
          op.pos2 = apply_swaps(f.swaps, op.pos2);
          op.pos1 = apply_swaps(f.swaps, op.pos1);
        }
        pl.push_back(op);
        return (uint32_t)(pl.size() - 1);
      };
      auto shell = [&]() {
        Item b;
        b.type = ITEM_FUSED;
        b.lc = f.lc;
        b.h = f.h;
        for (uint32_t r = 0; r < (uint32_t)FMAX_ROWS; ++r) b.hb[r] = f.hb[r];
        return b;
      };
      if (f.type != ITEM_FUSED) {  // a single op, or a remap undone
        Item b;
        b.type = f.type;
        b.inv = f.type == ITEM_REMAP;
        b.ops.push_back(push(f.ops[0]));
        items.push_back(std::move(b));
        continue;
      }
      // the pass's densities (its last stages) become the injections that open its reverse
      // pass (one injection pass; a single one stays a single op), then its gate stages in
      // reverse with the forward's swaps undone in reverse order
      size_t ng = f.stages.size();
      while (ng > 0 && is_meas(mrec.plan[f.stages[ng - 1][0]])) --ng;
      for (size_t j = ng; j < f.stages.size(); ++j)
        for (uint32_t fi : f.stages[j])
          if (!is_meas(mrec.plan[fi])) return false;  // (the planner keeps densities last)
      if (ng < f.stages.size()) {
        Item m = shell();
        for (size_t j = f.stages.size(); j-- > ng;) {
          const uint32_t bi = push(f.stages[j][0]);
          m.ops.push_back(bi);
          m.stages.push_back({bi});
        }
        if (m.ops.size() == 1) {
          m.type = ITEM_OP;
          m.stages.clear();
        }
        items.push_back(std::move(m));
      }
      if (ng == 0) continue;
      Item b = shell();
      for (auto it = f.swaps.rbegin(); it != f.swaps.rend(); ++it) b.swaps.push_back(*it);
      for (size_t j = ng; j-- > 0;) {
        std::vector<uint32_t> st;
        for (size_t t = f.stages[j].size(); t-- > 0;) {
          if (is_meas(mrec.plan[f.stages[j][t]])) return false;
          const uint32_t bi = push(f.stages[j][t]);
          st.push_back(bi);
          b.ops.push_back(bi);
        }
        b.stages.push_back(std::move(st));
        b.mirror_of.push_back({(uint32_t)k, (uint32_t)j});
      }
      items.push_back(std::move(b));
    }
    c.first_inject = first_injection(pl);
    return true;
  }
  // plan index of the first cotangent injection (the ops before it only uncompute fwd), or the
  // plan's size
  size_t first_injection(const std::vector<qdc_plan_op>& pl) const {
    for (size_t i = 0; i < pl.size(); ++i)
      if (pl[i].type == QDC_PLAN_OP && is_diff_density(ins[pl[i].instr].kind)) return i;
    return pl.size();
  }
  static constexpr uint32_t TILE_CHUNKS_1 = FusionPlanner::TILE_CHUNKS_1;
  static constexpr uint32_t TILE_CHUNKS_2 = FusionPlanner::TILE_CHUNKS_2;
  FusionPlanner planner(bool mirror_fwd) const {
    FusionPlanner P{ins, inexact, nl, k.fuse != 0, k.fuse_meas != 0, k.fuse_max_ops, k.fuse_lcmin};
    // gate-only passes permute their tile on the way out when they are register-resident
    // (sharded circuits too, round 5: later remaps' victims are relabelled, qdc_fusion.hpp
    // relabel_remap; QDC_RQ_PERM_SHARD=0 keeps their layouts fixed)
    P.permute = k.rq_permute && k.use_rq && (g == 0 || k.rq_perm_shard) && sizeof(real) == 4;
    P.ng = g;
    P.rq_grad = k.rq_grad32 && k.use_rq && (sizeof(real) == 4 || k.rq64);
    P.gamma_cap = k.rq_gcap;
    if (k.rq_perm_low) P.perm_low = k.rq_perm_low;
    P.tile1_chunks = k.tile1_chunks;
    P.mirror = mirror_on() && mirror_fwd;
    P.defer_q1 = k.defer_q1 != 0;
    P.search = k.fuse_search != 0;
    P.gamma_stage_cap = k.rq_gstage != 0;
    P.split_dens = k.dens_split != 0;
    return P;
  }
  void fuse_items(Call& c) const {
    c.items.clear();
    for (FusionItem& f : c.P.fuse_items(c.plan, c.backward, c.first_inject)) {
      Item it;
      static_cast<FusionItem&>(it) = std::move(f);
      if (it.type == ITEM_FUSED) it.stages = c.P.stage_partition(it.ops, c.plan, c.backward);
      c.items.push_back(std::move(it));
    }
  }
  // The pass schedule of a call (fuse_items + stage_partition, ~1-2 ms at C2 n = 28) depends on
  // the plan, the inexact flags and the mode only, not on the gate values: the last schedule
  // per direction is kept and reused when those are unchanged (QDC_SCHED_CACHE=0: off).
  struct SchedCache {
    bool valid = false;
    size_t first_inject = 0;
    bool mirror = false;
    std::vector<qdc_plan_op> in_plan, out_plan;
    std::vector<uint8_t> inexact;
    std::vector<Item> items;
  };
  SchedCache sched_cache[2];  // forward / run, backward
  static bool same_plan(const std::vector<qdc_plan_op>& a, const std::vector<qdc_plan_op>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
      const qdc_plan_op &x = a[i], &y = b[i];
      if (x.type != y.type || x.instr != y.instr || x.pos2 != y.pos2 || x.pos1 != y.pos1 ||
          x.nvictims != y.nvictims || x.pack != y.pack)
        return false;
      for (unsigned k = 0; k < x.nvictims && k < 8; ++k)
        if (x.victims[k] != y.victims[k]) return false;
    }
    return true;
  }
  // c.plan (rewritten by the permuting passes) and c.first_inject into c.items
  void schedule(Call& c) {
    SchedCache& sc = sched_cache[c.backward ? 1 : 0];
    if (k.sched_cache_on && sc.valid && sc.first_inject == c.first_inject && sc.inexact == inexact &&
        sc.mirror == c.mirror_fwd && same_plan(sc.in_plan, c.plan)) {
      c.plan = sc.out_plan;
      c.items = sc.items;
      return;
    }
    sc.valid = false;
    sc.in_plan = c.plan;
    fuse_items(c);
    if (k.sched_cache_on) {
      sc.out_plan = c.plan;
      sc.items = c.items;
      sc.inexact = inexact;
      sc.first_inject = c.first_inject;
      sc.mirror = c.mirror_fwd;
      sc.valid = true;
    }
  }
  // register-layout plans of passes (rq_plan, ~20 us each), by the pass's stages and tile
  std::map<std::vector<uint64_t>, RqPlan> rq_plan_cache;
  const RqPlan& rq_plan_cached(const std::vector<RqStage>& rs, uint32_t tbits, const uint32_t* src,
                               bool maxcl, uint32_t ns, bool keep = false) {
    std::vector<uint64_t> key = {tbits, ns, (maxcl ? 1u : 0u) | (keep ? 2u : 0u), src ? 1u : 0u};
    if (src)
      for (int i = 0; i < 4; ++i) key.push_back(src[i]);
    for (const RqStage& r : rs) {
      key.push_back(((uint64_t)r.kind << 48) | ((uint64_t)r.t1 << 24) | r.t2);
      key.push_back(r.deps);
    }
    auto it = rq_plan_cache.find(key);
    if (it != rq_plan_cache.end()) return it->second;
    if (rq_plan_cache.size() >= 8192) rq_plan_cache.clear();
    return rq_plan_cache.emplace(std::move(key), rq_plan(rs, tbits, src, maxcl, ns, keep)).first->second;
  }
  // per call: which gates are not unitary to working precision (qdc_fusion.hpp)
  void mark_inexact(const Flat& cg, const Flat& vg, const std::vector<size_t>& gidx) {
    inexact.assign(ins.size(), 0);
    const double utol = sizeof(real) == 4 ? 1e-6 : 1e-13;
    for (size_t k = 0; k < ins.size(); ++k)
      if (is_const(ins[k].kind) || is_var(ins[k].kind)) {
        const qdc_complex* g4 = is_const(ins[k].kind) ? cg.at(gidx[k]) : vg.at(gidx[k]);
        inexact[k] = unitarity_error(g4, ins[k].kind) > utol ? 1 : 0;
      }
  }
  // max |U^+ U - I| of a gate's host matrix (diagonal: max ||d_i|^2 - 1|)
  static double unitarity_error(const qdc_complex* g, int kind) {
    if (is_diag(kind)) {
      double e = 0;
      for (int i = 0; i < 4; ++i) {
        const double m = (double)g[i].re * g[i].re + (double)g[i].im * g[i].im;
        e = std::max(e, std::abs(m - 1.0));
      }
      return e;
    }
    const int R = is_q1_gate(kind) ? 2 : 4;
    double e = 0;
    for (int p = 0; p < R; ++p)
      for (int q = 0; q < R; ++q) {
        double re = 0, im = 0;  // (U^+ U)[p][q] = sum_k conj(U[k][p]) U[k][q]
        for (int k = 0; k < R; ++k) {
          const qdc_complex a = g[k * R + p], b = g[k * R + q];
          re += (double)a.re * b.re + (double)a.im * b.im;
          im += (double)a.re * b.im - (double)a.im * b.re;
        }
        e = std::max(e, std::hypot(re - (p == q ? 1.0 : 0.0), im));
      }
    return e;
  }
  // --- the pass program: build_program and its steps --------------------------------------------
  // One stage op of the pass being built: the op as the LDS kernel takes it, its qubits (a mask
  // of physical positions), its order classes (qdc_fusion.hpp) and its reduction slot (Gamma
  // stages), else -1
  struct StageOp {
    fop F;
    uint64_t q;
    uint32_t cls;
    int slot;
  };
  // One build_program call: the call it builds for, the write cursors of the program (fo fops
  // and mo matrix values so far, the next Gamma slot) and the per-pass scratch, reserved once and
  // reused
  struct Build {
    Call& c;
    fop* fops;
    cx* mats;
    size_t fo, mo;
    uint32_t next_slot;
    std::vector<StageOp> ops;        // the pass's stage ops in program order
    std::vector<StageGateIn> gates;  // the gates of the stage being composed
    std::vector<RqStage> rs;
    std::vector<SpecStep> sst;
    std::vector<uint32_t> key;
  };
  // Lay out every fused pass's stage descriptors and stage matrices (A = product of the
  // applied matrices, B = product of the bwd pull-backs) in one pinned buffer, then upload it.
  // backward: `first_inject` = plan index of the first cotangent injection (passes before it
  // only uncompute fwd); gradient stages get slots nvar, nvar+1, ... of the gradient buffer and
  // a recipe in c.stage_post (qdc_stage.hpp).
  // forward: densities reduce into dens slot out_idx[instr]; backward: injections read their
  // cotangent from dg.
  const char* build_program(Call& c) {
    std::vector<Item>& items = c.items;
    if (spec_cache.size() >= 4096 && !dry) spec_cache.clear();  // bounded; items of this call point into it
    size_t nops = 0;
    for (const Item& it : items)
      if (it.type == ITEM_FUSED) nops += it.stages.size();
    if (nops == 0) return nullptr;
    QDC_TRY(reserve_program(nops, items.size(), c.mats_off));
    Build B{c, reinterpret_cast<fop*>(prog_host), reinterpret_cast<cx*>(prog_host + c.mats_off), 0, 0,
            c.nvar, {}, {}, {}, {}, {}};
    B.ops.reserve(k.fuse_max_ops);
    B.gates.reserve(k.fuse_max_ops);
    B.rs.reserve(k.fuse_max_ops);
    B.sst.reserve(2 * (size_t)k.fuse_max_ops + 1);
    for (size_t ii = 0; ii < items.size(); ++ii) {
      Item& it = items[ii];
      if (it.type != ITEM_FUSED) continue;
      const bool two = c.two_state(it);
      QDC_TRY(build_stages(B, it, ii, two));
      QDC_TRY(classify_pass(B, it, two));
      if (it.rq)
        QDC_TRY(emit_rq_pass(B, it, two));
      else
        emit_lds_pass(B, it);
    }
    if (dry) {  // the kernels this call would compile / load
      for (Item& it : items)
        if (it.spec && std::find(dry_specs.begin(), dry_specs.end(), it.spec) == dry_specs.end())
          dry_specs.push_back(it.spec);
      return nullptr;
    }
    for (auto& d : devs) {  // prog_host is not rewritten before the call's final sync
      QDC_TRY(d->ctx.use());
      QDC_HIP(hipMemcpyAsync(d->prog_dev, prog_host, c.mats_off + B.mo * sizeof(cx),
                             hipMemcpyHostToDevice, d->ctx.stream));
    }
    return spec_load(items);
  }
  // Step 1: size the program of nops stages in nitems items and, where it outgrew them,
  // reallocate the pinned staging buffer and every device's copy (a dry run: dry_prog)
  const char* reserve_program(size_t nops, size_t nitems, size_t& mats_off) {
    // register-resident passes add relayout ops (<= one per stage, plus the return to L0) and
    // 12-cx layout descriptors (one per relayout, plus L0)
    const size_t nfops = 2 * nops + nitems;
    mats_off = ((nfops * sizeof(fop) + 255) / 256) * 256;
    // matrices <= 2 R^2 = 32 per stage; layouts <= 12 cx; one rqio per register-resident pass
    const size_t bytes =
        mats_off + (nops * 32 + nfops * (sizeof(rq_layout) / sizeof(cx)) +
                    nitems * (sizeof(rqio) / sizeof(cx))) *
                       sizeof(cx);
    if (dry && bytes > prog_cap) {
      dry_prog.resize(bytes);
      prog_host = dry_prog.data();
      prog_cap = bytes;
    }
    if (bytes > prog_cap) {
      QDC_TRY(sync_all());
      for (auto& d : devs) {
        QDC_TRY(d->ctx.use());
        if (d->prog_dev) QDC_HIP(hipFree(d->prog_dev));
        d->prog_dev = nullptr;
        QDC_HIP(hipMalloc(&d->prog_dev, bytes));
      }
      if (prog_host) QDC_HIP(hipHostFree(prog_host));
      prog_host = nullptr;
      QDC_HIP(hipHostMalloc(&prog_host, bytes));
      prog_cap = bytes;
    }
    return nullptr;
  }
  // the tile-local amplitude bit of physical position p in the pass's tile
  static uint32_t local_bit(const Item& it, uint32_t p) {
    if (p < (uint32_t)LV + it.lc) return p;
    for (uint32_t r = 0; r < it.h; ++r)
      if (it.hb[r] == p - LV) return LV + it.lc + r;
    return 0xffffffffu;  // unreachable: tile_config covered every bit
  }
  // Step 2: the pass's stage ops into B.ops, their matrices into the matrix area
  const char* build_stages(Build& B, Item& it, size_t ii, bool two) {
    it.fop_off = B.fo * sizeof(fop);
    it.grad_slots.clear();
    it.flops_per_amp = 0;
    it.has_red = false;
    it.writes_f = false;
    B.ops.clear();
    const Call& c = B.c;
    const FusionPlanner& PL = c.P;
    for (size_t sj = 0; sj < it.stages.size(); ++sj) {
      const auto& st = it.stages[sj];
      StageOp so{fop{}, 0, 0, -1};
      for (uint32_t pi : st) {
        so.q |= (1ull << c.plan[pi].pos2) | (1ull << c.plan[pi].pos1);
        so.cls |= PL.op_class(c.plan[pi], c.backward);
      }
      B.ops.push_back(so);
      if (PL.is_meas(c.plan[st[0]]))
        measure_stage(B, it, ii, c.plan[st[0]]);
      else
        QDC_TRY(gate_stage(B, it, ii, sj, two));
    }
    return nullptr;
  }
  // a density (forward) or a cotangent injection (backward)
  void measure_stage(Build& B, Item& it, size_t ii, const qdc_plan_op& op) {
    if (B.c.record) B.c.stage_mats[ii].push_back(smat_identity(2));
    const bool q1 = is_q1_density(ins[op.instr].kind);
    const int R = q1 ? 2 : 4;
    fop& F = B.ops.back().F;
    F.t1 = local_bit(it, q1 ? op.pos2 : op.pos1);
    F.t2 = local_bit(it, op.pos2);
    F.mat = (uint32_t)B.mo;
    cx* m = B.mats + B.mo;
    for (int i = 0; i < 2 * R * R; ++i) m[i] = cx{0, 0};
    if (B.c.backward) {  // b += (G^T on pos) (2 conj f), G = conj of the JAX cotangent
      F.kind = q1 ? FK_INJ1 : FK_INJ2;
      const qdc_complex* gd = B.c.dg->at(B.c.gidx[op.instr]);
      if (q1) {
        const mat<2> t = transpose<2>(to_mat<2>(gd));
        for (int i = 0; i < 4; ++i) m[i] = t.a[i];
      } else {
        const mat<4> t = transpose<4>(to_mat<4>(gd));
        for (int i = 0; i < 16; ++i) m[i] = t.a[i];
      }
    } else {
      F.kind = q1 ? FK_DENS1 : FK_DENS2;
      it.grad_slots.push_back(B.c.out_idx[op.instr]);
      it.has_red = true;
    }
    it.flops_per_amp += 8.0 * (q1 ? 2.0 : 4.0);
    B.mo += 2 * R * R;
  }
  // a stage of gates: compose it (qdc_stage.hpp), take the forward's adjoint where the pass
  // mirrors one, record it for the trace, write its matrices A and B
  const char* gate_stage(Build& B, Item& it, size_t ii, size_t sj, bool two) {
    Call& c = B.c;
    const auto& st = it.stages[sj];
    // stage qubits (physical positions), lo < hi
    const uint64_t qm = B.ops.back().q;
    const uint32_t lo = (uint32_t)__builtin_ctzll(qm);
    const uint32_t hi = 63u - (uint32_t)__builtin_clzll(qm);
    const int R = lo == hi ? 2 : 4;
    bool any_grad = false;
    B.gates.clear();
    for (uint32_t pi : st) {
      const qdc_plan_op& op = c.plan[pi];
      const Instr& in = ins[op.instr];
      GateMats M;
      QDC_TRY(gate_mats(in.kind, c.gate(in, op.instr), c.backward, M));
      B.gates.emplace_back();
      StageGateIn& g = B.gates.back();
      for (int i = 0; i < M.count(); ++i) {
        g.a[i] = cd(M.a[i].x, M.a[i].y);
        g.b[i] = cdd(M.b[i].x, M.b[i].y);
      }
      g.diag = M.diag;
      g.role = stage_role(R, is_q1_gate(in.kind), op.pos2, lo, hi);
      const bool grad = two && is_var(in.kind);
      g.var = grad ? (int)c.var_idx[op.instr] : -1;
      any_grad = any_grad || grad;
    }
    SMat A;
    SMatD Bp;
    StagePost post;
    stage_compose(B.gates.data(), B.gates.size(), R, A, Bp, post);
    const bool all_diag = post.diag_only;
    if (c.record) c.stage_mats[ii].push_back(A);  // the forward's matrix, its own frame
    SMat Aup = A;
    const bool from_fwd = c.backward && mirror_adjoint(c.plan, it, sj, R, Aup);
    if (tracing) {  // (physical positions; trace_logical maps them to logical qubits)
      TraceOp t{c.backward ? 1u : 0u, (uint32_t)ii, hi, lo, (uint32_t)R, all_diag ? 1u : 0u,
                from_fwd ? 1u : 0u, 0u, {}};
      for (int i = 0; i < R * R; ++i) {
        const bool keep = !all_diag || i % (R + 1) == 0;
        t.m[i].re = keep ? (qdc_real)(real)Aup.a[i].real() : 0;
        t.m[i].im = keep ? (qdc_real)(real)Aup.a[i].imag() : 0;
      }
      trace.push_back(t);
    }
    fop& F = B.ops.back().F;
    F.t1 = local_bit(it, lo);
    F.t2 = local_bit(it, hi);
    F.mat = (uint32_t)B.mo;
    F.kind = (all_diag ? FK_DIAG : (R == 2 ? FK_Q1 : FK_Q2)) | (any_grad ? FOP_GAMMA : 0u);
    it.writes_f = true;
    const int nm = all_diag ? 4 : R * R;
    cx* m = B.mats + B.mo;
    for (int i = 0; i < nm; ++i) {
      const cd va = all_diag ? Aup.a[i * 4 + i] : Aup.a[i];
      const cdd vb = all_diag ? Bp.a[i * 4 + i] : Bp.a[i];
      m[i] = cx{(real)va.real(), (real)va.imag()};
      m[nm + i] = cx{(real)vb.real(), (real)vb.imag()};
    }
    B.mo += 2 * nm;
    // complex MACs per amplitude: 1 (diagonal), 2 (one qubit), 4 (two qubits) per matrix
    // applied (A; B too when two-state) and per Gamma accumulated; 8 real FLOPs each
    const double cmac = all_diag ? 1.0 : (R == 2 ? 2.0 : 4.0);
    it.flops_per_amp += 8.0 * cmac * ((two ? 2.0 : 1.0) + (any_grad ? 1.0 : 0.0));
    if (any_grad) {
      post.slot = B.next_slot++;
      it.grad_slots.push_back(post.slot);
      B.ops.back().slot = (int)post.slot;
      it.has_red = true;
      c.stage_post.push_back(std::move(post));
    }
    return nullptr;
  }
  // A mirrored backward stage of unitary gates uncomputes with exactly the adjoint of the matrix
  // its forward stage applied (same rounding: Aup, true), where the forward recorded one of this
  // basis.  The forward frame's two qubits may have swapped order under the forward pass's
  // permutation: swapped when the forward's lower qubit now sits above the other.
  bool mirror_adjoint(const std::vector<qdc_plan_op>& plan, const Item& it, size_t sj, int R,
                      SMat& Aup) const {
    if (it.mirror_of.empty()) return false;
    for (uint32_t pi : it.stages[sj])
      if (is_nonu(ins[plan[pi].instr].kind)) return false;
    const auto& of = it.mirror_of[sj];
    if (of.first >= mrec.stage_mats.size() || of.second >= mrec.stage_mats[of.first].size())
      return false;
    const SMat& Pf = mrec.stage_mats[of.first][of.second];
    if (Pf.R != R) return false;
    const Item& f = mrec.items[of.first];
    uint32_t flo = 64, fhi = 0;
    for (uint32_t fi : f.stages[of.second]) {
      const qdc_plan_op& fo = mrec.plan[fi];
      flo = std::min({flo, fo.pos2, fo.pos1});
      fhi = std::max({fhi, fo.pos2, fo.pos1});
    }
    Aup = stage_mirror_adjoint(Pf, R == 4 && apply_swaps(f.swaps, flo) > apply_swaps(f.swaps, fhi));
    return true;
  }
  // Step 3: which kernel runs the pass.  Register-resident: gate stages only (no densities /
  // injections), f32 or rq64; else the LDS kernel, or k_dens1 for a read-only pass of one-qubit
  // densities.
  const char* classify_pass(const Build& B, Item& it, bool two) const {
    bool rq = k.use_rq && (sizeof(real) == 4 || k.rq64) && it.writes_f;
    for (const StageOp& o : B.ops) rq = rq && (o.F.kind & 7u) <= FK_DIAG;
    it.rq = rq;
    if (!it.swaps.empty() && !rq)
      return fail("internal: a permuting fused pass is not register-resident");
    it.tbits = (uint32_t)LV + it.lc + it.h;
    // the kernels index their per-wave accumulators by reduction op: a pass with more
    // reduction ops than accumulators is a planner bug, never folded into another slot
    const size_t nred = it.grad_slots.size();
    // (the kernels' storage bound; the planner's cap, k.rq_gcap, lies within it)
    const size_t cap = rq ? (size_t)FMAX_GRAD_RQ : (size_t)FMAX_GRAD;
    if (nred > cap)
      return fail("internal: a fused pass has %zu reduction ops, the kernel holds %zu", nred, cap);
    if (rq) return nullptr;
    bool d1 = k.dens1_kernel && !two && !it.writes_f && !B.ops.empty() && B.ops.size() <= (size_t)DENS1_MAX;
    for (const StageOp& o : B.ops) d1 = d1 && (o.F.kind & 7u) == FK_DENS1;
    it.dens1 = d1;
    return nullptr;
  }
  // Step 4, LDS kernel: the stage ops as they are
  static void emit_lds_pass(Build& B, Item& it) {
    for (const StageOp& o : B.ops) B.fops[B.fo++] = o.F;
    it.nstage = (uint32_t)B.ops.size();
  }
  uint32_t put_layout(Build& B, const RqLayout& L, uint32_t tbits) const {
    const rq_layout d = rq_descriptor(L, tbits);
    const uint32_t off = (uint32_t)B.mo;
    std::memcpy(&B.mats[B.mo], &d, sizeof d);
    B.mo += sizeof(rq_layout) / sizeof(cx);
    return off;
  }
  // Step 4, register-resident kernel: the stages' dependencies, the kernel variant, the
  // register-layout plan (rq_plan), the load descriptor and the HBM address tables (rqio), then
  // the plan's steps — relayouts with their descriptors, stages with their slot case
  const char* emit_rq_pass(Build& B, Item& it, bool two) {
    B.rs.clear();
    for (size_t k = 0; k < B.ops.size(); ++k) {
      const StageOp& ok = B.ops[k];
      RqStage r{ok.F.kind & 7u, ok.F.t1, ok.F.t2, 0};
      for (size_t i = 0; i < k; ++i)
        if ((B.ops[i].q & ok.q) || (FusionPlanner::conflicts_of(B.ops[i].cls) & ok.cls) ||
            (FusionPlanner::conflicts_of(ok.cls) & B.ops[i].cls))
          r.deps |= 1ull << i;
      B.rs.push_back(r);
    }
    // a permuting pass: tile bit t's value is stored where tile bit dest[t] sits
    uint32_t dest[32], src[4] = {0, 1, 2, 3};
    const bool perm = !it.swaps.empty();
    if (perm) {
      for (uint32_t t = 0; t < it.tbits; ++t) {
        const uint32_t p = t < (uint32_t)LV + it.lc ? t : (uint32_t)LV + it.hb[t - LV - it.lc];
        dest[t] = local_bit(it, apply_swaps(it.swaps, p));
        if (dest[t] < 4) src[dest[t]] = t;
      }
    }
    // the kernel variant that will run the pass: the plan's register slots come from it
    QDC_TRY(rq_variant(two, it.tbits, it.var));
    const RqVariant& V = *it.var;
    const RqPlan& P = rq_plan_cached(B.rs, it.tbits, perm ? src : nullptr, k.rq_maxcl != 0, V.ns,
                                     rq_keep(V, k.spec_half != 0));
    it.l0 = put_layout(B, P.load, it.tbits);
    {  // rqio after the load descriptor
      rqio io{};
      rq_hbm(P.load, it.tbits, it.lc, it.hb, io.gv_ld, io.offi_ld);
      rq_hbm(P.store, it.tbits, it.lc, it.hb, io.gv_st, io.offi_st, perm ? dest : nullptr);
      // gapped offsets (interleaved pair): the kernel gaps only the tile base, and the gap
      // is linear over the disjoint bit sets of base, thread and register offsets
      for (uint64_t* a : {io.gv_ld, io.gv_st})
        for (int k = 0; k < 8; ++k) a[k] += a[k] & gm;
      for (uint64_t* a : {io.offi_ld, io.offi_st})
        for (int k = 0; k < RQ_R; ++k) a[k] += a[k] & gm;
      std::memcpy(&B.mats[B.mo], &io, sizeof io);
      B.mo += sizeof(rqio) / sizeof(cx);
    }
    uint32_t nfop = 0;
    it.grad_slots.clear();  // the kernel reduces Gamma stages in execution order
    // the variant's specialized pass (one-state passes: QDC_SPEC_FWD)
    const bool spec = V.prefix && spec_on() && (two || k.spec_fwd);
    B.sst.clear();
    RqLayout lcur = P.load;
    for (const RqStep& step : P.steps) {
      fop F{};
      if (step.relayout) {
        F.kind = FK_RELAYOUT;
        F.mat = put_layout(B, step.L, it.tbits);
        if (spec) B.sst.push_back(SpecStep{true, lcur, step.L, F});
        lcur = step.L;
      } else {
        const int slot = B.ops[step.stage].slot;
        if (slot >= 0) it.grad_slots.push_back((uint32_t)slot);
        F = B.ops[step.stage].F;
        F.t2 = 0;
        // the canonical slot case (rq_slot_case): where it exchanged the slots, exchange them
        // in the matrices by permuting their index bits, and the stage's Gamma back on the host
        bool swapped = false;
        F.t1 = rq_slot_case(F.kind, step.cs, swapped);
        if (swapped) {
          stage_swap_slots(&B.mats[F.mat], (F.kind & 7u) == FK_DIAG);
          if (slot >= 0)
            for (StagePost& sp : B.c.stage_post)
              if (sp.slot == (uint32_t)slot) sp.swapped = true;
        }
        if (spec) B.sst.push_back(SpecStep{false, lcur, lcur, F});
      }
      B.fops[B.fo++] = F;
      ++nfop;
    }
    it.nstage = nfop;
    it.spec = spec ? spec_entry(B, V, it.tbits, P.load) : nullptr;
    if (k.rq_stats)
      fprintf(stderr, "rq pass: %zu stages, %u ops (T=%u lc=%u)\n", B.ops.size(), nfop, it.tbits, it.lc);
    if (k.rq_stats >= 2) {  // the pass's stages for offline planner studies (tools/)
      fprintf(stderr, "rq stages %s T=%u perm=%d:", two ? "two" : "one", it.tbits, perm ? 1 : 0);
      for (const RqStage& r : B.rs)
        fprintf(stderr, " %u,%u,%u,%llx", r.kind, r.t1, r.t2, (unsigned long long)r.deps);
      fprintf(stderr, "\n");
    }
    return nullptr;
  }
  // Step 5: the specialized kernel of the pass whose steps are B.sst, from spec_cache.  The
  // source is generated once per distinct program (per process): the key is everything it
  // depends on, the layouts, stage kinds, slot cases and Gamma flags
  SpecEntry* spec_entry(Build& B, const RqVariant& V, uint32_t tbits, const RqLayout& load) {
    const bool half = spec_half_buffer(V, k.spec_half != 0, B.sst);
    std::vector<uint32_t>& key = B.key;
    key.assign({(uint32_t)(&V - rq_variants()), tbits, spec_imm() ? 1u : 0u, half ? 1u : 0u});
    auto put_layout_key = [&](const RqLayout& L) {
      key.push_back(L.ns | (L.tfix ? 0x100u : 0u));
      for (uint32_t q = 0; q < RQ_SLOTS_MAX; ++q) key.push_back(L.slot[q]);
      for (int q = 0; q < 3; ++q) key.push_back(L.tfirst[q]);
    };
    put_layout_key(load);
    for (const SpecStep& ss : B.sst) {
      if (ss.relayout) {
        key.push_back(0xffffffffu);
        put_layout_key(ss.Ln);
      } else {
        key.push_back(ss.F.kind);
        key.push_back(ss.F.t1);
      }
    }
    auto hit = spec_cache.find(key);
    if (hit == spec_cache.end())
      hit = spec_cache.emplace(key, spec_kernel_of(B.sst, V, tbits, half)).first;
    return &hit->second;
  }
  // specialized passes: circuits of >= spec_min_qubits local qubits (every shard runs the same
  // program; the kernels are loaded on each shard's device)
  bool spec_on() const { return k.spec_mode > 0 && (k.spec_mode >= 2 || nl >= k.spec_min_qubits); }
  // compile / load the kernels of this program's specialized passes (more distinct ones than
  // spec_max — deep random circuits would compile for minutes — go to the background compiler)
  const char* spec_load(std::vector<Item>& items) {
    if (items.empty()) return nullptr;
    size_t distinct = 0;
    ++spec_epoch;
    for (Item& it : items)
      if (it.spec && it.spec->epoch != spec_epoch) {
        it.spec->epoch = spec_epoch;
        ++distinct;
      }
    if (distinct == 0) return nullptr;
    const bool async = distinct > k.spec_max;
    if (async && !k.spec_async) {  // every pass of this call interpreted
      for (Item& it : items) it.spec = nullptr;
      return nullptr;
    }
    std::vector<int> devs;
    for (auto& s : sh)
      if (std::find(devs.begin(), devs.end(), s.c().device) == devs.end()) devs.push_back(s.c().device);
    for (size_t di = 0; di < devs.size(); ++di) {
      const int dev = devs[di];
      std::vector<SpecEntry*> todo;  // distinct kernels not loaded on dev yet
      ++spec_epoch;
      for (Item& it : items)
        if (it.spec && it.spec->epoch != spec_epoch) {
          it.spec->epoch = spec_epoch;
          if (!it.spec->fn.count(dev)) todo.push_back(it.spec);
        }
      if (todo.empty()) continue;
      std::vector<std::string> names, srcs;
      for (const SpecEntry* e : todo) {
        names.push_back(e->name);
        srcs.push_back(e->src);
      }
      for (auto& s : sh)
        if (s.c().device == dev) {
          QDC_TRY(s.c().use());
          break;
        }
      std::vector<hipFunction_t> fns;
      if (async)  // (what is compiled loads now, the rest compiles in the background)
        SpecJit::get().ensure_async(dev, names, srcs, fns);
      else
        SpecJit::get().ensure(dev, names, srcs, fns);
      for (size_t k = 0; k < todo.size(); ++k)
        if (fns[k]) todo[k]->fn[dev] = fns[k];
    }
    return nullptr;
  }
  // the pass's specialized kernel on a device, or none (the interpreted kernel runs)
  static hipFunction_t spec_fn_on(const Item& it, int dev) {
    if (!it.spec) return nullptr;
    auto f = it.spec->fn.find(dev);
    return f == it.spec->fn.end() ? nullptr : f->second;
  }
  // What a fused launch used, handed back to run_fused, which commits the pass's reduction
  // slots with it
  struct GridUse {
    uint32_t grid = 0;  // the blocks launched (size_grid's input: the resident blocks)
    uint32_t ndyn = 0;  // granule partials per slot
  };
  // Run one fused group on every shard.  grads != nullptr: two-state reverse program whose
  // gradient gates write partials for gradient buffer rows var_idx[...].
  template <bool TWO, bool HASRED, bool WF>
  const char* launch_fused(Ctx& ctx, const char* name, double bytes, const fgeo& fg, chunk* f,
                           chunk* b, const fop* fops, const cx* mats, cx* partials,
                           uint64_t stride, GridUse& use) {
    // one-state passes on the smaller tile (QDC_TILE1_CHUNKS = TILE_CHUNKS_2): the LDS kernel
    // of that tile size (a k_fused tile is always TB chunks)
    if constexpr (!TWO) {
      if ((1ull << (fg.lc + fg.h)) == TILE_CHUNKS_2)
        return launch_fused_tb<TWO, HASRED, WF, (int)TILE_CHUNKS_2>(ctx, name, bytes, fg, f, b, fops,
                                                                    mats, partials, stride, use);
    }
    constexpr int TB = TWO ? (int)TILE_CHUNKS_2 : (int)TILE_CHUNKS_1;
    return launch_fused_tb<TWO, HASRED, WF, TB>(ctx, name, bytes, fg, f, b, fops, mats, partials, stride,
                                                use);
  }
  template <bool TWO, bool HASRED, bool WF, int TB>
  const char* launch_fused_tb(Ctx& ctx, const char* name, double bytes, const fgeo& fg, chunk* f,
                              chunk* b, const fop* fops, const cx* mats, cx* partials,
                              uint64_t stride, GridUse& use) {
    if ((1ull << (fg.lc + fg.h)) != (uint64_t)TB)
      return fail("internal: a %llu-chunk fused tile on the %d-chunk LDS kernel",
                  (unsigned long long)(1ull << (fg.lc + fg.h)), TB);
    // 256 threads per tile (measured: 128 threads with twice the quartets per thread and
    // occupancy 2 was 2-4 % slower)
    constexpr int NT = 256;
    auto kern = k_fused<TWO, TB, HASRED, WF, NT>;
    QDC_TRY(fused_grid((const void*)kern, nullptr, NT, use.grid));
    fgeo g = fg;
    QDC_TRY(size_grid(ctx, g, use, false, "fused"));
    return ctx.launch_block(name, bytes, kern, use.grid, (uint32_t)NT, f, b, fops, mats, g, partials,
                            stride);
  }
  // a density-only pass (k_dens1): the tile of the one-state LDS kernel of its size
  const char* launch_dens1(Ctx& ctx, const char* name, double bytes, const fgeo& fg, chunk* f,
                           const fop* fops, cx* partials, uint64_t stride, GridUse& use) {
    if ((1ull << (fg.lc + fg.h)) == TILE_CHUNKS_2)
      return launch_dens1_tb<(int)TILE_CHUNKS_2>(ctx, name, bytes, fg, f, fops, partials, stride, use);
    return launch_dens1_tb<(int)TILE_CHUNKS_1>(ctx, name, bytes, fg, f, fops, partials, stride, use);
  }
  template <int TB>
  const char* launch_dens1_tb(Ctx& ctx, const char* name, double bytes, const fgeo& fg, chunk* f,
                              const fop* fops, cx* partials, uint64_t stride, GridUse& use) {
    if ((1ull << (fg.lc + fg.h)) != (uint64_t)TB)
      return fail("internal: a %llu-chunk density tile on the %d-chunk kernel",
                  (unsigned long long)(1ull << (fg.lc + fg.h)), TB);
    if (fg.nops == 0 || fg.nops > (uint32_t)DENS1_MAX || fg.ngrad != fg.nops)
      return fail("internal: a density pass of %u ops, %u reductions", fg.nops, fg.ngrad);
    constexpr int NT = 256;
    auto kern = k_dens1<TB, NT>;
    QDC_TRY(fused_grid((const void*)kern, nullptr, NT, use.grid));
    fgeo g = fg;
    QDC_TRY(size_grid(ctx, g, use, false, "density"));  // (ngrad = nops > 0: always a reduction)
    return ctx.launch_block(name, bytes, kern, use.grid, (uint32_t)NT, (const chunk*)f, fops, g,
                            partials, stride);
  }
  // register-resident pass (qdc_rq.hpp) on its kernel variant V (emit_rq_pass's choice,
  // qdc_variant.hpp), or on the pass's own specialized kernel where one is loaded: the same
  // block size, tile shares and arguments either way
  const char* launch_rq(Ctx& ctx, const char* name, double bytes, const fgeo& fg, bool two,
                        uint32_t tbits, const RqVariant* V, uint32_t l0, chunk* f, chunk* b,
                        const fop* fops, const cx* mats, cx* partials, uint64_t stride,
                        hipFunction_t spec, GridUse& use) {
    if (!V || V->two != two || V->tbits != tbits || (spec && !V->prefix))
      return fail("internal: a register-resident pass without its kernel variant");
    // a register-resident pass holds gate stages only (classify_pass), and only two-state
    // stages accumulate Gamma: a one-state pass never reduces.  Its dynamic tail (no granule
    // partials) and the one-state kernels (no reduction code) rest on that.
    if (!two && fg.ngrad > 0)
      return fail("internal: a one-state register-resident pass with %u reductions", fg.ngrad);
    // (a pass of more than RQ_GACC_SMALL Gamma stages: the instance with FMAX_GRAD_RQ accumulators)
    const rq_kernel_t kernel = V->kernel_for(fg.ngrad);
    QDC_TRY(fused_grid((const void*)kernel, spec && V->own_grid ? spec : nullptr, (int)V->threads,
                       use.grid));
    fgeo g = fg;
    QDC_TRY(size_grid(ctx, g, use, V->dyn, "fused"));
    if (spec)
      return ctx.launch_module(name, bytes, spec, use.grid, V->threads, f, b, fops, mats, g, l0,
                               partials, stride);
    return ctx.launch_block(name, bytes, kernel, use.grid, V->threads, f, b, fops, mats, g, l0,
                            partials, stride);
  }
  // One wave of resident blocks of a kernel (occupancy query, cached per kernel), or
  // QDC_FUSED_BLOCKS.  fn: a loaded specialized kernel asked for its own occupancy instead (it
  // may differ from the interpreted kernel's).
  const char* fused_grid(const void* kernel, hipFunction_t fn, int nt, uint32_t& grid) {
    if (k.fused_blocks) {
      grid = k.fused_blocks;
      return nullptr;
    }
    const void* key = fn ? (const void*)fn : kernel;
    for (auto& e : fused_resident_cache)
      if (e.first == key) {
        grid = e.second;
        return nullptr;
      }
    int per_cu = 0, dev = 0, cus = 0;
    if (fn)
      QDC_HIP(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, nt, 0));
    else
      QDC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, nt, 0));
    QDC_HIP(hipGetDevice(&dev));
    QDC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    grid = (uint32_t)std::max(1, std::min(per_cu * cus, (int)NBMAX));
    fused_resident_cache.push_back({key, grid});
    return nullptr;
  }
  // The tile shares of a fused launch over g.ntiles tiles, from `grid` resident blocks: static
  // shares + a dynamic tail where the kernel takes one (dyn) and Ctx::plan_dyn finds one, else a
  // power-of-two number of tiles per block on the fewest blocks that need.  Sets g's shares and
  // hands back the launch's grid and granule partials (GridUse).
  const char* size_grid(Ctx& ctx, fgeo& g, GridUse& use, bool dyn, const char* what) {
    uint32_t& grid = use.grid;
    if (!(dyn && grid >= 8 && g.ntiles >= 4ull * grid && ctx.plan_dyn(g, grid))) {
      uint64_t tpb = 1;
      while (tpb * grid < g.ntiles) tpb <<= 1;
      g.tpb = (uint32_t)tpb;
      grid = (uint32_t)((g.ntiles + tpb - 1) / tpb);
    }
    if (g.ngrad > 0 && grid > NBMAX) return fail("%s reduction grid %u exceeds %u", what, grid, NBMAX);
    use.ndyn = g.ndyn ? ctx.last_ndyn : 0u;
    return nullptr;
  }

  // Run one fused pass on every shard.  two: fwd and bwd (reverse sweep).  Reductions (Gamma
  // stages, densities) go to slots it.grad_slots of red_base (grads or dens of each shard).
  const char* run_fused(const Call& c, const Item& it, bool two) {
    fgeo fg{};
    fg.order = it.rq ? (uint32_t)k.rq_order : 0u;
    fg.gm = gm;
    fg.lc = it.lc;
    fg.h = it.h;
    for (uint32_t k = 0; k < FMAX_ROWS; ++k) fg.hb[k] = it.hb[k];
    fg.nops = it.nstage;
    fg.ngrad = it.has_red ? (uint32_t)it.grad_slots.size() : 0;
    fg.ntiles = nchunks_of(nl) >> (it.lc + it.h);

    // algorithmic bytes: each state read once, written once if the pass changes it
    const double S = state_bytes(nl);
    const double bytes = two ? (it.writes_f ? 4.0 : 3.0) * S : (it.writes_f ? 2.0 : 1.0) * S;
    const double flops = it.flops_per_amp * (double)((uint64_t)1 << nl);
    // one name per kernel variant (bytes per launch differ: 4S, 3S, 2S, S)
    const char* name = two ? (it.writes_f ? "fused_reverse" : "fused_inject")
                           : (it.writes_f ? "fused_apply" : "fused_density");
    for (auto& s : sh) {
      Ctx& ctx = s.c();
      QDC_TRY(ctx.use());
      const fop* fops = reinterpret_cast<const fop*>(s.d->prog_dev + it.fop_off);
      const cx* mats = reinterpret_cast<const cx*>(s.d->prog_dev + c.mats_off);
      chunk* f = reinterpret_cast<chunk*>(s.state);
      chunk* b = reinterpret_cast<chunk*>(s.bwd);
      cx* parts = nullptr;
      if (fg.ngrad > 0) {
        cx* base = c.backward ? s.grads : s.dens;
        QDC_TRY(ctx.begin_reduction(base, 0));
        if (ctx.pending_dst.size() + fg.ngrad > (size_t)FIN_MAX) QDC_TRY(ctx.flush());
        ctx.pending_base = base;
        ctx.pending_accumulate = 0;
        parts = ctx.slot_ptr();
      }
      const uint64_t stride = (uint64_t)NBMAX * RED;
      ctx.next_flops = flops;
      GridUse use;
      if (it.rq) {
        QDC_TRY(launch_rq(ctx, name, bytes, fg, two, it.tbits, it.var, it.l0, f, b, fops, mats, parts,
                          stride, spec_fn_on(it, ctx.device), use));
      } else if (two) {
        if (it.writes_f)
          QDC_TRY((launch_fused<true, true, true>(ctx, name, bytes, fg, f, b, fops, mats, parts, stride, use)));
        else
          QDC_TRY((launch_fused<true, false, false>(ctx, name, bytes, fg, f, b, fops, mats, parts, stride, use)));
      } else if (it.dens1) {
        QDC_TRY(launch_dens1(ctx, name, bytes, fg, f, fops, parts, stride, use));
      } else if (!it.has_red) {
        QDC_TRY((launch_fused<false, false, true>(ctx, name, bytes, fg, f, b, fops, mats, parts, stride, use)));
      } else if (it.writes_f) {
        QDC_TRY((launch_fused<false, true, true>(ctx, name, bytes, fg, f, b, fops, mats, parts, stride, use)));
      } else {
        QDC_TRY((launch_fused<false, true, false>(ctx, name, bytes, fg, f, b, fops, mats, parts, stride, use)));
      }
      if (fg.ngrad > 0)
        for (uint32_t slot : it.grad_slots) ctx.commit(slot, use.grid, use.ndyn);
    }
    return nullptr;
  }

  // one gate on one state: forward, or (uncompute) the reverse sweep before its first cotangent
  const char* apply_gate(Ctx& ctx, const Instr& in, const qdc_complex* g4, cx* s, uint32_t p2,
                         uint32_t p1, bool uncompute) {
    GateMats M;
    QDC_TRY(gate_mats(in.kind, g4, uncompute, M));
    if (M.diag)
      return apply_diag(ctx, s, GateMats::diagonal(M.a), p2, p1, nl,
                        uncompute ? "uncompute_q2_diag" : "apply_q2_diag");
    if (M.R == 2)
      return apply_dense<2>(ctx, s, GateMats::dense<2>(M.a), p2, p2, nl,
                            uncompute ? "uncompute_q1" : "apply_q1");
    return apply_dense<4>(ctx, s, GateMats::dense<4>(M.a), p2, p1, nl,
                          uncompute ? "uncompute_q2" : "apply_q2");
  }

  // The trace entries of this call's fused stages (gate_stage, physical positions) mapped to
  // logical qubits by replaying the call's layout changes (step_layout) from `layout` (the
  // call's start), with the single-gate items' matrices (as apply_gate / reverse_dense apply
  // them) inserted in item order.  Dry runs only.
  const char* trace_logical(const Call& c) {
    std::vector<TraceOp> fused(trace.begin() + (std::ptrdiff_t)c.trace_start, trace.end());
    trace.resize(c.trace_start);
    QubitMap m = layout;
    size_t t = 0;
    for (size_t ii = 0; ii < c.items.size(); ++ii) {
      const Item& it = c.items[ii];
      for (; t < fused.size() && fused[t].item == ii; ++t) {
        TraceOp s = fused[t];
        s.q2 = m.logi[s.q2];
        s.q1 = m.logi[s.q1];
        trace.push_back(s);
      }
      if (it.type == ITEM_OP) {
        const qdc_plan_op& op = c.plan[it.ops[0]];
        const Instr& in = ins[op.instr];
        if (is_const(in.kind) || is_var(in.kind)) {
          TraceOp s{c.backward ? 1u : 0u, (uint32_t)ii, m.logi[op.pos2], m.logi[op.pos1], 4u,
                    is_diag(in.kind) ? 1u : 0u, 0u, 1u, {}};
          GateMats M;
          QDC_TRY(gate_mats(in.kind, c.gate(in, op.instr), c.backward, M));
          s.R = (uint32_t)M.R;
          if (M.R == 2) s.q1 = s.q2;
          for (int i = 0; i < M.count(); ++i)  // (a diagonal expanded)
            s.m[M.diag ? i * 5 : i] = qdc_complex{(qdc_real)M.a[i].x, (qdc_real)M.a[i].y};
          trace.push_back(s);
        }
      }
      step_layout(m, it, c.plan);
    }
    return nullptr;
  }

  const char* dyn_reset_all() {
    for (auto& d : devs) {
      QDC_TRY(d->ctx.use());
      QDC_TRY(d->ctx.dyn_reset());
    }
    return nullptr;
  }

  // --- the sweep: one loop over a call's items, forward or reverse ------------------------------
  // One plan op outside the fused passes, on every shard.  A gate: applied (forward), only
  // uncomputed on fwd (reverse sweep before its first cotangent), or reversed on the state pair
  // with its gradient.  A density: measured (forward), or its cotangent injected (backward).
  const char* run_single(Call& c, const qdc_plan_op& op) {
    const Instr& in = ins[op.instr];
    const bool gate = is_const(in.kind) || is_var(in.kind), var = is_var(in.kind);
    const bool q1 = is_q1_density(in.kind);
    const qdc_complex* g4 = gate ? c.gate(in, op.instr) : c.backward ? c.dg->at(c.gidx[op.instr]) : nullptr;
    for (auto& s : sh) {
      Ctx& ctx = s.c();
      QDC_TRY(ctx.use());
      if (gate && !c.have_bwd)
        QDC_TRY(apply_gate(ctx, in, g4, s.state, op.pos2, op.pos1, c.backward));
      else if (gate)
        QDC_TRY(reverse_gate(ctx, in, g4, s.state, s.bwd, op.pos2, op.pos1, var ? s.grads : nullptr,
                             c.var_idx[op.instr]));
      else if (!c.backward && q1)
        QDC_TRY(density<2>(ctx, s.state, op.pos2, op.pos2, nl, s.dens, c.out_idx[op.instr], 0));
      else if (!c.backward)
        QDC_TRY(density<4>(ctx, s.state, op.pos2, op.pos1, nl, s.dens, c.out_idx[op.instr], 0));
      else if (q1)
        QDC_TRY(inject<2>(ctx, s.state, s.bwd, transpose<2>(to_mat<2>(g4)), op.pos2, op.pos2, nl,
                          !c.have_bwd));
      else
        QDC_TRY(inject<4>(ctx, s.state, s.bwd, transpose<4>(to_mat<4>(g4)), op.pos2, op.pos1, nl,
                          !c.have_bwd));
    }
    if (!gate && c.backward) c.have_bwd = true;
    return nullptr;
  }
  // a run of diagonal cotangent injections: one elementwise pass (no pass program)
  const char* run_diag_inject(Call& c, const Item& item) {
    diag_tab T;
    const uint32_t ng = diag_table(c, item, T);
    for (auto& s : sh) {
      QDC_TRY(s.c().use());
      QDC_TRY(qdc::diag_inject(s.c(), s.state, s.bwd, T, ng, nl, gm, c.have_bwd));
    }
    c.have_bwd = true;
    return nullptr;
  }
  const char* run_item(Call& c, const Item& item) {
    switch (item.type) {
      case ITEM_DIAG_INJECT:
        return run_diag_inject(c, item);
      case ITEM_FUSED: {
        const bool two = c.two_state(item);
        if (two && !c.have_bwd) {  // the first injection is fused: it adds into a zero bwd
          for (auto& s : sh) {
            QDC_TRY(s.c().use());
            QDC_TRY(zero_bwd(s));
          }
          c.have_bwd = true;
        }
        return run_fused(c, item, two);
      }
      case ITEM_REMAP:
        return remap(c.plan[item.ops[0]], item.inv, c.have_bwd);
      default:
        return run_single(c, c.plan[item.ops[0]]);
    }
  }
  // The call's items from `from` on: each run (a dry run launches nothing), then the layout it
  // leaves
  const char* run_items(Call& c, size_t from = 0) {
    for (size_t ii = from; ii < c.items.size(); ++ii) {
      if (!dry) QDC_TRY(run_item(c, c.items[ii]));
      step_layout(layout, c.items[ii], c.plan);
    }
    return nullptr;
  }
  // the program built and (a dry, traced run) the call's trace entries made logical
  const char* build_and_trace(Call& c, const char* what) {
    QDC_TRY(build_program(c));
    c.ht[3] = hclock::now();
    if (k.rq_stats) fprintf(stderr, "%s plan+build %.3f ms\n", what, ms_between(c.ht[2], c.ht[3]));
    return dry && tracing ? trace_logical(c) : nullptr;
  }

  // --- forward (Circuit::run / Circuit::forward) --------------------------------------------
  const char* execute(int mode, const Flat& cg, const Flat& vg, qdc_complex* out) {
    Call c(*this, mode, false, mode == QDC_MODE_FORWARD, &cg, &vg);
    QDC_TRY(validate_forward(cg, vg, c.gidx));
    std::vector<int> widths;
    outputs(mode, c.out_idx, widths);
    const size_t nout = widths.size();
    if (!dry) {
      QDC_TRY(dyn_reset_all());
      QDC_TRY(ensure_out(true, std::max<size_t>(nout, 1) * RED));
    }
    // every pass starts from `initial`, which is always in the identity layout
    layout.identity(n, g);
    for (auto& s : sh) {
      QDC_TRY(s.c().use());
      QDC_TRY(copy_initial(s));
    }
    mark_inexact(cg, vg, c.gidx);
    c.ht[1] = hclock::now();
    c.plan = plan(mode);
    schedule(c);
    c.ht[2] = hclock::now();
    // a mirrored forward records what its backward will undo (forward mode only)
    mrec.valid = false;
    c.record = mirror_on() && mode == QDC_MODE_FORWARD;
    c.stage_mats.resize(c.record ? c.items.size() : 0);
    QDC_TRY(build_and_trace(c, "forward"));
    if (c.record) mrec.capture(cg, vg, c.plan, c.items, std::move(c.stage_mats), inexact);
    QDC_TRY(run_items(c));
    if (!dry) {
      c.ht[4] = hclock::now();
      QDC_TRY(flush_all());
    }
    if (c.record) {  // (valid once every pass ran; the backward starts from this layout)
      mrec.end_phys = layout.phys;
      mrec.valid = true;
    }
    if (dry) return nullptr;
    std::vector<cx*> bufs;
    for (auto& s : sh) bufs.push_back(s.dens);
    QDC_TRY(ex.allreduce(sh, bufs, nout * RED));
    QDC_TRY(collect(sh[0].dens, widths, out));
    c.ht[5] = hclock::now();
    host_record(0, c.ht);
    return nullptr;
  }

  // D2H of `total` (>= widths.size()) result slots into host_out; the first widths.size()
  // are unpacked into `out`.
  const char* collect(const cx* dev, const std::vector<int>& widths, qdc_complex* out,
                      size_t total = 0) {
    const size_t count = widths.size();
    total = std::max(total, count);
    if (total == 0) return sync_all();
    QDC_TRY(ensure_host(total * RED));
    Ctx& c0 = sh[0].c();
    QDC_TRY(c0.use());
    QDC_HIP(hipMemcpyAsync(host_out, dev, sizeof(cx) * total * RED, hipMemcpyDeviceToHost,
                           c0.stream));
    QDC_TRY(sync_all());
    size_t w = 0;
    for (size_t j = 0; j < count; ++j) {
      for (int k = 0; k < widths[j]; ++k) {
        out[w + k].re = host_out[j * RED + k].x;
        out[w + k].im = host_out[j * RED + k].y;
      }
      w += widths[j];
    }
    return nullptr;
  }

  // --- diagonal cotangent injections ----------------------------------------------------------
  // the injection's diagonal (G^T on its qubits has the diagonal of G), or false
  bool diag_cotangent(const Call& c, const qdc_plan_op& op) const {
    if (op.type != QDC_PLAN_OP || !is_diff_density(ins[op.instr].kind)) return false;
    const int R = is_q1_density(ins[op.instr].kind) ? 2 : 4;
    if (op.pos2 >= (uint32_t)(4 * DI_GROUPS) || op.pos1 >= (uint32_t)(4 * DI_GROUPS)) return false;
    if (R == 4 && op.pos2 / 4 != op.pos1 / 4) return false;  // both bits in one table group
    const qdc_complex* g = c.dg->at(c.gidx[op.instr]);
    for (int p = 0; p < R; ++p)
      for (int q = 0; q < R; ++q)
        if (p != q && (g[p * R + q].re != 0 || g[p * R + q].im != 0)) return false;
    return true;
  }
  // Consecutive items that are injections only, all with diagonal cotangents, become one
  // ITEM_DIAG_INJECT (their plan ops in order).  Injections only add to bwd from the (unchanged) fwd, so a
  // run of them commutes and sums.
  void merge_diag_injections(Call& c) const {
    auto eligible = [&](const Item& it) {
      if (it.type != ITEM_OP && it.type != ITEM_FUSED) return false;
      for (uint32_t k : it.ops)
        if (!diag_cotangent(c, c.plan[k])) return false;
      return !it.ops.empty();
    };
    std::vector<Item> out;
    for (Item& it : c.items) {
      if (eligible(it)) {
        if (!out.empty() && out.back().type == ITEM_DIAG_INJECT) {
          out.back().ops.insert(out.back().ops.end(), it.ops.begin(), it.ops.end());
          continue;
        }
        Item m;
        m.type = ITEM_DIAG_INJECT;
        m.ops = it.ops;
        out.push_back(std::move(m));
        continue;
      }
      out.push_back(std::move(it));
    }
    c.items = std::move(out);
  }
  // D(i) tables of an ITEM_DIAG_INJECT: T[g * 16 + e] = sum of the diagonal entries that the densities
  // on bits 4g..4g+3 select for the pattern e of those bits (summed in double); returns the
  // number of groups in use
  uint32_t diag_table(const Call& c, const Item& item, diag_tab& T) const {
    cd acc[DI_GROUPS * 16] = {};
    uint32_t ng = 1;
    for (uint32_t k : item.ops) {
      const qdc_plan_op& op = c.plan[k];
      const bool q1 = is_q1_density(ins[op.instr].kind);
      const int R = q1 ? 2 : 4;
      const qdc_complex* gd = c.dg->at(c.gidx[op.instr]);
      const uint32_t grp = op.pos2 / 4;
      ng = std::max(ng, grp + 1);
      for (uint32_t e = 0; e < 16; ++e) {
        const uint32_t b2 = (e >> (op.pos2 % 4)) & 1u, b1 = (e >> (op.pos1 % 4)) & 1u;
        const int r = q1 ? (int)b2 : (int)(2 * b2 + b1);
        acc[grp * 16 + e] += cd(gd[r * R + r].re, gd[r * R + r].im);
      }
    }
    for (int i = 0; i < DI_GROUPS * 16; ++i) T.t[i] = cx{(real)acc[i].real(), (real)acc[i].imag()};
    return ng;
  }

  // --- backward (Circuit::backward, circuit.rs:266-429) --------------------------------------
  // apply_gate's counterpart on the state pair: uncompute f, pull b back and, for a variable
  // gate, reduce its gradient into row dst of gbase
  const char* reverse_gate(Ctx& ctx, const Instr& in, const qdc_complex* g4, cx* f, cx* b,
                           uint32_t p2, uint32_t p1, cx* gbase, uint32_t dst) {
    GateMats M;
    QDC_TRY(gate_mats(in.kind, g4, true, M));
    if (M.diag) return reverse_diag(ctx, f, b, GateMats::diagonal(M.b), p2, p1, nl, gbase, dst);
    if (M.R == 2)
      return reverse_dense<2>(ctx, f, b, GateMats::dense<2>(M.a), GateMats::dense<2>(M.b), p2, p2,
                              nl, gbase, dst);
    return reverse_dense<4>(ctx, f, b, GateMats::dense<4>(M.a), GateMats::dense<4>(M.b), p2, p1, nl,
                            gbase, dst);
  }
  // The backward's schedule: the forward's passes in reverse (mirror_schedule) when this backward
  // follows that forward with the same gates, else its own plan, fused as usual
  const char* schedule_backward(Call& c) {
    bool mirrored = false;
    if (mirror_on() && mrec.valid && mrec.inexact == inexact && mrec.end_phys == layout.phys)
      mirrored = mrec.same_gates(*c.cg, *c.vg) && mirror_schedule(c);
    mrec.valid = false;  // (this backward changes the layout and the state)
    if (mirrored) return nullptr;
    c.plan = plan(QDC_PLAN_BACKWARD);
    c.first_inject = first_injection(c.plan);
    // QDC_MIRROR=2 (tests): a backward that cannot mirror its forward is an error
    if (mirror_on() && k.mirror == 2)
      return fail("mirror: the backward does not follow a forward call with the same gates");
    schedule(c);
    return nullptr;
  }
  const char* backward(const Flat& dg, const Flat& cg, const Flat& vg, qdc_complex* out) {
    Call c(*this, QDC_PLAN_BACKWARD, true, false, &cg, &vg, &dg);
    QDC_TRY(validate_backward(dg, cg, vg, c.gidx));
    if (!dry) QDC_TRY(dyn_reset_all());
    c.var_idx.assign(ins.size(), 0);
    for (size_t k = 0; k < ins.size(); ++k)
      if (is_var(ins[k].kind)) c.var_idx[k] = c.nvar++;
    const size_t nvar = c.nvar;
    for (auto& s : sh) {
      if (!s.bwd) {
        QDC_TRY(s.c().use());
        QDC_HIP(hipMalloc(&s.bwd, ((size_t)1 << nl) * sizeof(cx)));
        s.owned.push_back(s.bwd);
      }
      s.bwd_live = true;
    }
    // slots [0, nvar): per-gate gradients; [nvar, nvar + stages): fused stages' Gamma
    const size_t nslots = std::max<size_t>(2 * nvar, 1);
    if (!dry) QDC_TRY(ensure_out(false, nslots * RED));
    // variable gates met before the first cotangent keep zero gradients (circuit.rs:327-331)
    for (auto& s : sh) {
      QDC_TRY(s.c().use());
      QDC_HIP(hipMemsetAsync(s.grads, 0, sizeof(cx) * nslots * RED, s.c().stream));
    }
    mark_inexact(cg, vg, c.gidx);
    c.ht[1] = hclock::now();
    QDC_TRY(schedule_backward(c));
    if (k.diag_inject) merge_diag_injections(c);
    c.ht[2] = hclock::now();
    // the backward's leading diagonal-injection passes need no program: they are launched
    // before it is built, so the device runs them during the host's build (round 6;
    // QDC_EARLY_INJECT=0: after)
    size_t lead = 0;
    if (!dry && k.early_inject)
      for (; lead < c.items.size() && c.items[lead].type == ITEM_DIAG_INJECT; ++lead)
        QDC_TRY(run_diag_inject(c, c.items[lead]));
    QDC_TRY(build_and_trace(c, "backward"));
    QDC_TRY(run_items(c, lead));
    if (dry) return nullptr;
    c.ht[4] = hclock::now();
    QDC_TRY(flush_all());
    const size_t used = nvar + c.stage_post.size();
    std::vector<cx*> bufs;
    for (auto& s : sh) bufs.push_back(s.grads);
    QDC_TRY(ex.allreduce(sh, bufs, used * RED));
    std::vector<int> widths;
    for (auto& in : ins)
      if (is_var(in.kind)) widths.push_back(gate_len(in.kind));
    QDC_TRY(collect(sh[0].grads, widths, out, used));
    // gradients of fused stages: G = ptrace(L Gamma Rt) per gate (qdc_stage.hpp)
    if (!c.stage_post.empty()) {
      std::vector<size_t> off(widths.size() + 1, 0);
      for (size_t j = 0; j < widths.size(); ++j) off[j + 1] = off[j] + widths[j];
      stage_gradients(c.stage_post, host_out, (size_t)RED, off, widths, out);
    }
    c.ht[5] = hclock::now();
    host_record(1, c.ht);
    return nullptr;
  }
};

}  // namespace qdc

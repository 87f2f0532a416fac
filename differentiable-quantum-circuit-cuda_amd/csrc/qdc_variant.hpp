// qdc_variant.hpp — the register-resident kernel variants the runtime can launch (qdc_rq.hpp:
// k_rq, k_rw), one row each, and the one function that picks a pass's row from the knobs.
//
// A row says everything the host needs to know about a variant: the tile it runs, its block
// size and register slots, whether its launch may take a dynamic tail (Ctx::plan_dyn), the
// generic kernel, and — where the variant has one — the specialized pass that replaces the
// generic kernel (qdc_spec.hpp, qdc_jit.hpp spec_kind).  Circuit::emit_rq_pass selects a row
// per pass (rq_select) and plans and generates from it, Circuit::launch_rq launches from it,
// and the host-only hooks (qdc_rq_variant, qdc_spec_selftest) read the same rows: a kernel is
// never launched with the block size, slots or grid of another.
#pragma once

#include "qdc_rq.hpp"

namespace qdc {

// every k_rq / k_rw instantiation (and every specialized pass kernel) has this signature
using rq_kernel_t = void (*)(chunk*, chunk*, const fop*, const cx*, fgeo, uint32_t, cx*, uint64_t);

struct RqVariant {
  const char* label;   // the generic kernel as written in source
  rq_kernel_t kernel;  // ... and as launched
  bool two;            // two-state (reverse sweep) or one-state
  uint32_t tbits;      // amplitude bits of the tile
  uint32_t threads;    // block size (k_rw: 64 W, k_rq: NT)
  uint32_t ns;         // register slots the pass is planned for
  bool dyn;            // the launch may use static shares + a dynamic tail (Ctx::plan_dyn)
  // the specialized pass (prefix == nullptr: none): kernel name prefix, the generic kernel's
  // body with the program and its amdgpu_waves_per_eu; the same for programs that relayout
  // through half the buffer (pass_half == nullptr: no such form)
  const char* prefix;
  const char* pass;
  const char* waves;
  const char* pass_half;
  const char* waves_half;
  // a specialized launch sizes its grid from the specialized kernel's own occupancy (else from
  // the generic kernel's).  Kept exactly as measured; DESIGN.md lists unifying it as follow-up
  bool own_grid;
  // two-state rows: the generic kernel with FMAX_GRAD_RQ Gamma accumulators, which runs the
  // passes of more than RQ_GACC_SMALL Gamma stages (`kernel` holds RQ_GACC_SMALL: the LDS
  // footprint of a pass that needs no more does not grow with the storage bound); nullptr: a
  // one-state row
  rq_kernel_t kernel_wide = nullptr;
  // the generic kernel of a pass with `gamma` Gamma stages
  rq_kernel_t kernel_for(uint32_t gamma) const {
    return gamma > (uint32_t)RQ_GACC_SMALL && kernel_wide ? kernel_wide : kernel;
  }
};

#define QDC_RQ_KERNEL(...) #__VA_ARGS__, __VA_ARGS__
#define QDC_RQ_NO_SPEC nullptr, nullptr, nullptr, nullptr, nullptr, false
#ifndef QDC_F64
// f32: 16 amplitudes per lane and state and register group
enum RqVariantId {
  RV_TWO_S5, RV_TWO, RV_TWO_AGPR, RV_TWO_RQ,
  RV_ONE_S5, RV_ONE_S5_PF, RV_ONE, RV_ONE_RQ_PF, RV_ONE_RQ,
  RV_ONE12_RW, RV_ONE12_RQ_PF, RV_ONE12_RQ,
  RV_COUNT
};
inline const RqVariant* rq_variants() {
  static const RqVariant V[RV_COUNT] = {
      {QDC_RQ_KERNEL(k_rw<true, 2, false, 1, true>), true, 11, 64, 5, true, "qdc_spec_",
       "qdc::rw_pass<true, 2, false, 1, true, Prog>", "QDC_RW_WAVES, QDC_RW_WAVES",
       "qdc::rw_pass<true, 2, false, 1, true, Prog, true>", "QDC_RW_WAVES, QDC_RW_WAVES", true,
       k_rw<true, 2, false, 1, true, FMAX_GRAD_RQ>},
      {QDC_RQ_KERNEL(k_rw<true, 2, false, 1>), true, 11, 64, 4, true, QDC_RQ_NO_SPEC,
       k_rw<true, 2, false, 1, false, FMAX_GRAD_RQ>},
      // the next tile prefetched into AGPRs, one wave per SIMD
      {QDC_RQ_KERNEL(k_rw<true, 2, true, 1>), true, 11, 64, 4, false, QDC_RQ_NO_SPEC,
       k_rw<true, 2, true, 1, false, FMAX_GRAD_RQ>},
      {QDC_RQ_KERNEL(k_rq<true, 128, false>), true, 11, 128, 4, false, QDC_RQ_NO_SPEC,
       k_rq<true, 128, false, FMAX_GRAD_RQ>},
      // one wave per 2^11 tile (QDC_TILE1_CHUNKS=1024, or a mirrored forward).  The half-buffer
      // form needs 8 KiB of LDS per wave and is compiled for QDC_RW_WAVES_HALF_ONE [5] waves per
      // SIMD (~96 VGPRs, a few spilled; 4 waves at 106 VGPRs measured 0.7-1.0 % slower per step)
      {QDC_RQ_KERNEL(k_rw<false, 2, false, 1, true>), false, 11, 64, 5, true, "qdc_specf_",
       "qdc::rw_pass<false, 2, false, 1, true, Prog>", "QDC_RW_WAVES_ONE, QDC_RW_WAVES_ONE",
       "qdc::rw_pass<false, 2, false, 1, true, Prog, true>",
       "QDC_RW_WAVES_HALF_ONE, QDC_RW_WAVES_HALF_ONE", true},
      // ... the next tile prefetched into pinned VGPRs
      {QDC_RQ_KERNEL(k_rw<false, 2, true, 1, true>), false, 11, 64, 5, true, "qdc_specf_",
       "qdc::rw_pass<false, 2, true, 1, true, Prog>", "QDC_RW_WAVES, QDC_RW_WAVES", nullptr, nullptr,
       false},
      {QDC_RQ_KERNEL(k_rw<false, 2, false, 1>), false, 11, 64, 4, true, QDC_RQ_NO_SPEC},
      {QDC_RQ_KERNEL(k_rq<false, 128, true>), false, 11, 128, 4, true, QDC_RQ_NO_SPEC},
      {QDC_RQ_KERNEL(k_rq<false, 128, false>), false, 11, 128, 4, false, QDC_RQ_NO_SPEC},
      // 2^12 tiles: two waves, or four (prefetching: the forward's default)
      {QDC_RQ_KERNEL(k_rw<false, 2, false, 2>), false, 12, 128, 4, false, QDC_RQ_NO_SPEC},
      {QDC_RQ_KERNEL(k_rq<false, 256, true>), false, 12, 256, 4, true, "qdc_specf_",
       "qdc::rq_pass<false, 256, true, Prog>", "QDC_RQ_PF_WAVES", nullptr, nullptr, false},
      {QDC_RQ_KERNEL(k_rq<false, 256, false>), false, 12, 256, 4, false, QDC_RQ_NO_SPEC},
  };
  return V;
}
#else
// f64: 16 amplitudes (4 VGPRs each) per lane and state; two-state 2^10-amplitude tiles on one
// wave, one-state 2^10 (a reverse sweep's passes before the first injection) or 2^11 on two
enum RqVariantId { RV_TWO, RV_ONE, RV_ONE11, RV_COUNT };
inline const RqVariant* rq_variants() {
  static const RqVariant V[RV_COUNT] = {
      {QDC_RQ_KERNEL(k_rw<true, 1, false, 1>), true, 10, 64, 4, true, "qdc_spec_d_",
       "qdc::rw_pass<true, 1, false, 1, false, Prog>", "QDC_RW_WAVES, QDC_RW_WAVES", nullptr, nullptr,
       false, k_rw<true, 1, false, 1, false, FMAX_GRAD_RQ>},
      {QDC_RQ_KERNEL(k_rw<false, 1, false, 1>), false, 10, 64, 4, true, "qdc_specf_d_",
       "qdc::rw_pass<false, 1, false, 1, false, Prog>", "QDC_RW_WAVES_ONE, QDC_RW_WAVES_ONE", nullptr,
       nullptr, false},
      {QDC_RQ_KERNEL(k_rw<false, 1, false, 2>), false, 11, 128, 4, false, "qdc_specf_d_",
       "qdc::rw_pass<false, 1, false, 2, false, Prog>", "QDC_RW_WAVES_ONE, QDC_RW_WAVES_ONE", nullptr,
       nullptr, false},
  };
  return V;
}
#endif
#undef QDC_RQ_KERNEL
#undef QDC_RQ_NO_SPEC

// The knobs that choose among the rows (Circuit::read_knobs)
struct RqKnobs {
  // QDC_RW: bit 0 two-state passes on k_rw (one wave per tile), bit 1 one-state passes on k_rw,
  // bit 2 two-state passes prefetch the next tile into AGPRs, bit 3 one-state one-wave
  // five-slot passes prefetch the next tile (with QDC_RQ_PF)
  int rq_wave = 1;
  int rq_prefetch = 1;  // one-state passes prefetch the next tile (QDC_RQ_PF)
  int rq_slots5 = 1;    // f32 one-wave passes plan five register slots (QDC_RQ_SLOTS5)
};

// The variant that runs a two- or one-state pass on tiles of 2^tbits amplitudes; `mirror`: the
// circuit's forwards are mirrored (their one-state passes run on the two-state tile, one wave
// each).  nullptr: no register-resident kernel runs such a tile.
inline const RqVariant* rq_select(bool two, uint32_t tbits, const RqKnobs& k, bool mirror) {
  const RqVariant* V = rq_variants();
#ifndef QDC_F64
  const bool w0 = k.rq_wave & 1, w1 = k.rq_wave & 2, w2 = k.rq_wave & 4, w3 = k.rq_wave & 8;
  const bool pf = k.rq_prefetch != 0, s5 = k.rq_slots5 != 0;
  if (two && tbits == 11) return &V[!w0 ? RV_TWO_RQ : w2 ? RV_TWO_AGPR : s5 ? RV_TWO_S5 : RV_TWO];
  if (!two && tbits == 11) {
    if (w1 || mirror) return &V[!s5 ? RV_ONE : (w3 && pf) ? RV_ONE_S5_PF : RV_ONE_S5];
    return &V[pf ? RV_ONE_RQ_PF : RV_ONE_RQ];
  }
  if (!two && tbits == 12) return &V[w1 ? RV_ONE12_RW : pf ? RV_ONE12_RQ_PF : RV_ONE12_RQ];
#else
  (void)k;
  (void)mirror;
  if (two && tbits == 10) return &V[RV_TWO];
  if (!two && tbits == 10) return &V[RV_ONE];
  if (!two && tbits == 11) return &V[RV_ONE11];
#endif
  return nullptr;
}

// A variant's five-slot passes (2^11 tiles) are planned to keep a slot in place across every
// relayout where they can, for the half-buffer specialized form (rq_plan keep; spec_half:
// QDC_SPEC_HALF)
inline bool rq_keep(const RqVariant& V, bool spec_half) { return spec_half && V.ns == 5; }

// The slot case a stage of this kind runs with, from the plan's case cs = 8 S1 + S2: two-qubit
// and diagonal stages run with the lower slot first (half the kernels' cases).  swapped: the
// slots were exchanged, so the caller exchanges the matrices' index bits to match.
inline uint32_t rq_slot_case(uint32_t kind, uint32_t cs, bool& swapped) {
  const uint32_t kd = kind & 7u;
  swapped = (kd == FK_Q2 || kd == FK_DIAG) && (cs >> 3) > (cs & 7u);
  return swapped ? (cs & 7u) * 8u + (cs >> 3) : cs;
}

}  // namespace qdc

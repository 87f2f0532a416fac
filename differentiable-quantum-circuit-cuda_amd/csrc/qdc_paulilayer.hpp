// qdc_paulilayer.hpp — diagonal Pauli layers (include/qdc/pauli.h: qdc_pauli_layer,
// qdc_pauli_layer_reverse): K rotations about Z-only strings P_k = Z^{z_k} in one pass,
//     U = exp(-i/2 sum_k theta_k P_k),   (U psi)[i] = e^{-i phi(i)} psi[i],
//     phi(i) = 1/2 sum_k theta_k s_k(i),  s_k(i) = (-1)^popcount(i & z_k).
// Reverse step: fwd <- e^{+i phi} fwd, bwd <- e^{-i phi} bwd (U^T = U), and
//     dL/dtheta_k = 1/2 Im sum_i s_k(i) bwd[i] fwd[i]
// (qdc_pauli_rot_reverse's convention at nY = 0); bwd[i] fwd[i] does not change under the layer,
// so a layer split over launches is exact.
//
// The skeleton is k_prot_self's: 16-byte chunks, blocks of 256 striding over spans of
// 256 * PAULI_FU chunks, every load of a span issued before its first store, a guarded path for a
// state below one span.  A span is 2^L amplitudes (L = PAULI_W: 11 in f32, 10 in f64), so an index
// splits as i = (i_hi, i_lo) with i_hi the span's number, and i_lo = (u, t, v): u the chunk of the
// thread inside the span (PAULI_FU values), t the thread (8 bits), v the amplitude of the chunk.
// (u, v) is the thread's register SLOT, PL_NS = PAULI_FU * VEC of them.
//
// Phase, in fixed point.  The host turns theta_k into t_k = round(theta_k / 4 pi 2^B) mod 2^B
// (long double; B = 32 in f32, 64 in f64): phi / 2 pi in units of 2^-B turns.  The kernel adds and
// subtracts these as unsigned integers: wrap-around is the range reduction, the sum is exact and
// its order changes no bit.  Terms are grouped by low mask m = z mod 2^L:
//     T_m(span)  = sum_{k in m} (-1)^popcount(i_hi & z_hi,k) t_k      span-uniform: scalar code
//     phi(i_lo)  = sum_m s_m(i_lo) T_m,   s_m(i_lo) = s_m(t) s_m(slot)
// The groups are ordered by their slot pattern p (the bits of m that select among the slots), so
//     F_p = sum_{m with pattern p} s_m(t) T_m                         one signed add per GROUP and
//     phi(slot) = sum_p (-1)^popcount(slot & p) F_p                   thread; then a butterfly over
// the PL_NS patterns.  Per amplitude that is 1 / PL_NS signed adds per distinct low mask plus
// log2(PL_NS) adds; a term that lies wholly in the high bits costs nothing per amplitude.  The
// signed sum becomes x = phi / pi in [-1, 1) and sincospi(x) gives the factor (an accurate sincos:
// the argument needs no further reduction).
//
// Gradients (GRAD), grouped like the phase.  q(slot) = Im(bwd fwd); the same butterfly gives
//     W_p = sum_slot (-1)^popcount(slot & p) q(slot)                  once per span and thread,
//     w_m = s_m(t) W_p(m)                                             once per group,
//     A_k += s_k(i_hi) w_m(k)                                         one signed add per term,
// in the uniform walk of the table the phase takes (pattern, group, term).  The per-thread
// accumulators A_k are indexed by that walk, so they live in LDS (column t of [PL_GCAP][256],
// each thread its own words: no synchronisation, no atomics) and not in registers.  They are
// reduced once per block (block_reduce_store, two real gradients per complex value: 2 RED = 32
// terms per reducing launch), then reduce_into / k_finalize: every order fixed.  Streaming launches carry up to PL_CAP = 128 terms in the kernel
// arguments; larger layers split in term order, each launch handling its own terms completely.
#pragma once

#include <algorithm>
#include <utility>
#include <vector>

#include "qdc_paulirot.hpp"

namespace qdc {

#ifdef QDC_F64
using pfix = uint64_t;
#else
using pfix = uint32_t;
#endif
constexpr uint32_t PL_L = PAULI_W;            // log2(amplitudes of a span)
constexpr int PL_NS = PAULI_FU * VEC;         // register slots of a thread and span
constexpr uint32_t PL_CAP = 128;              // terms of a streaming launch
constexpr uint32_t PL_GCAP = 2u * RED;        // terms of a reducing launch
static_assert((1u << PL_L) == 256u * PAULI_FU * VEC, "a span is 2^L amplitudes");
static_assert((PAULI_FU & (PAULI_FU - 1)) == 0, "the slots are index bits");

struct ltab {
  uint32_t nt;             // terms
  uint16_t pg[PL_NS + 1];  // groups [pg[p], pg[p + 1]) have slot pattern p
  uint32_t gi[PL_CAP];     // group: end of its terms | thread mask << 16
  uint32_t zhi[PL_CAP];    // term: z >> L
  pfix t[PL_CAP];          // term: the angle in 2^-B turns of phi (negated: the reverse)
};
static_assert(sizeof(ltab) <= 3584, "the table travels in the kernel arguments (4 KiB)");

// the slot pattern and the thread mask of a low mask m < 2^L.  lv = log2 of the index values a
// chunk holds: LV for amplitudes, 0 where a chunk is one pair (qdc_paulixlayer.hpp, f32 at x = 1);
// L = 10 + lv and a thread has PAULI_FU << lv slots.
constexpr uint32_t pl_pattern(uint32_t m, uint32_t lv = LV) {
  return (m & ((1u << lv) - 1u)) | (((m >> (8 + lv)) & (uint32_t)(PAULI_FU - 1)) << lv);
}
constexpr uint32_t pl_tmask(uint32_t m, uint32_t lv = LV) { return (m >> lv) & 0xffu; }
constexpr uint32_t pl_span_bits(uint32_t lv = LV) { return PL_L - (uint32_t)LV + lv; }

// ph[slot] = phi(i_hi, slot, t) in 2^-B turns.  Everything but the thread's sign is uniform.
template <int NS>
__device__ __forceinline__ void pl_phases(const ltab& T, uint32_t ihi, uint32_t t,
                                          pfix (&ph)[NS]) {
  static_assert(NS <= PL_NS && (NS & (NS - 1)) == 0, "the slots of a table");
  uint32_t g = 0, k = 0;
#pragma unroll
  for (int p = 0; p < NS; ++p) {
    pfix F = 0;
    const uint32_t ge = T.pg[p + 1];
    for (; g < ge; ++g) {
      const uint32_t gi = T.gi[g], ke = gi & 0xffffu, tm = gi >> 16;
      pfix Tm = 0;
      for (; k < ke; ++k) {
        const pfix tk = T.t[k];
        Tm += (__popc(ihi & T.zhi[k]) & 1) ? (pfix)0 - tk : tk;
      }
      F += (__popc(t & tm) & 1) ? (pfix)0 - Tm : Tm;
    }
    ph[p] = F;
  }
  // ph[s] <- sum_p (-1)^popcount(s & p) ph[p]
#pragma unroll
  for (int bit = 1; bit < NS; bit <<= 1)
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (!(s & bit)) {
        const pfix a = ph[s], b = ph[s | bit];
        ph[s] = a + b;
        ph[s | bit] = a - b;
      }
}

// (cos phi, sin phi) of a phase in 2^-B turns: the signed value is phi / pi in [-1, 1)
__device__ __forceinline__ cx pl_cis(pfix ph) {
  cx r;
#ifdef QDC_F64
  sincospi((double)(int64_t)ph * 0x1p-63, &r.y, &r.x);
#else
  sincospif((float)(int32_t)ph * 0x1p-31f, &r.y, &r.x);
#endif
  return r;
}

// A[k] += the span's share of sum_i s_k(i) q(i), k < T.nt <= PL_GCAP; A = the thread's column of
// the block's accumulators in LDS, term k at A[256 k].  q is left transformed.
template <int NS>
__device__ __forceinline__ void pl_grad(const ltab& T, uint32_t ihi, uint32_t t,
                                        real (&q)[NS], real* A) {
  // q[p] <- W_p = sum_s (-1)^popcount(s & p) q[s]
#pragma unroll
  for (int bit = 1; bit < NS; bit <<= 1)
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (!(s & bit)) {
        const real a = q[s], b = q[s | bit];
        q[s] = a + b;
        q[s | bit] = a - b;
      }
  uint32_t g = 0, k = 0;
#pragma unroll
  for (int p = 0; p < NS; ++p) {
    const uint32_t ge = T.pg[p + 1];
    for (; g < ge; ++g) {
      const uint32_t gi = T.gi[g], ke = gi & 0xffffu, tm = gi >> 16;
      const real w = pauli_sgn((uint32_t)__popc(t & tm) & 1u, q[p]);
      for (; k < ke; ++k)
        A[256u * k] += pauli_sgn((uint32_t)__popc(ihi & T.zhi[k]) & 1u, w);  // (uniform sign)
    }
  }
}

// One span held in registers: f <- e^{-i phi} f, b <- e^{+i phi} b, the gradients' shares.
template <bool BWD, bool GRAD>
__device__ __forceinline__ void pl_span(const ltab& T, uint32_t ihi, uint32_t t,
                                        chunk (&fa)[PAULI_FU], chunk (&ba)[PAULI_FU],
                                        real* A) {
  pfix ph[PL_NS];
  pl_phases(T, ihi, t, ph);
  if constexpr (GRAD) {
    real q[PL_NS];
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const cx x = fa[u].v[v], y = ba[u].v[v];
        q[u * VEC + v] = fma(y.x, x.y, y.y * x.x);  // Im(b f)
      }
    pl_grad(T, ihi, t, q, A);
  }
#pragma unroll
  for (int u = 0; u < PAULI_FU; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const cx e = pl_cis(ph[u * VEC + v]);
      const cx x = fa[u].v[v];
      fa[u].v[v] = {fma(x.x, e.x, x.y * e.y), fma(x.y, e.x, -(x.x * e.y))};
      if constexpr (BWD) {
        const cx y = ba[u].v[v];
        ba[u].v[v] = {fma(y.x, e.x, -(y.y * e.y)), fma(y.y, e.x, y.x * e.y)};
      }
    }
}

// nch chunks of namps amplitudes (namps < VEC: a one-amplitude state in f32, one guarded chunk).
// GRAD: partials[block] = {A_0, A_1}, {A_2, A_3}, ...
template <bool BWD, bool GRAD>
__global__ __launch_bounds__(256) void k_player(cx* __restrict__ f, cx* __restrict__ b, ltab T,
                                                uint64_t nch, uint32_t namps,
                                                cx* __restrict__ partials) {
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  chunk* fc = reinterpret_cast<chunk*>(f);
  chunk* bc = reinterpret_cast<chunk*>(b);
  const uint32_t t = threadIdx.x;
  __shared__ real acc_lds[GRAD ? PL_GCAP : 1][256];
  real* A = &acc_lds[0][GRAD ? t : 0];
  if constexpr (GRAD) {
#pragma unroll
    for (int k = 0; k < (int)PL_GCAP; ++k) A[256u * k] = 0;
  }
  for (uint64_t s = (uint64_t)blockIdx.x * SPAN; s < nch; s += (uint64_t)gridDim.x * SPAN) {
    const uint32_t ihi = (uint32_t)(s / SPAN);
    chunk fa[PAULI_FU], ba[PAULI_FU];
    if (s + SPAN <= nch) {
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        fa[u] = ldc(fc + s + 256u * u + t);
        if constexpr (BWD) ba[u] = ldc(bc + s + 256u * u + t);
      }
      pl_span<BWD, GRAD>(T, ihi, t, fa, ba, A);
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        stc(fc + s + 256u * u + t, fa[u]);
        if constexpr (BWD) stc(bc + s + 256u * u + t, ba[u]);
      }
    } else {  // a state below one span (s = 0): chunks past it read as zeros and are not stored
      const bool part = namps < (uint32_t)VEC;  // below one chunk: nch = 1
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        const uint64_t ci = s + 256u * u + t;
        fa[u] = chunk{};
        ba[u] = chunk{};
        if (ci < nch) {
          fa[u] = part ? pauli_ld(f, 0, namps) : ldc(fc + ci);
          if constexpr (BWD) ba[u] = part ? pauli_ld(b, 0, namps) : ldc(bc + ci);
        }
      }
      pl_span<BWD, GRAD>(T, ihi, t, fa, ba, A);
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        const uint64_t ci = s + 256u * u + t;
        if (ci >= nch) continue;
        if (part) {
          pauli_st(f, 0, namps, fa[u]);
          if constexpr (BWD) pauli_st(b, 0, namps, ba[u]);
        } else {
          stc(fc + ci, fa[u]);
          if constexpr (BWD) stc(bc + ci, ba[u]);
        }
      }
    }
  }
  if constexpr (GRAD) {
    cx acc[RED];
#pragma unroll
    for (int j = 0; j < RED; ++j) acc[j] = {A[256u * (2 * j)], A[256u * (2 * j + 1)]};
    block_reduce_store<RED>(acc, partials + (uint64_t)blockIdx.x * RED);
  }
}

// ---- host ----------------------------------------------------------------------------------
// theta / 4 pi in 2^-B turns, mod 2^B
inline pfix pl_fix(double theta) {
  constexpr int B = 8 * (int)sizeof(pfix);
  long double x = (long double)theta / (4.0L * 3.14159265358979323846264338327950288L);
  x -= floorl(x);
  const long double y = roundl(ldexpl(x, B));
  return y >= ldexpl(1.0L, B) ? (pfix)0 : (pfix)y;
}

inline const char* pl_check(const unsigned long long* zm, const double* theta, size_t terms,
                            size_t n) {
  if (terms == 0) return fail("The layer has no terms.");
  if (!zm) return fail("The layer has no masks.");
  for (size_t k = 0; k < terms; ++k) {
    if ((zm[k] >> n) != 0) return fail("pos is out of the bound.");
    if (theta && !std::isfinite(theta[k])) return fail("Pauli coefficients must be finite.");
  }
  return nullptr;
}

// low mask of a term on n qubits (n < L: the whole mask)
inline uint32_t pl_low(uint64_t z, uint32_t lv = LV) {
  return (uint32_t)(z & ((1u << pl_span_bits(lv)) - 1u));
}

// The table of terms [k0, k1) (k1 - k0 <= PL_CAP), ordered by slot pattern, low mask and term
// number; perm[j] = the term at table place j.  theta == nullptr: the shape only.
inline void pl_table(const unsigned long long* zm, const double* theta, size_t k0, size_t k1,
                     bool reverse, ltab& T, uint32_t* perm, uint32_t lv = LV) {
  T = ltab{};
  std::vector<uint32_t> ord(k1 - k0);
  for (size_t j = 0; j < ord.size(); ++j) ord[j] = (uint32_t)(k0 + j);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t ma = pl_low(zm[a], lv), mb = pl_low(zm[b], lv);
    return std::make_pair(pl_pattern(ma, lv), ma) < std::make_pair(pl_pattern(mb, lv), mb);
  });
  T.nt = (uint32_t)ord.size();
  uint32_t ng = 0;
  for (uint32_t j = 0; j < T.nt; ++j) {
    const uint64_t z = zm[ord[j]];
    const uint32_t m = pl_low(z, lv), p = pl_pattern(m, lv);
    if (j == 0 || pl_low(zm[ord[j - 1]], lv) != m) ++ng;  // a new group
    T.gi[ng - 1] = (j + 1) | (pl_tmask(m, lv) << 16);
    for (uint32_t pp = p + 1; pp <= (uint32_t)PL_NS; ++pp) T.pg[pp] = (uint16_t)ng;
    T.zhi[j] = (uint32_t)(z >> pl_span_bits(lv));
    const pfix t = theta ? pl_fix(theta[ord[j]]) : (pfix)0;
    T.t[j] = reverse ? (pfix)0 - t : t;
    if (perm) perm[j] = ord[j];
  }
}

struct PauliLayerPlan {
  unsigned groups = 0, high = 0, fwd = 0, rev = 0, rev_grad = 0;
};
inline PauliLayerPlan pl_plan(const unsigned long long* zm, size_t terms, uint32_t lv = LV) {
  PauliLayerPlan P;
  std::vector<uint32_t> low(terms);
  for (size_t k = 0; k < terms; ++k) {
    low[k] = pl_low(zm[k], lv);
    if ((zm[k] >> pl_span_bits(lv)) != 0) ++P.high;
  }
  std::sort(low.begin(), low.end());
  P.groups = (unsigned)(std::unique(low.begin(), low.end()) - low.begin());
  P.fwd = P.rev = (unsigned)((terms + PL_CAP - 1) / PL_CAP);
  P.rev_grad = (unsigned)((terms + PL_GCAP - 1) / PL_GCAP);
  return P;
}

inline uint32_t pl_grid(uint32_t n, uint32_t cap) {
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  return pauli_grid((prot_chunks(n) + SPAN - 1) / SPAN, cap);
}

template <bool BWD, bool GRAD>
inline const char* pl_launch(Ctx& c, const char* name, double bytes, cx* f, cx* b, const ltab& T,
                             uint32_t n, uint32_t grid, cx* out) {
  return c.launch_block(name, bytes, k_player<BWD, GRAD>, grid, 256u, f, b, T, prot_chunks(n),
                        (uint32_t)std::min<uint64_t>((uint64_t)1 << n, VEC), out);
}

// How a layer's launches run: the diagonal kernel here, the paired ones in qdc_paulixlayer.hpp.
struct PlDiag {
  uint32_t lv = LV;
  const char *fwd_name = "pauli_layer", *rev_name = "pauli_layer_rev";
  uint32_t grid(uint32_t n, uint32_t cap) const { return pl_grid(n, cap); }
  template <bool BWD, bool GRAD>
  const char* launch(Ctx& c, const char* name, double bytes, cx* f, cx* b, const ltab& T,
                     uint32_t n, uint32_t grid, cx* out) const {
    return pl_launch<BWD, GRAD>(c, name, bytes, f, b, T, n, grid, out);
  }
};

// s <- U s
template <class R>
inline const char* pl_forward(Ctx& c, const R& r, cx* s, const unsigned long long* zm,
                              const double* theta, size_t terms, uint32_t n) {
  const uint32_t grid = r.grid(n, 1u << 20);
  ltab T;
  for (size_t k0 = 0; k0 < terms; k0 += PL_CAP) {
    pl_table(zm, theta, k0, std::min(terms, k0 + PL_CAP), false, T, nullptr, r.lv);
    QDC_TRY((r.template launch<false, false>(c, r.fwd_name, 2.0 * state_bytes(n), s, nullptr, T,
                                             n, grid, nullptr)));
  }
  return nullptr;
}

// f <- U^-1 f; b <- U^T b (b != nullptr); dtheta[k] += 1/2 sum s_k q (dtheta != nullptr: one stream
// synchronisation per FIN_MAX reducing launches, FIN_MAX * PL_GCAP = 1024 terms).
template <class R>
inline const char* pl_reverse(Ctx& c, const R& r, cx* f, cx* b, const unsigned long long* zm,
                              const double* theta, size_t terms, uint32_t n, double* dtheta) {
  const char* name = r.rev_name;
  ltab T;
  if (!dtheta) {
    const uint32_t grid = r.grid(n, 1u << 20);
    for (size_t k0 = 0; k0 < terms; k0 += PL_CAP) {
      pl_table(zm, theta, k0, std::min(terms, k0 + PL_CAP), true, T, nullptr, r.lv);
      if (b)
        QDC_TRY((r.template launch<true, false>(c, name, 4.0 * state_bytes(n), f, b, T, n, grid,
                                                nullptr)));
      else
        QDC_TRY((r.template launch<false, false>(c, name, 2.0 * state_bytes(n), f, nullptr, T, n,
                                                 grid, nullptr)));
    }
    return nullptr;
  }
  const uint32_t grid = r.grid(n, c.k.red_cap);
  const size_t nl = (terms + PL_GCAP - 1) / PL_GCAP;
  std::vector<uint32_t> perm(terms);
  for (size_t l0 = 0; l0 < nl; l0 += FIN_MAX) {
    const size_t l1 = std::min<size_t>(nl, l0 + FIN_MAX);
    for (size_t l = l0; l < l1; ++l) {
      const size_t k0 = l * PL_GCAP;
      pl_table(zm, theta, k0, std::min(terms, k0 + PL_GCAP), true, T, perm.data() + k0, r.lv);
      QDC_TRY(reduce_into(c, c.results, (uint32_t)(l - l0), 0, grid, [&](cx* out) {
        return r.template launch<true, true>(c, name, 4.0 * state_bytes(n), f, b, T, n, grid, out);
      }));
    }
    QDC_TRY(c.flush());
    QDC_HIP(hipMemcpyAsync(c.host_results, c.results, sizeof(cx) * RED * (l1 - l0),
                           hipMemcpyDeviceToHost, c.stream));
    QDC_HIP(hipStreamSynchronize(c.stream));
    for (size_t l = l0; l < l1; ++l) {
      const size_t k0 = l * PL_GCAP, k1 = std::min(terms, k0 + PL_GCAP);
      for (size_t j = 0; j < k1 - k0; ++j) {
        const cx v = c.host_results[(l - l0) * RED + j / 2];
        dtheta[perm[k0 + j]] += 0.5 * (double)(j & 1 ? v.y : v.x);
      }
    }
  }
  return nullptr;
}

inline const char* pauli_layer(Ctx& c, cx* s, const unsigned long long* zm, const double* theta,
                               size_t terms, uint32_t n) {
  return pl_forward(c, PlDiag{}, s, zm, theta, terms, n);
}
inline const char* pauli_layer_reverse(Ctx& c, cx* f, cx* b, const unsigned long long* zm,
                                       const double* theta, size_t terms, uint32_t n,
                                       double* dtheta) {
  return pl_reverse(c, PlDiag{}, f, b, zm, theta, terms, n, dtheta);
}

}  // namespace qdc

// qdc_paulixlayer.hpp — Pauli layers with a shared X/Y footprint (include/qdc/pauli.h:
// qdc_pauli_xlayer, qdc_pauli_xlayer_reverse): K commuting rotations about strings P_k = (x, z_k)
// with one x != 0 in one pass,  U = exp(-i/2 sum_k theta_k P_k).
//
// With nY_k = popcount(x & z_k), j = i ^ x and s_k(i) = (-1)^popcount(i & z_k):
//     (P_k psi)[i] = i^nY_k (-1)^popcount(j & z_k) psi[j] = ph0 eps_k s_k(i) psi[j]
// where the strings commute iff every nY_k has one parity par, ph0 = i^par, and
// eps_k = (-1)^((nY_k - par) / 2 + nY_k) is a sign of the host.  On a pair (i, j) the generator
// sum_k theta_k P_k is r(i) [[0, ph0], [conj ph0, 0]], r(i) = sum_k eps_k theta_k s_k(i), and
// r(j) = (-1)^par r(i).  With phi = r(i) / 2:
//     out[i] = cos phi psi[i] - i ph0      sin phi psi[j]
//     out[j] = cos phi psi[j] - i conj ph0 sin phi psi[i]
// phi is the diagonal layer's phase (qdc_paulilayer.hpp) for the angles eps_k theta_k: summed in
// fixed point, one sincospi per PAIR.
//
// The pair belongs to its end i with bit hb (the highest set bit of x) clear.  Deleting bit hb
// from i and from every z_k leaves an ordinary diagonal-layer phase on the (n-1)-bit pair index
// p: the table (pl_table), the phases (pl_phases) and the gradient walk (pl_grad) are the diagonal
// layer's, run on the reduced masks.  A Z or Y on qubit hb only enters nY_k and eps_k.
//   k_pxlayer (x >> LV != 0): chunk pair cp of nch / 2 is ci = cp with a zero inserted at bit
//     hb - LV, cj = ci ^ (x >> LV) (k_prot_pair's addressing); amplitude v of the pair has the
//     pair index p = cp * VEC + v, so a span of 256 * PAULI_FU chunk pairs is 2^L pair indices
//     laid out like k_player's amplitudes.
//   k_pxlayer_self (f32, x = 1): a chunk is one pair (owner v = 0), the pair index is the chunk's
//     number: L - 1 index bits per span and PAULI_FU slots per thread (lv = 0 in pl_table).
//
// Reverse: fwd <- U(-theta) fwd (the table negated), bwd <- U^T bwd; P^T = (-1)^nY P, so U^T is
// U(theta) at par = 0 and U(-theta) at par = 1.  Gradients, fwd and bwd as the call receives them:
//     dL/dtheta_k = 1/2 Im sum_i bwd[i] (P_k fwd)[i] = 1/2 eps_k sum_pairs s_k(p) q(pair),
//     q = Im(ph0 b_i f_j + conj ph0 b_j f_i)
// one real q per pair, then pl_grad's walk with the accumulators in LDS, block_reduce_store,
// reduce_into, k_finalize: no atomics.  q-weighted sums do not change under the other (commuting)
// terms, so a layer split over launches is exact; the caps are the diagonal layer's.
#pragma once

#include "qdc_paulilayer.hpp"

namespace qdc {

struct pxgeo {
  uint64_t xc;   // x >> LV: the partner chunk is ci ^ xc
  uint32_t hbc;  // highest set bit of xc
  uint32_t par;  // nY & 1 of every string
  uint32_t x0;   // f32: bit 0 of x (the partner chunk's amplitudes are swapped)
};

// One amplitude pair, e = (cos phi, sin phi):  (fi, fj) <- U (fi, fj); BWD: (bi, bj) <- U^T of
// the OPPOSITE angle's table (the reverse step: e belongs to -theta).
template <bool BWD>
__device__ __forceinline__ void px_mix(uint32_t par, cx e, cx& fi, cx& fj, cx& bi, cx& bj) {
  // -i ph0 a_j and -i conj(ph0) a_i: (-i a_j, -i a_i) at par = 0, (a_j, -a_i) at par = 1
  const real c = e.x, s = e.y;
  {
    const cx wj = par ? fj : cx{fj.y, -fj.x};
    const cx wi = par ? cx{-fi.x, -fi.y} : cx{fi.y, -fi.x};
    const cx oi = {fma(s, wj.x, c * fi.x), fma(s, wj.y, c * fi.y)};
    const cx oj = {fma(s, wi.x, c * fj.x), fma(s, wi.y, c * fj.y)};
    fi = oi;
    fj = oj;
  }
  if constexpr (BWD) {
    const real sb = par ? s : -s;
    const cx wj = par ? bj : cx{bj.y, -bj.x};
    const cx wi = par ? cx{-bi.x, -bi.y} : cx{bi.y, -bi.x};
    const cx oi = {fma(sb, wj.x, c * bi.x), fma(sb, wj.y, c * bi.y)};
    const cx oj = {fma(sb, wi.x, c * bj.x), fma(sb, wi.y, c * bj.y)};
    bi = oi;
    bj = oj;
  }
}

// q = Im(ph0 b_i f_j + conj(ph0) b_j f_i)
__device__ __forceinline__ real px_q(uint32_t par, cx fi, cx fj, cx bi, cx bj) {
  const real q0 = fma(bi.x, fj.y, bi.y * fj.x) + fma(bj.x, fi.y, bj.y * fi.x);  // Im(bi fj + bj fi)
  const real q1 = fma(bi.x, fj.x, -(bi.y * fj.y)) - fma(bj.x, fi.x, -(bj.y * fi.y));  // Re(bi fj - bj fi)
  return par ? q1 : q0;
}

// One span of chunk pairs in registers: fa / ba = the owners' chunks, fb / bb = their partners'
// (swapped so that amplitude v of both is a pair).
template <bool BWD, bool GRAD>
__device__ __forceinline__ void px_span(const ltab& T, uint32_t par, uint32_t ihi, uint32_t t,
                                        chunk (&fa)[PAULI_FU], chunk (&fb)[PAULI_FU],
                                        chunk (&ba)[PAULI_FU], chunk (&bb)[PAULI_FU], real* A) {
  pfix ph[PL_NS];
  pl_phases(T, ihi, t, ph);
  if constexpr (GRAD) {
    real q[PL_NS];
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        q[u * VEC + v] = px_q(par, fa[u].v[v], fb[u].v[v], ba[u].v[v], bb[u].v[v]);
    pl_grad(T, ihi, t, q, A);
  }
#pragma unroll
  for (int u = 0; u < PAULI_FU; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      px_mix<BWD>(par, pl_cis(ph[u * VEC + v]), fa[u].v[v], fb[u].v[v], ba[u].v[v], bb[u].v[v]);
}

// npairs = nch / 2 chunk pairs.  GRAD: partials[block] = {A_0, A_1}, {A_2, A_3}, ...
template <bool BWD, bool GRAD>
__global__ __launch_bounds__(256) void k_pxlayer(cx* __restrict__ f, cx* __restrict__ b, ltab T,
                                                 pxgeo G, uint64_t npairs,
                                                 cx* __restrict__ partials) {
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  chunk* fc = reinterpret_cast<chunk*>(f);
  chunk* bc = reinterpret_cast<chunk*>(b);
  const uint32_t t = threadIdx.x;
  const bool x0 = VEC == 2 && G.x0 != 0;
  __shared__ real acc_lds[GRAD ? PL_GCAP : 1][256];
  real* A = &acc_lds[0][GRAD ? t : 0];
  if constexpr (GRAD) {
#pragma unroll
    for (int k = 0; k < (int)PL_GCAP; ++k) A[256u * k] = 0;
  }
  for (uint64_t s = (uint64_t)blockIdx.x * SPAN; s < npairs; s += (uint64_t)gridDim.x * SPAN) {
    const uint32_t ihi = (uint32_t)(s / SPAN);
    uint64_t ci[PAULI_FU], cj[PAULI_FU];
    chunk fa[PAULI_FU], fb[PAULI_FU], ba[PAULI_FU], bb[PAULI_FU];
    if (s + SPAN <= npairs) {  // every load of the span before its first store
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        ci[u] = insert_zero(s + 256u * u + t, G.hbc);
        cj[u] = ci[u] ^ G.xc;
        fa[u] = ldc(fc + ci[u]);
        fb[u] = prot_swap(ldc(fc + cj[u]), x0);
        if constexpr (BWD) {
          ba[u] = ldc(bc + ci[u]);
          bb[u] = prot_swap(ldc(bc + cj[u]), x0);
        }
      }
      px_span<BWD, GRAD>(T, G.par, ihi, t, fa, fb, ba, bb, A);
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        stc(fc + ci[u], fa[u]);
        stc(fc + cj[u], prot_swap(fb[u], x0));
        if constexpr (BWD) {
          stc(bc + ci[u], ba[u]);
          stc(bc + cj[u], prot_swap(bb[u], x0));
        }
      }
    } else {  // a state below one span (s = 0): pairs past it read as zeros and are not stored
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        const uint64_t cp = s + 256u * u + t;
        const bool in = cp < npairs;
        ci[u] = insert_zero(in ? cp : 0, G.hbc);
        cj[u] = ci[u] ^ G.xc;
        fa[u] = fb[u] = ba[u] = bb[u] = chunk{};
        if (in) {
          fa[u] = ldc(fc + ci[u]);
          fb[u] = prot_swap(ldc(fc + cj[u]), x0);
          if constexpr (BWD) {
            ba[u] = ldc(bc + ci[u]);
            bb[u] = prot_swap(ldc(bc + cj[u]), x0);
          }
        }
      }
      px_span<BWD, GRAD>(T, G.par, ihi, t, fa, fb, ba, bb, A);
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        if (s + 256u * u + t >= npairs) continue;
        stc(fc + ci[u], fa[u]);
        stc(fc + cj[u], prot_swap(fb[u], x0));
        if constexpr (BWD) {
          stc(bc + ci[u], ba[u]);
          stc(bc + cj[u], prot_swap(bb[u], x0));
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

#ifndef QDC_F64
// f32, x = 1: chunk c = {psi[2c], psi[2c + 1]} is pair c.  The table is built with lv = 0.
template <bool BWD, bool GRAD>
__device__ __forceinline__ void px_span_self(const ltab& T, uint32_t par, uint32_t ihi, uint32_t t,
                                             chunk (&fa)[PAULI_FU], chunk (&ba)[PAULI_FU],
                                             real* A) {
  pfix ph[PAULI_FU];
  pl_phases(T, ihi, t, ph);
  if constexpr (GRAD) {
    real q[PAULI_FU];
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) q[u] = px_q(par, fa[u].v[0], fa[u].v[1], ba[u].v[0], ba[u].v[1]);
    pl_grad(T, ihi, t, q, A);
  }
#pragma unroll
  for (int u = 0; u < PAULI_FU; ++u)
    px_mix<BWD>(par, pl_cis(ph[u]), fa[u].v[0], fa[u].v[1], ba[u].v[0], ba[u].v[1]);
}

// nch >= 1 whole chunks (x = 1 needs n >= 1).
template <bool BWD, bool GRAD>
__global__ __launch_bounds__(256) void k_pxlayer_self(cx* __restrict__ f, cx* __restrict__ b,
                                                      ltab T, uint32_t par, uint64_t nch,
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
    const bool whole = s + SPAN <= nch;
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) {
      const uint64_t ci = s + 256u * u + t;
      fa[u] = ba[u] = chunk{};
      if (whole || ci < nch) {  // (chunks past a small state read as zeros and are not stored)
        fa[u] = ldc(fc + ci);
        if constexpr (BWD) ba[u] = ldc(bc + ci);
      }
    }
    px_span_self<BWD, GRAD>(T, par, ihi, t, fa, ba, A);
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) {
      const uint64_t ci = s + 256u * u + t;
      if (!whole && ci >= nch) continue;
      stc(fc + ci, fa[u]);
      if constexpr (BWD) stc(bc + ci, ba[u]);
    }
  }
  if constexpr (GRAD) {
    cx acc[RED];
#pragma unroll
    for (int j = 0; j < RED; ++j) acc[j] = {A[256u * (2 * j)], A[256u * (2 * j + 1)]};
    block_reduce_store<RED>(acc, partials + (uint64_t)blockIdx.x * RED);
  }
}
#endif

// ---- host ----------------------------------------------------------------------------------
// A shared-footprint layer as a diagonal layer on the pair index.
struct PxLayer {
  uint32_t lv = LV;      // pl_table's layout: LV, or 0 for the self-paired form
  const char *fwd_name = "pauli_xlayer", *rev_name = "pauli_xlayer_rev";
  bool self = false;     // x < VEC
  uint32_t hb = 0;       // the deleted bit: the highest set bit of x
  pxgeo G{};
  std::vector<unsigned long long> zr;  // z_k without bit hb
  std::vector<double> eps;             // eps_k

  uint64_t items(uint32_t n) const { return self ? prot_chunks(n) : prot_chunks(n) / 2; }
  uint32_t grid(uint32_t n, uint32_t cap) const {
    constexpr uint64_t SPAN = 256u * PAULI_FU;
    return pauli_grid((items(n) + SPAN - 1) / SPAN, cap);
  }
  // the table and the geometry against the state, before anything reaches the device
  const char* check(const ltab& T, uint32_t n, bool grad) const {
    const uint32_t ns = (uint32_t)PAULI_FU << lv;
    bool ok = T.nt >= 1 && T.nt <= (grad ? PL_GCAP : PL_CAP) && T.pg[0] == 0 && T.pg[ns] <= T.nt;
    for (uint32_t p = 0; ok && p < ns; ++p) ok = T.pg[p] <= T.pg[p + 1];
    for (uint32_t g = 0; ok && g < T.pg[ns]; ++g)
      ok = (T.gi[g] & 0xffffu) <= T.nt && (g == 0 || (T.gi[g - 1] & 0xffffu) <= (T.gi[g] & 0xffffu));
    ok = ok && (T.pg[ns] == 0 || (T.gi[T.pg[ns] - 1] & 0xffffu) == T.nt);
    const uint64_t nch = prot_chunks(n);
    if (self)
      ok = ok && VEC == 2 && n >= 1;
    else
      ok = ok && nch >= 2 && G.xc != 0 && G.xc < nch && (G.xc >> G.hbc) == 1;
    return ok ? nullptr : fail("invalid Pauli layer table");
  }
  template <bool BWD, bool GRAD>
  const char* launch(Ctx& c, const char* name, double bytes, cx* f, cx* b, const ltab& T,
                     uint32_t n, uint32_t grid, cx* out) const {
    QDC_TRY(check(T, n, GRAD));
#ifndef QDC_F64
    if (self)
      return c.launch_block(name, bytes, k_pxlayer_self<BWD, GRAD>, grid, 256u, f, b, T, G.par,
                            prot_chunks(n), out);
#endif
    return c.launch_block(name, bytes, k_pxlayer<BWD, GRAD>, grid, 256u, f, b, T, G,
                          prot_chunks(n) / 2, out);
  }
};

// x != 0.  theta == nullptr: the shape only.  The checks of pl_check first, in its order.
inline const char* pxl_make(unsigned long long x, const unsigned long long* zm,
                            const double* theta, size_t terms, size_t n, PxLayer& P) {
  QDC_TRY(pl_check(zm, theta, terms, n));
  if ((x >> n) != 0) return fail("pos is out of the bound.");
  P = PxLayer{};
  const uint32_t par = (uint32_t)__builtin_popcountll(x & zm[0]) & 1u;
  while (((x >> P.hb) >> 1) != 0) ++P.hb;
  P.self = (x >> LV) == 0;
  P.lv = P.self ? 0u : (uint32_t)LV;
  P.G.xc = (uint64_t)x >> LV;
  P.G.hbc = P.self ? 0u : P.hb - (uint32_t)LV;
  P.G.par = par;
  P.G.x0 = (uint32_t)(x & 1u);
  P.zr.resize(terms);
  P.eps.resize(terms);
  const unsigned long long lowm = ((unsigned long long)1 << P.hb) - 1;
  for (size_t k = 0; k < terms; ++k) {
    const uint32_t ny = (uint32_t)__builtin_popcountll(x & zm[k]);
    if ((ny & 1u) != par) return fail("The strings of a layer must commute.");
    P.eps[k] = (((ny - par) / 2 + ny) & 1u) ? -1.0 : 1.0;
    P.zr[k] = (zm[k] & lowm) | ((zm[k] >> (P.hb + 1)) << P.hb);
  }
  return nullptr;
}

// eps_k theta_k
inline std::vector<double> pxl_angles(const PxLayer& P, const double* theta) {
  std::vector<double> te(P.eps.size());
  for (size_t k = 0; k < te.size(); ++k) te[k] = P.eps[k] * theta[k];
  return te;
}

// s <- U s
inline const char* pauli_xlayer(Ctx& c, cx* s, const PxLayer& P, const double* theta, uint32_t n) {
  const std::vector<double> te = pxl_angles(P, theta);
  return pl_forward(c, P, s, P.zr.data(), te.data(), te.size(), n);
}

// f <- U^-1 f; b <- U^T b (b != nullptr); dtheta[k] += dL/dtheta_k (dtheta != nullptr)
inline const char* pauli_xlayer_reverse(Ctx& c, cx* f, cx* b, const PxLayer& P,
                                        const double* theta, uint32_t n, double* dtheta) {
  const std::vector<double> te = pxl_angles(P, theta);
  if (!dtheta) return pl_reverse(c, P, f, b, P.zr.data(), te.data(), te.size(), n, nullptr);
  std::vector<double> d(te.size(), 0.0);
  QDC_TRY(pl_reverse(c, P, f, b, P.zr.data(), te.data(), te.size(), n, d.data()));
  for (size_t k = 0; k < d.size(); ++k) dtheta[k] += P.eps[k] * d[k];
  return nullptr;
}

}  // namespace qdc

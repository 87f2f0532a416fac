// qdc_paulirot.hpp — Pauli-rotation gates R(theta; P) = exp(-i theta/2 P) = cos(theta/2) I -
// i sin(theta/2) P (include/qdc/pauli.h: qdc_pauli_rot, qdc_pauli_rot_reverse), P = (x, z) as in
// qdc_pauli.hpp: (P psi)[i] = ph sgn(j) psi[j], j = i ^ x, ph = i^nY, sgn(j) = (-1)^popcount(j & z).
//
// With c = cos(theta/2), s = sin(theta/2) (host, double, rounded once) and m = -i s ph:
//     (R psi)[a]        = c psi[a] + sgn(a ^ x) m psi[a ^ x]
//     (R(-theta) psi)[a] = c psi[a] - sgn(a ^ x) m psi[a ^ x]            (the uncompute)
//     (R^T psi)[a]       = c psi[a] + sgn(a ^ x) (-1)^nY m psi[a ^ x]    (P^T = (-1)^nY P)
// and over a pair (i, j = i ^ x), sgn(i) = (-1)^nY sgn(j): one popcount serves both ends,
//     out[i] = c psi[i] + sgn(j) m psi[j],   out[j] = c psi[j] + sgn(j) m2 psi[i],  m2 = (-1)^nY m.
// The gradient of the angle needs no uncomputed value (dR/dtheta = -(i/2) P R):
//     dL/dtheta = 1/2 Im sum_i bwd[i] (P fwd_out)[i] = 1/2 Im(ph S),  S = sum_i sgn(j) bwd[i] fwd_out[j]
// and a pair adds sgn(j) (b_i f_j + (-1)^nY b_j f_i) to S.  The kernels reduce S (block_reduce_store,
// the context's reduction slots, k_finalize: no atomics); the host applies ph and the 1/2.
//
// Both kernels work on 16-byte chunks.  Chunk c pairs with chunk c ^ xc, xc = x >> log2(VEC); in
// f32 with bit 0 of x set the partner chunk's two amplitudes are swapped.
//   k_prot_pair (xc != 0): chunk pair p of nch / 2 is ci = p with a zero inserted at the highest
//     set bit of xc, cj = ci ^ xc; each chunk is read and written once, in place.
//   k_prot_self (xc == 0: x = 0, the diagonal strings and the identity; x = 1 in f32): a chunk
//     pairs with itself, elementwise over the chunks.
// Blocks stride over spans of 256 * PAULI_FU items; a span inside the state keeps PAULI_FU items
// per thread in flight, the last span of a state that is no multiple of it (and a state below
// one chunk) goes item by item behind a bound (pauli_ld / pauli_st).
#pragma once

#include "qdc_pauli.hpp"

namespace qdc {

struct prot {
  uint64_t x, z;
  uint32_t hbc;  // highest set bit of x >> LV (k_prot_pair)
  uint32_t nyp;  // nY & 1
  real c;        // cos(theta / 2)
  cx mf, mf2;    // fwd: f[i] <- c f[i] + sgn(j) mf f[j], f[j] <- c f[j] + sgn(j) mf2 f[i]
  cx mb, mb2;    // bwd: the same with (mb, mb2)
};

__device__ __forceinline__ cx prot_sgn(uint32_t parity, cx m) {
  return {pauli_sgn(parity, m.x), pauli_sgn(parity, m.y)};
}
// c a + m b
__device__ __forceinline__ cx prot_mix(real c, cx a, cx m, cx b) {
  return cfma(m, b, cx{c * a.x, c * a.y});
}
// the chunk with its two amplitudes swapped where x0 is set (f32; f64 chunks hold one)
__device__ __forceinline__ chunk prot_swap(const chunk& r, bool x0) {
  if constexpr (VEC == 2) {
    chunk o;
    o.v[0] = x0 ? r.v[1] : r.v[0];
    o.v[1] = x0 ? r.v[0] : r.v[1];
    return o;
  } else {
    return r;
  }
}

// One chunk pair: fa / ba = chunk ci of fwd / bwd, fb / bb = chunk cj, the latter swapped so that
// amplitude v of both has the index pair (i, i ^ x).  acc += the pair's share of S.
template <bool BWD, bool GRAD>
__device__ __forceinline__ void prot_pair(const prot& T, uint64_t ci, chunk& fa, chunk& fb,
                                          chunk& ba, chunk& bb, cx& acc) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint64_t j = (ci * VEC + v) ^ T.x;
    const uint32_t par = (uint32_t)__popcll(j & T.z);
    const cx fi = fa.v[v], fj = fb.v[v];
    if constexpr (GRAD) {
      const cx t = cfma(ba.v[v], fj, prot_sgn(T.nyp, cmul(bb.v[v], fi)));
      acc = cadd(acc, prot_sgn(par, t));
    }
    fa.v[v] = prot_mix(T.c, fi, prot_sgn(par, T.mf), fj);
    fb.v[v] = prot_mix(T.c, fj, prot_sgn(par, T.mf2), fi);
    if constexpr (BWD) {
      const cx bi = ba.v[v], bj = bb.v[v];
      ba.v[v] = prot_mix(T.c, bi, prot_sgn(par, T.mb), bj);
      bb.v[v] = prot_mix(T.c, bj, prot_sgn(par, T.mb2), bi);
    }
  }
}

// One self-paired chunk (x < VEC): amplitude a takes its partner a ^ x from the same chunk.
template <bool BWD, bool GRAD>
__device__ __forceinline__ void prot_self(const prot& T, uint64_t ci, chunk& f, chunk& b,
                                          cx& acc) {
  const bool x0 = (T.x & 1u) != 0;
  const chunk fp = prot_swap(f, x0);
  chunk bp;
  if constexpr (BWD) bp = prot_swap(b, x0);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint64_t j = (ci * VEC + v) ^ T.x;
    const uint32_t par = (uint32_t)__popcll(j & T.z);
    if constexpr (GRAD) acc = cadd(acc, prot_sgn(par, cmul(b.v[v], fp.v[v])));
    f.v[v] = prot_mix(T.c, f.v[v], prot_sgn(par, T.mf), fp.v[v]);
    if constexpr (BWD) b.v[v] = prot_mix(T.c, b.v[v], prot_sgn(par, T.mb), bp.v[v]);
  }
}

// npairs = nch / 2 chunk pairs.  BWD: b is pulled back too; GRAD: partials[block] = {S share}.
template <bool BWD, bool GRAD>
__global__ __launch_bounds__(256) void k_prot_pair(cx* __restrict__ f, cx* __restrict__ b, prot T,
                                                   uint64_t npairs, cx* __restrict__ partials) {
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  chunk* fc = reinterpret_cast<chunk*>(f);
  chunk* bc = reinterpret_cast<chunk*>(b);
  const uint64_t xc = T.x >> LV;
  const bool x0 = VEC == 2 && (T.x & 1u) != 0;
  cx acc = {0, 0};
  for (uint64_t s = (uint64_t)blockIdx.x * SPAN; s < npairs; s += (uint64_t)gridDim.x * SPAN) {
    if (s + SPAN <= npairs) {  // a whole span: PAULI_FU pairs of each state in flight
      uint64_t ci[PAULI_FU], cj[PAULI_FU];
      chunk fa[PAULI_FU], fb[PAULI_FU], ba[PAULI_FU], bb[PAULI_FU];
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        ci[u] = insert_zero(s + 256u * u + threadIdx.x, T.hbc);
        cj[u] = ci[u] ^ xc;
        fa[u] = ldc(fc + ci[u]);
        fb[u] = ldc(fc + cj[u]);
        if constexpr (BWD) {
          ba[u] = ldc(bc + ci[u]);
          bb[u] = ldc(bc + cj[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        fb[u] = prot_swap(fb[u], x0);
        if constexpr (BWD) bb[u] = prot_swap(bb[u], x0);
        prot_pair<BWD, GRAD>(T, ci[u], fa[u], fb[u], ba[u], bb[u], acc);
        stc(fc + ci[u], fa[u]);
        stc(fc + cj[u], prot_swap(fb[u], x0));
        if constexpr (BWD) {
          stc(bc + ci[u], ba[u]);
          stc(bc + cj[u], prot_swap(bb[u], x0));
        }
      }
    } else {  // the tail (a state below one span is all tail)
      for (int u = 0; u < PAULI_FU; ++u) {
        const uint64_t p = s + 256u * u + threadIdx.x;
        if (p >= npairs) break;
        const uint64_t ci = insert_zero(p, T.hbc), cj = ci ^ xc;
        chunk fa = ldc(fc + ci), fb = prot_swap(ldc(fc + cj), x0), ba, bb;
        if constexpr (BWD) {
          ba = ldc(bc + ci);
          bb = prot_swap(ldc(bc + cj), x0);
        }
        prot_pair<BWD, GRAD>(T, ci, fa, fb, ba, bb, acc);
        stc(fc + ci, fa);
        stc(fc + cj, prot_swap(fb, x0));
        if constexpr (BWD) {
          stc(bc + ci, ba);
          stc(bc + cj, prot_swap(bb, x0));
        }
      }
    }
  }
  if constexpr (GRAD) {
    cx a1[1] = {acc};
    block_reduce_store<1>(a1, partials + (uint64_t)blockIdx.x * RED);
  }
}

// nch chunks of namps amplitudes (namps < VEC: a one-amplitude state in f32, one guarded chunk).
template <bool BWD, bool GRAD>
__global__ __launch_bounds__(256) void k_prot_self(cx* __restrict__ f, cx* __restrict__ b, prot T,
                                                   uint64_t nch, uint32_t namps,
                                                   cx* __restrict__ partials) {
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  chunk* fc = reinterpret_cast<chunk*>(f);
  chunk* bc = reinterpret_cast<chunk*>(b);
  cx acc = {0, 0};
  for (uint64_t s = (uint64_t)blockIdx.x * SPAN; s < nch; s += (uint64_t)gridDim.x * SPAN) {
    if (s + SPAN <= nch) {
      chunk fa[PAULI_FU], ba[PAULI_FU];
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        fa[u] = ldc(fc + s + 256u * u + threadIdx.x);
        if constexpr (BWD) ba[u] = ldc(bc + s + 256u * u + threadIdx.x);
      }
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) {
        const uint64_t ci = s + 256u * u + threadIdx.x;
        prot_self<BWD, GRAD>(T, ci, fa[u], ba[u], acc);
        stc(fc + ci, fa[u]);
        if constexpr (BWD) stc(bc + ci, ba[u]);
      }
    } else {
      for (int u = 0; u < PAULI_FU; ++u) {
        const uint64_t ci = s + 256u * u + threadIdx.x;
        if (ci >= nch) break;
        // (a state below one chunk: nch = 1, its amplitudes and zeros)
        const bool part = namps < (uint32_t)VEC;
        chunk fa = part ? pauli_ld(f, 0, namps) : ldc(fc + ci), ba;
        if constexpr (BWD) ba = part ? pauli_ld(b, 0, namps) : ldc(bc + ci);
        prot_self<BWD, GRAD>(T, ci, fa, ba, acc);
        if (part) {
          pauli_st(f, 0, namps, fa);
          if constexpr (BWD) pauli_st(b, 0, namps, ba);
        } else {
          stc(fc + ci, fa);
          if constexpr (BWD) stc(bc + ci, ba);
        }
      }
    }
  }
  if constexpr (GRAD) {
    cx a1[1] = {acc};
    block_reduce_store<1>(a1, partials + (uint64_t)blockIdx.x * RED);
  }
}

// ---- host ----------------------------------------------------------------------------------
// The constants of one rotation.  reverse: (mf, mf2) uncompute, (mb, mb2) pull back.  n <= 40.
inline const char* prot_make(unsigned long long x, unsigned long long z, double theta, size_t n,
                             bool reverse, prot& T) {
  if (((x | z) >> n) != 0) return fail("pos is out of the bound.");
  if (!std::isfinite(theta)) return fail("Pauli coefficients must be finite.");
  T = prot{};
  T.x = x;
  T.z = z;
  const uint64_t xc = (uint64_t)x >> LV;
  while (((xc >> T.hbc) >> 1) != 0) ++T.hbc;
  const int ny = __builtin_popcountll(x & z);
  T.nyp = (uint32_t)ny & 1u;
  const double c = std::cos(0.5 * theta), s = std::sin(0.5 * theta);
  // m = -i s i^nY
  const double mr[4] = {0, s, 0, -s}, mi[4] = {-s, 0, s, 0};
  const double sg = T.nyp ? -1.0 : 1.0, rv = reverse ? -1.0 : 1.0;
  const double m[2] = {mr[ny & 3], mi[ny & 3]};
  T.c = (real)c;
  T.mf = {(real)(rv * m[0]), (real)(rv * m[1])};
  T.mf2 = {(real)(rv * sg * m[0]), (real)(rv * sg * m[1])};
  T.mb = {(real)(sg * m[0]), (real)(sg * m[1])};
  T.mb2 = {(real)m[0], (real)m[1]};
  return nullptr;
}

// chunks of a state (a state below one chunk: one) and the blocks of a launch over its items
inline uint64_t prot_chunks(uint32_t n) { return std::max<uint64_t>(1, nchunks_of(n)); }
inline uint32_t prot_grid(const prot& T, uint32_t n, uint32_t cap) {
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  const uint64_t items = (T.x >> LV) != 0 ? prot_chunks(n) / 2 : prot_chunks(n);
  return pauli_grid((items + SPAN - 1) / SPAN, cap);
}

template <bool BWD, bool GRAD>
inline const char* prot_launch(Ctx& c, const char* name, double bytes, cx* f, cx* b, const prot& T,
                               uint32_t n, uint32_t grid, cx* out) {
  const uint64_t nch = prot_chunks(n);
  if ((T.x >> LV) != 0)
    return c.launch_block(name, bytes, k_prot_pair<BWD, GRAD>, grid, 256u, f, b, T, nch / 2, out);
  return c.launch_block(name, bytes, k_prot_self<BWD, GRAD>, grid, 256u, f, b, T, nch,
                        (uint32_t)std::min<uint64_t>((uint64_t)1 << n, VEC), out);
}

// s <- R(theta; P) s
inline const char* pauli_rot(Ctx& c, cx* s, const prot& T, uint32_t n) {
  return prot_launch<false, false>(c, "pauli_rot", 2.0 * state_bytes(n), s, nullptr, T, n,
                                   prot_grid(T, n, 1u << 20), nullptr);
}

// f <- R(-theta) f; *dtheta += dL/dtheta (dtheta != nullptr: one stream synchronisation);
// b <- R(theta)^T b (b != nullptr).  T from prot_make(reverse = true).
inline const char* pauli_rot_reverse(Ctx& c, cx* f, cx* b, const prot& T, uint32_t n,
                                     double* dtheta) {
  const char* name = "pauli_rot_rev";
  const uint32_t stream_grid = prot_grid(T, n, 1u << 20);
  if (!b)
    return prot_launch<false, false>(c, name, 2.0 * state_bytes(n), f, nullptr, T, n, stream_grid,
                                     nullptr);
  const double bytes = 4.0 * state_bytes(n);
  if (!dtheta) return prot_launch<true, false>(c, name, bytes, f, b, T, n, stream_grid, nullptr);
  const uint32_t grid = prot_grid(T, n, c.k.red_cap);
  QDC_TRY(reduce_into(c, c.results, 0, 0, grid, [&](cx* out) {
    return prot_launch<true, true>(c, name, bytes, f, b, T, n, grid, out);
  }));
  QDC_TRY(c.flush());
  QDC_HIP(hipMemcpyAsync(c.host_results, c.results, sizeof(cx) * RED, hipMemcpyDeviceToHost,
                         c.stream));
  QDC_HIP(hipStreamSynchronize(c.stream));
  // 1/2 Im(i^nY S)
  const double sr = (double)c.host_results[0].x, si = (double)c.host_results[0].y;
  const double im[4] = {si, sr, -si, -sr};
  *dtheta += 0.5 * im[__builtin_popcountll(T.x & T.z) & 3];
  return nullptr;
}

}  // namespace qdc

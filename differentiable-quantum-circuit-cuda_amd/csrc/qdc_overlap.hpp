// qdc_overlap.hpp — overlaps and transition elements between two states (include/qdc/overlap.h):
// o = <a|H|b> = sum_i conj(a[i]) (H b)[i] for H = sum_t c_t P_t (real c_t; the plain overlap <a|b>
// is H = I), and the cotangent injection of a real loss L(o) of o = <t|H|psi>.
//
// Cotangent.  The project's convention is dL/dtheta = Re sum_i bwd[i] (dpsi/dtheta)[i]
// (qdc_pauli_rot_reverse; qdc_pauli_inject's 2 w conj(H psi) is an instance).  With the target t a
// constant and g = dL/dRe o + i dL/dIm o, o = sum_j conj((H t)[j]) psi[j] is holomorphic in psi, so
// dL = Re(conj(g) do) = Re sum_j conj(g (H t)[j]) dpsi[j]:
//     bwd (+)= conj(g * (H t)).
// F = |o|^2 gives g = 2 o; E = <psi|H|psi> with the bra frozen at a copy of psi gives g = 2 w, the
// injection 2 w conj(H psi) of qdc_pauli_inject.
//
// Terms, groups, the host plan, the tables and the grids are those of qdc_pauli.hpp (pauli_plan,
// ptab, pauli_geo, pauli_grid: QDC_PAULI_GRID caps these kernels too); its one-state kernels are
// not touched.  With (H b)[i] = b[j] (wr - i wi), j = i ^ x, per group:
//
//   k_overlap: a streaming dot, OV_U chunks of each state in flight per thread, sum conj(a) b.
//     No LDS tile (H = I pays for none); a state below one chunk by the pauli_ld rule.
//   k_pauli_ov_window<OV_READ>: one pass for ALL window groups.  The block stages b's tile in LDS
//     as k_pauli_window stages f's, keeps a's own chunks in registers, takes the partner
//     p = b[l ^ x] from LDS and adds (wr - i wi) q, q = conj(a[i]) p, as a complex sum.
//   k_pauli_ov_far<OV_READ>: one pass per far group over the pairs (i, j = i ^ x): a[i], a[j], b[i],
//     b[j] are read once and the pair adds
//         conj(a[i]) b[j] (wr - i wi) + conj(a[j]) b[i] (wr + i wi)
//     (the signs are taken at j; at the other end every nY-odd term flips: the bookkeeping of
//     k_pauli_far's injection branch).  The "2 Re" pair identity of the energy kernel does not
//     apply: with a != b the two ends of a pair are not conjugates of each other.
//   <OV_STORE> / <OV_ACC>: the injection bwd (+)= conj(g) conj(h), h = H src as the one-state INJ
//     forms compute it, with the complex weight g in the kernel arguments; k_overlap_inj is the
//     H = I case, one streaming axpy-conj.  OV_STORE writes every amplitude without reading bwd;
//     the first launch of a storing call covers the whole state (the window pass, else the first
//     far pass, whose pairs partition the state), as in pauli_inject.
//
// Reductions as in qdc_pauli.hpp: block_reduce_store<1> with both parts used, the context's
// reduction slots, k_finalize, a host sum in launch order, one stream synchronisation per FIN_MAX
// launches.  No atomics: the same call returns the same bits.
#pragma once

#include "qdc_pauli.hpp"

namespace qdc {

constexpr int OV_U = 4;  // chunks of each state in flight per thread (k_overlap, k_overlap_inj)
enum OvMode { OV_READ = 0, OV_STORE = 1, OV_ACC = 2 };

// conj(g h)
__device__ __forceinline__ cx ov_conj_mul(cx g, cx h) {
  return {g.x * h.x - g.y * h.y, -(g.x * h.y + g.y * h.x)};
}

// chunk c of a state of nch chunks (namps < VEC: its one partial chunk, by the pauli_ld rule);
// zeros past the end
__device__ __forceinline__ chunk ov_ld(const cx* p, uint64_t c, uint64_t nch, uint32_t namps) {
  if (namps < (uint32_t)VEC) return pauli_ld(p, c < nch ? 0u : 1u, namps);
  chunk r = ldc(reinterpret_cast<const chunk*>(p) + (c < nch ? c : 0));
  if (c >= nch) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) r.v[v] = {0, 0};
  }
  return r;
}
// (c < nch)
__device__ __forceinline__ void ov_st(cx* p, uint64_t c, uint32_t namps, const chunk& r) {
  if (namps < (uint32_t)VEC)
    pauli_st(p, 0u, namps, r);
  else
    stc(reinterpret_cast<chunk*>(p) + c, r);
}

// partials[block] = the block's share of sum conj(a) b.  Blocks stride over spans of 256 * OV_U
// chunks; namps = min(2^n, 2^32 - 1) only tells a state below one chunk.  (a == b is allowed:
// neither is written.)
__global__ __launch_bounds__(256) void k_overlap(const cx* a, const cx* b, uint64_t nch,
                                                 uint32_t namps, cx* __restrict__ partials) {
  constexpr uint64_t SPAN = 256u * OV_U;
  cx acc[1] = {{0, 0}};
  for (uint64_t s = (uint64_t)blockIdx.x * SPAN; s < nch; s += (uint64_t)gridDim.x * SPAN) {
    chunk ra[OV_U], rb[OV_U];
#pragma unroll
    for (int u = 0; u < OV_U; ++u) {
      const uint64_t c = s + 256u * u + threadIdx.x;
      ra[u] = ov_ld(a, c, nch, namps);
      rb[u] = ov_ld(b, c, nch, namps);
    }
#pragma unroll
    for (int u = 0; u < OV_U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[0] = cfma_conj(rb[u].v[v], ra[u].v[v], acc[0]);
  }
  block_reduce_store<1>(acc, partials + (uint64_t)blockIdx.x * RED);
}

// b (+)= conj(g s): the H = I injection
template <bool ACC>
__global__ __launch_bounds__(256) void k_overlap_inj(const cx* __restrict__ s, cx* __restrict__ b,
                                                     uint64_t nch, uint32_t namps, cx g) {
  constexpr uint64_t SPAN = 256u * OV_U;
  for (uint64_t s0 = (uint64_t)blockIdx.x * SPAN; s0 < nch; s0 += (uint64_t)gridDim.x * SPAN) {
    chunk rs[OV_U], rb[OV_U];
#pragma unroll
    for (int u = 0; u < OV_U; ++u) {
      const uint64_t c = s0 + 256u * u + threadIdx.x;
      rs[u] = ov_ld(s, c, nch, namps);
      if constexpr (ACC) rb[u] = ov_ld(b, c, nch, namps);
    }
#pragma unroll
    for (int u = 0; u < OV_U; ++u) {
      const uint64_t c = s0 + 256u * u + threadIdx.x;
      chunk o;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const cx y = ov_conj_mul(g, rs[u].v[v]);
        o.v[v] = ACC ? cadd(rb[u].v[v], y) : y;
      }
      if (c < nch) ov_st(b, c, namps, o);
    }
  }
}

// chunk c of the tile of tamps amplitudes at p: whole tiles load plain chunks
__device__ __forceinline__ chunk ov_tile_ld(const cx* p, uint32_t c, uint32_t tamps) {
  if (tamps == (1u << PAULI_W)) return ldc(reinterpret_cast<const chunk*>(p) + c);
  return pauli_ld(p, c, tamps);
}

// The signed weights of one window group at the partners jl (amplitudes of the tile at `base`):
// wr over the table entries [e, mid) (nY even), wi over [mid, end) (nY odd); e advances to end.
__device__ __forceinline__ void ov_window_weights(const ptab& T, uint32_t& e, uint32_t mid,
                                                  uint32_t end, uint64_t base, uint32_t lmask,
                                                  const uint32_t (&jl)[PAULI_KC][VEC],
                                                  real (&wr)[PAULI_KC][VEC],
                                                  real (&wi)[PAULI_KC][VEC]) {
  for (; e < mid; ++e) {
    const uint64_t z = T.e[e].z;
    const real c = T.e[e].c;
    const uint32_t hp = (uint32_t)__popcll(base & z), zl = (uint32_t)z & lmask;
#pragma unroll
    for (int k = 0; k < PAULI_KC; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) wr[k][v] += pauli_sgn(__popc(jl[k][v] & zl) + hp, c);
  }
  for (; e < end; ++e) {
    const uint64_t z = T.e[e].z;
    const real c = T.e[e].c;
    const uint32_t hp = (uint32_t)__popcll(base & z), zl = (uint32_t)z & lmask;
#pragma unroll
    for (int k = 0; k < PAULI_KC; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) wi[k][v] += pauli_sgn(__popc(jl[k][v] & zl) + hp, c);
  }
}

// All window groups of T in one pass; wn = min(W, n), blocks stride over the tiles (k_pauli_window's
// geometry).  OV_READ: partials[block] = the block's share of <a|H_window|s>, s staged in LDS, a in
// registers.  OV_STORE / OV_ACC: b (+)= conj(g (H_window s)); a is not used.
template <int MODE>
__global__ __launch_bounds__(256) void k_pauli_ov_window(const cx* a, const cx* __restrict__ s,
                                                         cx* __restrict__ b, ptab T, uint32_t wn,
                                                         uint64_t ntiles, cx g,
                                                         cx* __restrict__ partials) {
  constexpr bool READ = MODE == OV_READ;
  __shared__ chunk lds[PAULI_TC];
  const uint32_t t = threadIdx.x;
  const uint32_t tamps = 1u << wn, lmask = tamps - 1u;
  cx osum = {0, 0};
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = tile << wn;
    cx own[PAULI_KC][VEC];  // a's amplitudes (OV_READ)
    {
      chunk rs[PAULI_KC], ra[PAULI_KC];  // every load in flight before the first use
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k) {
        rs[k] = ov_tile_ld(s + base, t + 256u * k, tamps);
        if constexpr (READ) ra[k] = ov_tile_ld(a + base, t + 256u * k, tamps);
      }
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k) {
        lds[t + 256u * k] = rs[k];
        if constexpr (READ) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) own[k][v] = ra[k].v[v];
        }
      }
    }
    __syncthreads();
    cx h[PAULI_KC][VEC];  // H s (injection)
#pragma unroll
    for (int k = 0; k < PAULI_KC; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) h[k][v] = {0, 0};
    uint32_t e = 0;
    for (uint32_t gi = 0; gi < T.ng; ++gi) {
      const uint32_t x = T.gx[gi], mid = T.gme[gi] & 0xffffu, end = T.gme[gi] >> 16;
      cx pj[PAULI_KC][VEC];
      uint32_t jl[PAULI_KC][VEC];
      real wr[PAULI_KC][VEC], wi[PAULI_KC][VEC];
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          // (partner < 2^wn: x < 2^wn; amplitudes past a small state hold zeros)
          jl[k][v] = ((t + 256u * k) * VEC + v) ^ x;
          pj[k][v] = reinterpret_cast<const cx*>(lds)[jl[k][v]];
          wr[k][v] = 0;
          wi[k][v] = 0;
        }
      ov_window_weights(T, e, mid, end, base, lmask, jl, wr, wi);
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const cx p = pj[k][v];
          if constexpr (READ) {  // (wr - i wi) q, q = conj(a[i]) p
            const cx o = own[k][v];
            const real qr = o.x * p.x + o.y * p.y, qi = o.x * p.y - o.y * p.x;
            osum.x += wr[k][v] * qr + wi[k][v] * qi;
            osum.y += wr[k][v] * qi - wi[k][v] * qr;
          } else {  // s[j] (wr - i wi)
            h[k][v].x += p.x * wr[k][v] + p.y * wi[k][v];
            h[k][v].y += p.y * wr[k][v] - p.x * wi[k][v];
          }
        }
    }
    if constexpr (!READ) {
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k) {
        const uint32_t c = t + 256u * k;
        chunk o;
        if constexpr (MODE == OV_ACC) o = pauli_ld(b + base, c, tamps);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const cx y = ov_conj_mul(g, h[k][v]);
          o.v[v] = MODE == OV_ACC ? cadd(o.v[v], y) : y;
        }
        pauli_st(b + base, c, tamps, o);
      }
    }
    __syncthreads();  // the next tile overwrites the staged one
  }
  if constexpr (READ) {
    cx acc[1] = {osum};
    block_reduce_store<1>(acc, partials + (uint64_t)blockIdx.x * RED);
  }
}

// One far group (k_pauli_far's table and geometry: pair p of npairs = 2^(n-1) is i = p with a zero
// inserted at bit hb, j = i ^ x; blocks stride over spans of 256 * PAULI_FU pairs).
template <int MODE>
__global__ __launch_bounds__(256) void k_pauli_ov_far(const cx* a, const cx* __restrict__ s,
                                                      cx* __restrict__ b, ptab T, uint32_t hb,
                                                      uint64_t npairs, cx g,
                                                      cx* __restrict__ partials) {
  constexpr bool READ = MODE == OV_READ;
  const uint64_t x = T.x64;
  const uint32_t mid = T.gme[0] & 0xffffu, end = T.gme[0] >> 16;
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  cx osum = {0, 0};
  for (uint64_t sp = (uint64_t)blockIdx.x * SPAN; sp < npairs; sp += (uint64_t)gridDim.x * SPAN) {
    uint64_t i[PAULI_FU], j[PAULI_FU];
    bool ok[PAULI_FU];
    cx si[PAULI_FU], sj[PAULI_FU], ai[PAULI_FU], aj[PAULI_FU];
    real wr[PAULI_FU], wi[PAULI_FU];
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) {
      const uint64_t pi = sp + 256u * u + threadIdx.x;
      ok[u] = pi < npairs;
      i[u] = insert_zero(ok[u] ? pi : 0, hb);
      j[u] = i[u] ^ x;
      si[u] = s[i[u]];
      sj[u] = s[j[u]];
      if constexpr (READ) {
        ai[u] = a[i[u]];
        aj[u] = a[j[u]];
      }
      if (!ok[u]) si[u] = sj[u] = ai[u] = aj[u] = {0, 0};
      wr[u] = 0;
      wi[u] = 0;
    }
    uint32_t e = 0;
    for (; e < mid; ++e) {
      const uint64_t z = T.e[e].z;
      const real c = T.e[e].c;
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) wr[u] += pauli_sgn((uint32_t)__popcll(j[u] & z), c);
    }
    for (; e < end; ++e) {
      const uint64_t z = T.e[e].z;
      const real c = T.e[e].c;
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u) wi[u] += pauli_sgn((uint32_t)__popcll(j[u] & z), c);
    }
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) {
      if constexpr (READ) {
        // q1 = conj(a[i]) s[j] takes (wr - i wi), q2 = conj(a[j]) s[i] takes (wr + i wi)
        const real q1r = ai[u].x * sj[u].x + ai[u].y * sj[u].y;
        const real q1i = ai[u].x * sj[u].y - ai[u].y * sj[u].x;
        const real q2r = aj[u].x * si[u].x + aj[u].y * si[u].y;
        const real q2i = aj[u].x * si[u].y - aj[u].y * si[u].x;
        osum.x += wr[u] * (q1r + q2r) + wi[u] * (q1i - q2i);
        osum.y += wr[u] * (q1i + q2i) - wi[u] * (q1r - q2r);
      } else {
        // (H s)[i] = s[j] (wr - i wi), (H s)[j] = s[i] (wr + i wi)
        const cx hi = {sj[u].x * wr[u] + sj[u].y * wi[u], sj[u].y * wr[u] - sj[u].x * wi[u]};
        const cx hj = {si[u].x * wr[u] - si[u].y * wi[u], si[u].y * wr[u] + si[u].x * wi[u]};
        cx yi = ov_conj_mul(g, hi), yj = ov_conj_mul(g, hj);
        if (ok[u]) {
          if constexpr (MODE == OV_ACC) {
            yi = cadd(b[i[u]], yi);
            yj = cadd(b[j[u]], yj);
          }
          b[i[u]] = yi;
          b[j[u]] = yj;
        }
      }
    }
  }
  if constexpr (READ) {
    cx acc[1] = {osum};
    block_reduce_store<1>(acc, partials + (uint64_t)blockIdx.x * RED);
  }
}

// ---- host ------------------------------------------------------------------------------------
struct OvGeo {
  uint64_t nch, spans;  // chunks of a state (one below a chunk), spans of 256 * OV_U chunks
  uint32_t namps;       // min(2^n, 2^32 - 1)
};
inline OvGeo ov_geo(uint32_t n) {
  OvGeo g{};
  const uint64_t amps = (uint64_t)1 << n;
  g.nch = std::max<uint64_t>(1, amps / VEC);
  g.spans = (g.nch + 256u * OV_U - 1) / (256u * OV_U);
  g.namps = (uint32_t)std::min<uint64_t>(amps, 0xffffffffu);
  return g;
}

// the first `count` slots of the results buffer, added to (re, im) in slot order: one stream
// synchronisation
inline const char* ov_collect(Ctx& c, size_t count, double& re, double& im) {
  QDC_TRY(c.flush());
  QDC_HIP(hipMemcpyAsync(c.host_results, c.results, sizeof(cx) * RED * count,
                         hipMemcpyDeviceToHost, c.stream));
  QDC_HIP(hipStreamSynchronize(c.stream));
  for (size_t l = 0; l < count; ++l) {
    re += (double)c.host_results[l * RED].x;
    im += (double)c.host_results[l * RED].y;
  }
  return nullptr;
}

// out += <a|b>
inline const char* overlap(Ctx& c, const cx* a, const cx* b, uint32_t n, double* out) {
  const OvGeo g = ov_geo(n);
  const uint32_t grid = pauli_grid(g.spans, c.k.red_cap);
  QDC_TRY(reduce_into(c, c.results, 0, 0, grid, [&](cx* part) {
    return c.launch_block("overlap", 2.0 * state_bytes(n), k_overlap, grid, 256u, a, b, g.nch,
                          g.namps, part);
  }));
  double re = 0, im = 0;
  QDC_TRY(ov_collect(c, 1, re, im));
  out[0] += re;
  out[1] += im;
  return nullptr;
}

// out += <a|H|b>: pauli_energy's launch loop on the two-state kernels
inline const char* pauli_overlap(Ctx& c, const cx* a, const cx* b, const PauliPlan& P, uint32_t n,
                                 double* out) {
  const PauliGeo g = pauli_geo(n);
  const size_t nl = P.launches();
  const cx g0 = {0, 0};
  double re = 0, im = 0;
  for (size_t l0 = 0; l0 < nl; l0 += FIN_MAX) {
    const size_t l1 = std::min<size_t>(nl, l0 + FIN_MAX);
    for (size_t l = l0; l < l1; ++l) {
      const bool window = l < P.win.size();
      const ptab& T = window ? P.win[l] : P.far[l - P.win.size()];
      const uint32_t grid = pauli_grid(window ? g.ntiles : g.spans, c.k.red_cap);
      QDC_TRY(reduce_into(c, c.results, (uint32_t)(l - l0), 0, grid, [&](cx* part) {
        if (window)
          return c.launch_block("pauli_overlap_window", 2.0 * state_bytes(n),
                                k_pauli_ov_window<OV_READ>, grid, 256u, a, b, (cx*)nullptr, T,
                                g.wn, g.ntiles, g0, part);
        return c.launch_block("pauli_overlap_far", 2.0 * state_bytes(n), k_pauli_ov_far<OV_READ>,
                              grid, 256u, a, b, (cx*)nullptr, T, P.far_hb[l - P.win.size()],
                              g.npairs, g0, part);
      }));
    }
    QDC_TRY(ov_collect(c, l1 - l0, re, im));
  }
  out[0] += re;
  out[1] += im;
  return nullptr;
}

// bwd (+)= conj(g src)
inline const char* overlap_inject(Ctx& c, const cx* src, cx* bwd, uint32_t n, double g_re,
                                  double g_im, bool accumulate) {
  const OvGeo g = ov_geo(n);
  const cx gw = {(real)g_re, (real)g_im};
  const uint32_t grid = pauli_grid(g.spans, 1u << 20);
  const double bytes = (accumulate ? 3.0 : 2.0) * state_bytes(n);
  return accumulate ? c.launch_block("overlap_inj", bytes, k_overlap_inj<true>, grid, 256u, src,
                                     bwd, g.nch, g.namps, gw)
                    : c.launch_block("overlap_inj", bytes, k_overlap_inj<false>, grid, 256u, src,
                                     bwd, g.nch, g.namps, gw);
}

// bwd (+)= conj(g H src): pauli_inject's launch loop with the complex weight
inline const char* pauli_overlap_inject(Ctx& c, const cx* src, cx* bwd, const PauliPlan& P,
                                        uint32_t n, double g_re, double g_im, bool accumulate) {
  const PauliGeo g = pauli_geo(n);
  const cx gw = {(real)g_re, (real)g_im};
  const cx* none = nullptr;
  bool acc = accumulate;
  for (size_t l = 0; l < P.launches(); ++l) {
    const bool window = l < P.win.size();
    const ptab& T = window ? P.win[l] : P.far[l - P.win.size()];
    const double bytes = (acc ? 3.0 : 2.0) * state_bytes(n);
    if (window) {
      const uint32_t grid = pauli_grid(g.ntiles, 1u << 20);
      QDC_TRY(c.launch_block("pauli_overlap_window_inj", bytes,
                             acc ? k_pauli_ov_window<OV_ACC> : k_pauli_ov_window<OV_STORE>, grid,
                             256u, none, src, bwd, T, g.wn, g.ntiles, gw, (cx*)nullptr));
    } else {
      const uint32_t grid = pauli_grid(g.spans, 1u << 20);
      QDC_TRY(c.launch_block("pauli_overlap_far_inj", bytes,
                             acc ? k_pauli_ov_far<OV_ACC> : k_pauli_ov_far<OV_STORE>, grid, 256u,
                             none, src, bwd, T, P.far_hb[l - P.win.size()], g.npairs, gw,
                             (cx*)nullptr));
    }
    acc = true;
  }
  return nullptr;
}

}  // namespace qdc

// qdc_pauli.hpp — Pauli-sum observables (include/qdc/pauli.h): the energy E = <psi|H|psi> of
// H = sum_t c_t P_t and its cotangent injection bwd (+)= 2 w conj(H psi), in a few passes.
//
// A term is (c, x, z): (P psi)[i] = i^nY (-1)^popcount(j & z) psi[j], j = i ^ x, nY =
// popcount(x & z).  Every term with the same x pairs the same amplitudes (i, i ^ x); the terms
// of such a group differ only in a sign s = (-1)^popcount(j & z) and a phase i^nY.  With
// q = conj(psi[i]) psi[j] a group contributes to amplitude i
//     Re(conj(psi[i]) (H psi)[i]) = wr Re q + wi Im q,     (H psi)[i] = psi[j] (wr - i wi)
//     wr = sum over its terms with nY even of c' s,   wi = the same over nY odd,
//     c' = c * (+1, -1, -1, +1)[nY mod 4]   (Re(i^nY q) = Re q, -Im q, -Re q, Im q)
// so a group costs one pairing and, per term, one popcount and one signed add.
//
// Host plan (pauli_plan, plain C++): terms with equal (x, z) merge; groups by x; a group is a
// WINDOW group when x < 2^min(W, n) — its partners lie inside an aligned tile of 2^W amplitudes
// — and a FAR group otherwise.  A launch reads its terms from a table in the kernel arguments
// (every lane reads the same entry: scalar loads), PAULI_CAP entries at most; larger groups are
// split over launches.  Within a group the nY-even entries come first.
//
//   k_pauli_window: one pass over the state for ALL window groups.  A block stages a tile of
//     2^W amplitudes in LDS (16 KiB: W = 11 in f32, 10 in f64 — the two-state tile of the fused
//     passes, ten blocks' worth of LDS per CU so the wave slots, not LDS, bound occupancy), keeps
//     its own 4 chunks per thread in registers and takes partners from LDS at amplitude l ^ x.
//     The high part of a sign, popcount(tile base & z), is block-uniform.
//   k_pauli_far: one pass per far group over the pairs (i, i ^ x), i with the highest set bit of
//     x clear.  Both ends of a pair are handled together (2 (wr Re q + wi Im q), the pair
//     identity of the issue): each amplitude is read once, and consecutive i have consecutive
//     partners inside runs of 2^(lowest set bit of x), whole cache lines either way.
//
// Injection forms (INJ) read fwd and write bwd: ACC = false stores without reading bwd.  The
// window form writes the sum over all window groups once; a far form with ACC = false also
// covers every amplitude (the pairs partition the state), so a call without window groups
// starts with it.
//
// Reductions: lanes, then waves (block_reduce_store), block partials in the context's reduction
// slots, k_finalize, the results buffer and a host sum in launch order.  No atomics: the same
// call returns the same bits.
#pragma once

#include <cmath>
#include <map>

#include "qdc_device.hpp"

namespace qdc {

constexpr uint32_t PAULI_W = sizeof(real) == 4 ? 11u : 10u;  // tile: 16 KiB of amplitudes
constexpr uint32_t PAULI_TC = (1u << PAULI_W) / VEC;         // chunks of a tile (1024)
constexpr int PAULI_KC = (int)(PAULI_TC / 256u);             // chunks per thread and tile
constexpr uint32_t PAULI_CAP = 128;                          // table entries of one launch
constexpr int PAULI_FU = 4;                                  // pairs per thread and far span
static_assert(PAULI_KC * 256 == (int)PAULI_TC, "a tile is whole chunks of the block");

struct pent {
  uint64_t z;
  real c;  // c' (the phase's sign folded in)
};
struct ptab {
  uint64_t x64;              // far launch: its group's x
  uint32_t ng;               // groups (window) / 1 (far)
  uint32_t gx[PAULI_CAP];    // window launch: x of group g
  // mid | end << 16: entries [end of g-1, mid) have nY even, [mid, end) nY odd
  uint32_t gme[PAULI_CAP];
  pent e[PAULI_CAP];
};
static_assert(sizeof(ptab) <= 3584, "the table travels in the kernel arguments (4 KiB)");

// -c where the parity is odd: bit 0 of the count moves into the sign bit
__device__ __forceinline__ real pauli_sgn(uint32_t parity, real c) {
#ifdef QDC_F64
  return __hiloint2double(__double2hiint(c) ^ (int)(parity << 31), __double2loint(c));
#else
  return __uint_as_float(__float_as_uint(c) ^ (parity << 31));
#endif
}

// chunk c of a tile of `tamps` amplitudes at p (a state below one chunk: its amplitudes, the
// rest zero)
__device__ __forceinline__ chunk pauli_ld(const cx* p, uint32_t c, uint32_t tamps) {
  if ((c + 1) * VEC <= tamps) return ldc(reinterpret_cast<const chunk*>(p) + c);
  chunk r;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const bool in = c * VEC + v < tamps;
    const cx a = p[in ? c * VEC + v : 0];
    r.v[v] = in ? a : cx{0, 0};
  }
  return r;
}
__device__ __forceinline__ void pauli_st(cx* p, uint32_t c, uint32_t tamps, const chunk& r) {
  if ((c + 1) * VEC <= tamps) {
    stc(reinterpret_cast<chunk*>(p) + c, r);
  } else {
#pragma unroll
    for (int v = 0; v < VEC; ++v)
      if (c * VEC + v < tamps) p[c * VEC + v] = r.v[v];
  }
}

// wn = min(W, n): a tile is 2^wn amplitudes (one tile when n < W).  Blocks stride over the
// tiles.  Energy: partials[block] = {sum, 0}.  Injection: b (+)= w2 conj(H f), w2 = 2 w.
template <bool INJ, bool ACC>
__global__ __launch_bounds__(256) void k_pauli_window(const cx* __restrict__ f,
                                                      cx* __restrict__ b, ptab T, uint32_t wn,
                                                      uint64_t ntiles, real w2,
                                                      cx* __restrict__ partials) {
  __shared__ chunk lds[PAULI_TC];
  const uint32_t t = threadIdx.x;
  const uint32_t tamps = 1u << wn, lmask = tamps - 1u;
  real esum = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t base = tile << wn;
    cx own[PAULI_KC][VEC];
    if (wn == PAULI_W) {  // whole tiles (n >= W): four independent loads in flight
      chunk raw[PAULI_KC];
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k)
        raw[k] = ldc(reinterpret_cast<const chunk*>(f + base) + t + 256u * k);
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k) {
        lds[t + 256u * k] = raw[k];
#pragma unroll
        for (int v = 0; v < VEC; ++v) own[k][v] = raw[k].v[v];
      }
    } else {
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k) {
        const chunk r = pauli_ld(f + base, t + 256u * k, tamps);
        lds[t + 256u * k] = r;
#pragma unroll
        for (int v = 0; v < VEC; ++v) own[k][v] = r.v[v];
      }
    }
    __syncthreads();
    cx h[PAULI_KC][VEC];
#pragma unroll
    for (int k = 0; k < PAULI_KC; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) h[k][v] = {0, 0};
    uint32_t e = 0;
    for (uint32_t g = 0; g < T.ng; ++g) {
      const uint32_t x = T.gx[g], mid = T.gme[g] & 0xffffu, end = T.gme[g] >> 16;
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
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const cx a = own[k][v], p = pj[k][v];
          if constexpr (INJ) {  // psi[j] (wr - i wi)
            h[k][v].x += p.x * wr[k][v] + p.y * wi[k][v];
            h[k][v].y += p.y * wr[k][v] - p.x * wi[k][v];
          } else {
            const real qr = a.x * p.x + a.y * p.y, qi = a.x * p.y - a.y * p.x;
            esum += wr[k][v] * qr + wi[k][v] * qi;
          }
        }
    }
    if constexpr (INJ) {
#pragma unroll
      for (int k = 0; k < PAULI_KC; ++k) {
        const uint32_t c = t + 256u * k;
        chunk o;
        if constexpr (ACC) o = pauli_ld(b + base, c, tamps);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const cx y = {w2 * h[k][v].x, -w2 * h[k][v].y};
          o.v[v] = ACC ? cadd(o.v[v], y) : y;
        }
        pauli_st(b + base, c, tamps, o);
      }
    }
    __syncthreads();  // the next tile overwrites the staged one
  }
  if constexpr (!INJ) {
    cx acc[1] = {{esum, 0}};
    block_reduce_store<1>(acc, partials + (uint64_t)blockIdx.x * RED);
  }
}

// One far group (T.x64, entries [0, mid) nY even, [mid, end) nY odd): pair p of
// npairs = 2^(n-1) is i = p with a zero inserted at bit hb (the highest set bit of x), j = i ^ x.
// Blocks stride over spans of 256 * PAULI_FU pairs.
template <bool INJ, bool ACC>
__global__ __launch_bounds__(256) void k_pauli_far(const cx* __restrict__ f, cx* __restrict__ b,
                                                   ptab T, uint32_t hb, uint64_t npairs, real w2,
                                                   cx* __restrict__ partials) {
  const uint64_t x = T.x64;
  const uint32_t mid = T.gme[0] & 0xffffu, end = T.gme[0] >> 16;
  constexpr uint64_t SPAN = 256u * PAULI_FU;
  real esum = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * SPAN; s < npairs; s += (uint64_t)gridDim.x * SPAN) {
    uint64_t i[PAULI_FU], j[PAULI_FU];
    bool ok[PAULI_FU];
    cx a[PAULI_FU], p[PAULI_FU];
    real wr[PAULI_FU], wi[PAULI_FU];
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) {
      const uint64_t pi = s + 256u * u + threadIdx.x;
      ok[u] = pi < npairs;
      i[u] = insert_zero(ok[u] ? pi : 0, hb);
      j[u] = i[u] ^ x;
      a[u] = f[i[u]];
      p[u] = f[j[u]];
      if (!ok[u]) a[u] = p[u] = {0, 0};
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
      if constexpr (INJ) {
        // (H f)[i] = f[j] (wr - i wi), (H f)[j] = f[i] (wr + i wi); b (+)= w2 conj(H f)
        cx yi = {w2 * (p[u].x * wr[u] + p[u].y * wi[u]), w2 * (p[u].x * wi[u] - p[u].y * wr[u])};
        cx yj = {w2 * (a[u].x * wr[u] - a[u].y * wi[u]), -w2 * (a[u].x * wi[u] + a[u].y * wr[u])};
        if (ok[u]) {
          if constexpr (ACC) {
            yi = cadd(b[i[u]], yi);
            yj = cadd(b[j[u]], yj);
          }
          b[i[u]] = yi;
          b[j[u]] = yj;
        }
      } else {
        const real qr = a[u].x * p[u].x + a[u].y * p[u].y, qi = a[u].x * p[u].y - a[u].y * p[u].x;
        esum += 2 * (wr[u] * qr + wi[u] * qi);
      }
    }
  }
  if constexpr (!INJ) {
    cx acc[1] = {{esum, 0}};
    block_reduce_store<1>(acc, partials + (uint64_t)blockIdx.x * RED);
  }
}

// ---- host plan ---------------------------------------------------------------------------
struct PauliPlan {
  size_t merged = 0;
  std::vector<uint64_t> win_x, far_x;  // the distinct x masks of each class, ascending
  std::vector<ptab> win, far;          // launches: the window tables, then one per far chunk
  std::vector<uint32_t> far_hb;        // highest set bit of each far launch's x
  size_t launches() const { return win.size() + far.size(); }
};

// coeff == nullptr: the plan's shape only (zero coefficients).  n <= 40 (check_n).
inline const char* pauli_plan(const unsigned long long* xm, const unsigned long long* zm,
                              const double* coeff, size_t terms, size_t n, PauliPlan& P) {
  if (terms == 0) return fail("The observable has no terms.");
  if (!xm || !zm) return fail("The observable has no masks.");
  std::map<std::pair<uint64_t, uint64_t>, double> merged;  // ordered by x, then z
  for (size_t t = 0; t < terms; ++t) {
    if (((xm[t] | zm[t]) >> n) != 0) return fail("pos is out of the bound.");
    const double c = coeff ? coeff[t] : 0.0;
    if (!std::isfinite(c)) return fail("Pauli coefficients must be finite.");
    merged[{(uint64_t)xm[t], (uint64_t)zm[t]}] += c;
  }
  P = PauliPlan{};
  P.merged = merged.size();
  const uint32_t wn = (uint32_t)std::min<size_t>(PAULI_W, n);
  ptab cur{};
  uint32_t used = 0;
  auto flush = [&](std::vector<ptab>& to) {
    if (cur.ng == 0) return;
    to.push_back(cur);
    cur = ptab{};
    used = 0;
  };
  auto it = merged.begin();
  std::vector<ptab> win, far;
  while (it != merged.end()) {
    const uint64_t x = it->first.first;
    const bool window = x < ((uint64_t)1 << wn);
    // the group's entries: nY even first, each class ascending in z (the map's order)
    std::vector<pent> ent[2];
    for (; it != merged.end() && it->first.first == x; ++it) {
      const uint64_t z = it->first.second;
      const int ny = __builtin_popcountll(x & z);
      const double c = (ny & 3) == 1 || (ny & 3) == 2 ? -it->second : it->second;
      ent[ny & 1].push_back(pent{z, (real)c});
    }
    (window ? P.win_x : P.far_x).push_back(x);
    std::vector<ptab>& to = window ? win : far;
    if (!window) flush(win);  // (the map's order: every window group precedes the far ones)
    uint32_t hb = 0;
    while (((x >> hb) >> 1) != 0) ++hb;
    size_t at[2] = {0, 0};
    while (at[0] < ent[0].size() || at[1] < ent[1].size()) {
      if (used == PAULI_CAP) flush(to);
      const uint32_t g = cur.ng++;
      cur.x64 = x;
      cur.gx[g] = (uint32_t)x;  // (window groups: x < 2^11)
      for (int cls = 0; cls < 2; ++cls) {
        while (at[cls] < ent[cls].size() && used < PAULI_CAP) cur.e[used++] = ent[cls][at[cls]++];
        if (cls == 0) cur.gme[g] = used;
      }
      cur.gme[g] |= used << 16;
      if (!window) {  // a far launch is one chunk of one group
        P.far_hb.push_back(hb);
        flush(to);
      }
    }
  }
  flush(win);
  P.win = std::move(win);
  P.far = std::move(far);
  return nullptr;
}

// QDC_PAULI_GRID: a block-count override of both kernels (tests: the stride loops at a small n)
inline uint32_t pauli_grid(uint64_t units, uint32_t cap) {
  cap = (uint32_t)knob_long(Knob::PAULI_GRID, (long)cap, 1, (long)cap);
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(units, cap));
}

struct PauliGeo {
  uint32_t wn;
  uint64_t ntiles, npairs, spans;
};
inline PauliGeo pauli_geo(uint32_t n) {
  PauliGeo g{};
  g.wn = std::min(PAULI_W, n);
  g.ntiles = (uint64_t)1 << (n - g.wn);
  g.npairs = n > 0 ? (uint64_t)1 << (n - 1) : 0;
  g.spans = (g.npairs + 256u * PAULI_FU - 1) / (256u * PAULI_FU);
  return g;
}

// *energy += <s|H|s>.  The launches reduce into slots of the results buffer, FIN_MAX at a time;
// the host adds the slots in launch order (one stream synchronisation per FIN_MAX launches).
inline const char* pauli_energy(Ctx& c, const cx* s, const PauliPlan& P, uint32_t n,
                                double* energy) {
  const PauliGeo g = pauli_geo(n);
  const size_t nl = P.launches();
  double sum = 0;
  for (size_t l0 = 0; l0 < nl; l0 += FIN_MAX) {
    const size_t l1 = std::min<size_t>(nl, l0 + FIN_MAX);
    for (size_t l = l0; l < l1; ++l) {
      const bool window = l < P.win.size();
      const ptab& T = window ? P.win[l] : P.far[l - P.win.size()];
      const uint32_t grid = pauli_grid(window ? g.ntiles : g.spans, c.k.red_cap);
      QDC_TRY(reduce_into(c, c.results, (uint32_t)(l - l0), 0, grid, [&](cx* out) {
        if (window)
          return c.launch_block("pauli_window", state_bytes(n), k_pauli_window<false, false>, grid,
                                256u, s, (cx*)nullptr, T, g.wn, g.ntiles, (real)0, out);
        return c.launch_block("pauli_far", state_bytes(n), k_pauli_far<false, false>, grid, 256u,
                              s, (cx*)nullptr, T, P.far_hb[l - P.win.size()], g.npairs, (real)0,
                              out);
      }));
    }
    QDC_TRY(c.flush());
    QDC_HIP(hipMemcpyAsync(c.host_results, c.results, sizeof(cx) * RED * (l1 - l0),
                           hipMemcpyDeviceToHost, c.stream));
    QDC_HIP(hipStreamSynchronize(c.stream));
    for (size_t l = l0; l < l1; ++l) sum += (double)c.host_results[(l - l0) * RED].x;
  }
  *energy += sum;
  return nullptr;
}

// b (+)= 2 w conj(H f).  The first launch of a storing call covers every amplitude: the window
// pass, or, without window groups, the first far pass (its pairs partition the state).
inline const char* pauli_inject(Ctx& c, const cx* f, cx* b, const PauliPlan& P, uint32_t n,
                                double weight, bool accumulate) {
  const PauliGeo g = pauli_geo(n);
  const real w2 = (real)(2.0 * weight);
  bool acc = accumulate;
  for (size_t l = 0; l < P.launches(); ++l) {
    const bool window = l < P.win.size();
    const ptab& T = window ? P.win[l] : P.far[l - P.win.size()];
    const double bytes = (acc ? 3.0 : 2.0) * state_bytes(n);
    if (window) {
      const uint32_t grid = pauli_grid(g.ntiles, 1u << 20);
      QDC_TRY(acc ? c.launch_block("pauli_window_inj", bytes, k_pauli_window<true, true>, grid,
                                   256u, f, b, T, g.wn, g.ntiles, w2, (cx*)nullptr)
                  : c.launch_block("pauli_window_inj", bytes, k_pauli_window<true, false>, grid,
                                   256u, f, b, T, g.wn, g.ntiles, w2, (cx*)nullptr));
    } else {
      const uint32_t grid = pauli_grid(g.spans, 1u << 20);
      const uint32_t hb = P.far_hb[l - P.win.size()];
      QDC_TRY(acc ? c.launch_block("pauli_far_inj", bytes, k_pauli_far<true, true>, grid, 256u, f,
                                   b, T, hb, g.npairs, w2, (cx*)nullptr)
                  : c.launch_block("pauli_far_inj", bytes, k_pauli_far<true, false>, grid, 256u, f,
                                   b, T, hb, g.npairs, w2, (cx*)nullptr));
    }
    acc = true;
  }
  return nullptr;
}

}  // namespace qdc

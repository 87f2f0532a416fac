// qdc_qkgrad.hpp — gradient and reduced density matrix of a dense k-qubit gate (k = 3..5) on
// MFMA: the two reductions that complete qdc_qkgate (qdc_qk.hpp) to the triple every other gate
// kind has (q1gate / q1grad / get_q1density, q2gate / q2grad / get_q2density).
//
//   grad[r*C + c]    = sum over groups of bwd[r] * fwd[c]            (no conjugation, as q2grad)
//   density[r*C + c] = sum over groups of state[r] * conj(state[c])  (as get_q2density)
//
// with C = 2^k and a group the C amplitudes that differ only in the target bits (local index
// bit (k-1-b) = qubit pos[b]).  In real form a group is a vector of 2C components (component
// 2c + p = part p of amplitude c) and both results are one real matrix
//   P[i][j] = sum over groups of a_i * b_j        (2C x 2C, a = bwd or state, b = fwd or state)
// an outer-product accumulation whose K dimension is the 2^(n-k) groups: v_mfma_{f32,f64}_16x16x4
// with A = 16 components of a, B = 16 components of b, four groups per instruction and
// (2C/16)^2 = 1 / 4 / 16 accumulator tiles per wave at k = 3 / 4 / 5.  The complex result is
// formed from the four real quadrants once, in the finalize kernel:
//   grad    = (RR - II) + i (RI + IR),   density = (RR + II) + i (IR - RI)
// (RR = P[2r][2c], RI = P[2r][2c+1], IR = P[2r+1][2c], II = P[2r+1][2c+1]).  The density is the
// same contraction with both operands read from one staged copy of the state (S bytes of
// traffic); P is then symmetric, only the tiles on and above the diagonal are computed and the
// finalize kernel mirrors them.
//
// Memory: the tiles of k_qkl (qdc_qk.hpp: 16 whole groups, loaded with 16-B lane-contiguous
// accesses, XOR-swizzled in LDS).  Lane l = kk*16 + i of K step s reads components i + 16 t of
// group 4 s + kk: amplitude (i >> 1) + 8 t, part i & 1.  States with fewer than 16 groups
// (n - k < 4, where qkl_plan gives up) take one gathered, zero-filled tile on one wave.
//
// Reduction: no atomics.  The four waves of a block add their accumulators in LDS in wave order,
// the block writes its 2C x 2C partial to a scratch buffer, and k_qkg_fin sums the partials in a
// fixed order: two calls on the same inputs give the same bits.
#pragma once

#include "qdc_qk.hpp"

namespace qdc {

struct qkg_geo {
  qkl_geo l;  // staged tiles (n - k >= 4)
  qk_geo q;   // gathered tile (fewer than 16 groups)
};

constexpr uint32_t QKG_GRID_MAX = 1024;  // blocks = partials of one call

template <int K, int NB, bool DENS, bool GATHER>
__global__ __launch_bounds__(256) void k_qkg(const cx* __restrict__ f, const cx* __restrict__ b,
                                             real* __restrict__ parts, qkg_geo g) {
  constexpr int C = 1 << K, R2 = 2 * C, NT = R2 / 16;
  constexpr int TA = 16 * C;         // amplitudes per tile
  constexpr int NP = TA / VEC / 64;  // 16-B pieces per lane per tile and state
  constexpr int NS = DENS ? 1 : 2;   // states staged (0: fwd / the state, NS - 1: bwd)
  // K = 3 has one accumulator tile: two chains (even / odd K steps) keep the dependent
  // 16x16x4 latency off the issue rate; at K >= 4 the tiles are the independent chains
  constexpr int NCH = NT == 1 ? 2 : 1;
  static_assert(NP >= 1, "tile smaller than one wave access");
#ifdef QDC_F64
  using acc_t = double __attribute__((ext_vector_type(4)));
#else
  using acc_t = float __attribute__((ext_vector_type(4)));
#endif
  constexpr size_t TILE_B = sizeof(chunk) * 4 * NS * NB * (TA / VEC);
  constexpr size_t RED_B = sizeof(real) * R2 * R2;
  __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_B > RED_B ? TILE_B : RED_B];
  using tiles_t = chunk[NS][NB][TA / VEC];
  tiles_t* lds = reinterpret_cast<tiles_t*>(smem);
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int kk = l >> 4, i = l & 15;
  const bool part = (i & 1) != 0;
  uint32_t rd[4][NT];  // this lane's operand cells, per K step and component tile
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int j = 4 * s + kk, c = (i >> 1) + 8 * t;
      rd[s][t] = GATHER ? (uint32_t)(j * C + c) : qkl_swz(g.l.eoff[c] | g.l.eg[j]);
    }
  acc_t acc[NCH][NT][NT];
#pragma unroll
  for (int h = 0; h < NCH; ++h)
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = 0; tj < NT; ++tj) acc[h][ti][tj] = acc_t{0, 0, 0, 0};
  // f32: an MFMA accumulator is one fmaf chain over every group its wave visits (2^11 and more
  // at n = 28), whose rounding error grows with its length.  Every FLUSH iterations the chains
  // are added into a second set of registers and restarted: two short chains instead of one
  // long one.  (f64 stays well inside its tolerance without, and has no registers to spare.)
  constexpr bool TWO = sizeof(real) == 4;
  constexpr uint32_t FLUSH = 4;
  acc_t outer[NT][NT];
#pragma unroll
  for (int ti = 0; ti < NT; ++ti)
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) outer[ti][tj] = acc_t{0, 0, 0, 0};
  // one staged tile: 4 K steps of 4 groups
  auto contract = [&](int nb) __attribute__((always_inline)) {
    const cx* cf = reinterpret_cast<const cx*>(&lds[w][0][nb][0]);
    const cx* cb = reinterpret_cast<const cx*>(&lds[w][NS - 1][nb][0]);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      real av[NT], bv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const cx xf = cf[rd[s][t]];
        bv[t] = part ? xf.y : xf.x;
        if constexpr (DENS) {
          av[t] = bv[t];
        } else {
          const cx xb = cb[rd[s][t]];
          av[t] = part ? xb.y : xb.x;
        }
      }
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
          if (DENS && tj < ti) continue;  // symmetric: mirrored by k_qkg_fin
          acc_t& d = acc[s % NCH][ti][tj];
#ifdef QDC_F64
          d = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ti], bv[tj], d, 0, 0, 0);
#else
          d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ti], bv[tj], d, 0, 0, 0);
#endif
        }
    }
  };
  if constexpr (GATHER) {
    // fewer than 16 groups: one tile on one wave, cell j*C + ci = amplitude ci of group j,
    // the dead groups (K lanes) zero
    if (blockIdx.x == 0 && w == 0) {
      cx* wf = reinterpret_cast<cx*>(&lds[0][0][0][0]);
      cx* wb = reinterpret_cast<cx*>(&lds[0][NS - 1][0][0]);
#pragma unroll
      for (int it = 0; it < TA / 64; ++it) {
        const uint32_t e = (uint32_t)(it * 64 + l);
        const uint64_t grp = e / C;
        const bool live = grp < g.q.ngroups;
        uint64_t base = grp;
#pragma unroll
        for (int t = 0; t < K; ++t) base = insert_zero(base, g.q.sorted[t]);
        const uint64_t a = base + g.q.off[e % C];
        wf[e] = live ? f[a] : cx{0, 0};
        if constexpr (!DENS) wb[e] = live ? b[a] : cx{0, 0};
      }
      __builtin_amdgcn_wave_barrier();
      contract(0);
    }
  } else {
    uint32_t pc[NP];  // this lane's pieces: LDS chunk and amplitude offset from the tile base
    uint64_t po[NP];
    const uint32_t hmask = (1u << g.l.h) - 1u;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const uint32_t e = (uint32_t)(p * 64 + l) * VEC;
      pc[p] = qkl_swz(e) / VEC;
      po[p] = g.l.choff[e >> g.l.h] + (e & hmask);
    }
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    chunk raw[NS][NB][NP];
    auto load = [&](uint64_t t0) __attribute__((always_inline)) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        uint64_t base = (t0 + nb) << g.l.h;
        for (uint32_t t = 0; t < g.l.nhi; ++t) base = insert_zero(base, g.l.hi[t]);
        if (t0 + nb < g.l.ntiles) {  // wave-uniform
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            raw[0][nb][p] = ldc(reinterpret_cast<const chunk*>(f + base + po[p]));
            if constexpr (!DENS)
              raw[1][nb][p] = ldc(reinterpret_cast<const chunk*>(b + base + po[p]));
          }
        }
      }
    };
    const uint64_t step = nwaves * NB;
    uint64_t t0 = wave * NB;
    if (t0 < g.l.ntiles) load(t0);
    uint32_t it = 0;
    while (t0 < g.l.ntiles) {
#pragma unroll
      for (int st = 0; st < NS; ++st)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int p = 0; p < NP; ++p) lds[w][st][nb][pc[p]] = raw[st][nb][p];
      __builtin_amdgcn_wave_barrier();
      const uint64_t cur = t0;
      t0 += step;
      // the staged tiles free the load registers: the next tiles' loads fly while these run on
      // the matrix cores
      if (t0 < g.l.ntiles) load(t0);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (cur + nb < g.l.ntiles) contract(nb);  // wave-uniform
      __builtin_amdgcn_wave_barrier();  // the next tiles overwrite these cells
      if constexpr (TWO) {
        if ((++it & (FLUSH - 1)) == 0) {
#pragma unroll
          for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < NT; ++tj) {
              if (DENS && tj < ti) continue;
#pragma unroll
              for (int h = 0; h < NCH; ++h) {
                outer[ti][tj] += acc[h][ti][tj];
                acc[h][ti][tj] = acc_t{0, 0, 0, 0};
              }
            }
        }
      }
    }
  }
  // block partial: the waves add their tiles in LDS in wave order (P row-major, 2C x 2C)
  __syncthreads();
  real* red = reinterpret_cast<real*>(smem);
  for (int wv = 0; wv < 4; ++wv) {
    if (w == wv) {
#pragma unroll
      for (int ti = 0; ti < NT; ++ti)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
          // the density's tiles below the diagonal stay unwritten in the partial (k_qkg_fin never
          // reads them).  Storing their zeros also tripped hipcc (ROCm 7): it paired two of the
          // constant stores into one ds_write2st64_b32 whose first half landed on tile (0, 1)
          if (DENS && tj < ti) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // D row of lane group kk, register r: f32 4 kk + r; f64 kk + 4 r (qk_operands)
#ifdef QDC_F64
            const int row = kk + 4 * r;
#else
            const int row = 4 * kk + r;
#endif
            real v = acc[0][ti][tj][r];
            if constexpr (NCH == 2) v += acc[NCH - 1][ti][tj][r];
            if constexpr (TWO) v += outer[ti][tj][r];
            const int at = (16 * ti + row) * R2 + 16 * tj + i;
            red[at] = wv == 0 ? v : red[at] + v;
          }
        }
    }
    __syncthreads();
  }
  real* out = parts + (size_t)blockIdx.x * (R2 * R2);
  for (int e = threadIdx.x; e < R2 * R2; e += 256) out[e] = red[e];
}

// out[r*C + c] = the complex combination of the four real quadrants of sum over partials of P.
// 64 outputs per block, the partials split over the block's four waves (p = wave, wave + 4, ...)
// and their sums added in wave order.
template <bool DENS>
__global__ __launch_bounds__(256) void k_qkg_fin(const real* __restrict__ parts, uint32_t nparts,
                                                 uint32_t C, cx* __restrict__ out) {
  __shared__ real sh[4][4][64];
  const uint32_t t = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const uint32_t o = blockIdx.x * 64 + t, r = o / C, c = o % C, R2 = 2 * C;
  // the density's tiles below the diagonal are not computed: P[i][j] = P[j][i]
  const bool mir = DENS && (c >> 3) < (r >> 3);
  const uint32_t i0 = mir ? 2 * c : 2 * r, j0 = mir ? 2 * r : 2 * c;
  real q[4] = {0, 0, 0, 0};
  for (uint32_t p = sl; p < nparts; p += 4) {
    const real* P = parts + (size_t)p * R2 * R2 + (size_t)i0 * R2 + j0;
    q[0] += P[0];
    q[1] += P[1];
    q[2] += P[R2];
    q[3] += P[R2 + 1];
  }
#pragma unroll
  for (int x = 0; x < 4; ++x) sh[sl][x][t] = q[x];
  __syncthreads();
  if (sl != 0) return;
#pragma unroll
  for (int x = 0; x < 4; ++x) q[x] = ((sh[0][x][t] + sh[1][x][t]) + sh[2][x][t]) + sh[3][x][t];
  const real rr = q[0], ri = mir ? q[2] : q[1], ir = mir ? q[1] : q[2], ii = q[3];
  out[o] = DENS ? cx{rr + ii, ir - ri} : cx{rr - ii, ri + ir};
}

// Per-device scratch of this path (the context's RED-wide reduction slots cannot hold C^2
// values): the blocks' partials, the device result and its pinned host copy.  Guarded by the
// ABI mutex; every call ends with a stream synchronisation, so growing never frees a buffer
// in use.
struct QkgScratch {
  real* parts = nullptr;
  size_t cap = 0;  // reals
  cx* dres = nullptr;
  cx* hres = nullptr;
  uint32_t resident[2][3] = {};  // blocks the device holds at once, per kernel (0: not asked yet)
  const char* reserve(size_t nreals) {
    if (!dres) {
      QDC_HIP(hipMalloc(&dres, sizeof(cx) << (2 * QK_MAX)));
      QDC_HIP(hipHostMalloc(&hres, sizeof(cx) << (2 * QK_MAX)));
    }
    if (nreals <= cap) return nullptr;
    if (parts) QDC_HIP(hipFree(parts));
    parts = nullptr;
    cap = 0;
    QDC_HIP(hipMalloc(&parts, nreals * sizeof(real)));
    cap = nreals;
    return nullptr;
  }
};

// host `out[0 .. C*C)` += the gradient (b != nullptr) or the density (b == nullptr) of the
// k >= 3 qubits pos[0..k).  One stream synchronisation, at the host copy.
inline const char* reduce_qk(Ctx& c, const cx* f, const cx* b, qdc_complex* out, const size_t* pos,
                             uint32_t k, uint32_t n, QkgScratch& sc) {
  const uint32_t C = 1u << k;
  const bool dens = b == nullptr;
  qkg_geo g{};
  const bool staged = qkl_plan(pos, k, n, g.l);
  if (!staged) {
    g.q.k = k;
    g.q.ngroups = (uint64_t)1 << (n - k);
    for (uint32_t t = 0; t < k; ++t) g.q.sorted[t] = (uint32_t)pos[t];
    std::sort(g.q.sorted, g.q.sorted + k);
    for (uint32_t ci = 0; ci < C; ++ci) {
      uint64_t o = 0;
      for (uint32_t t = 0; t < k; ++t)
        if ((ci >> (k - 1 - t)) & 1u) o |= (uint64_t)1 << pos[t];
      g.q.off[ci] = o;
    }
  }
  // tiles per wave iteration: 4 KiB per state and wave (f64 at k = 5: 8 KiB, one tile)
  constexpr bool f64 = sizeof(real) == 8;
  constexpr int NB3 = f64 ? 2 : 4, NB4 = f64 ? 1 : 2;
  const uint64_t nb = k == 3 ? NB3 : k == 4 ? NB4 : 1;
  using kern_t = void (*)(const cx*, const cx*, real*, qkg_geo);
  static const kern_t staged_k[2][3] = {
      {k_qkg<3, NB3, false, false>, k_qkg<4, NB4, false, false>, k_qkg<5, 1, false, false>},
      {k_qkg<3, NB3, true, false>, k_qkg<4, NB4, true, false>, k_qkg<5, 1, true, false>}};
  static const kern_t gather_k[2][3] = {
      {k_qkg<3, 1, false, true>, k_qkg<4, 1, false, true>, k_qkg<5, 1, false, true>},
      {k_qkg<3, 1, true, true>, k_qkg<4, 1, true, true>, k_qkg<5, 1, true, true>}};
  static const char* const names[2][3] = {{"grad_qk3", "grad_qk4", "grad_qk5"},
                                          {"density_qk3", "density_qk4", "density_qk5"}};
  const kern_t kern = (staged ? staged_k : gather_k)[dens][k - 3];
  uint32_t grid = 1;
  if (staged) {
    // blocks: what the device holds at once (registers and LDS decide: 1 to 5 blocks per CU,
    // `make resource`), at most four per CU; QDC_QKG_GRID: another cap
    uint32_t& res = sc.resident[dens][k - 3];
    if (res == 0) {
      int per_cu = 0, cus = 0;
      QDC_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, 0));
      QDC_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device));
      res = (uint32_t)std::max(1, std::min(per_cu, 4) * cus);
    }
    const uint32_t gmax = (uint32_t)knob_long(Knob::QKG_GRID, (long)std::min(res, QKG_GRID_MAX), 1,
                                              (long)QKG_GRID_MAX);
    const uint64_t waves = (g.l.ntiles + nb - 1) / nb;
    grid = (uint32_t)std::min<uint64_t>((waves + 3) / 4, gmax);
  }
  const size_t pw = (size_t)4 * C * C;  // reals per partial
  QDC_TRY(sc.reserve((size_t)grid * pw));
  c.next_flops = 8.0 * C * (double)((uint64_t)1 << n);  // C complex MACs per amplitude
  const double bytes = (dens ? 1.0 : 2.0) * state_bytes(n);
  QDC_TRY(c.launch_block(names[dens][k - 3], bytes, kern, grid, 256u, f, b, sc.parts, g));
  QDC_TRY(dens ? c.launch_block("finalize", 0.0, k_qkg_fin<true>, C * C / 64, 256u,
                                (const real*)sc.parts, grid, C, sc.dres)
               : c.launch_block("finalize", 0.0, k_qkg_fin<false>, C * C / 64, 256u,
                                (const real*)sc.parts, grid, C, sc.dres));
  QDC_HIP(hipMemcpyAsync(sc.hres, sc.dres, sizeof(cx) * C * C, hipMemcpyDeviceToHost, c.stream));
  QDC_HIP(hipStreamSynchronize(c.stream));
  for (uint32_t x = 0; x < C * C; ++x) {
    out[x].re += sc.hres[x].x;
    out[x].im += sc.hres[x].y;
  }
  return nullptr;
}

}  // namespace qdc

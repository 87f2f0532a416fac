// qdc_sample.hpp — bitstring sampling from |psi|^2 (include/qdc/sample.h: qdc_sample,
// qdc_sample_plan, qdc_sample_assign) by a two-pass inverse CDF.
//
// Definition.  p_i = re_i^2 + im_i^2 in double (two products, one sum, no contraction: what
// numpy computes from the stored amplitudes), N = sum p_i, C_i = sum_{j <= i} p_j, and for a
// uniform u in [0, 1) with t = u N (one double product)
//     out = min { i : C_i > t }.
// The sums are floating point; what holds by construction is: the chosen index has p > 0, the
// result is monotone in u, and the same call returns the same bits (fixed trees, no atomics).
//
// The state is cut into SEGMENTS of 2^G amplitudes (G = SAMPLE_G; a state below that: one).
//   pass A, k_sample_sums: one double per segment, the state read once.
//   host, sample_assign:   long-double prefix of the segment sums -> N; per shot t, its segment
//                          (first s with prefix_incl[s] > t: a zero-mass segment is never first;
//                          past the end: the last segment with mass) and the residual
//                          r = t - prefix_excl[s] >= 0; the shots ordered by (segment, r).
//   pass B, k_sample_locate: one block per distinct hit segment walks it span by span (a span is
//                          k_prot_self's: 256 * PAULI_FU chunks = 2^PL_L amplitudes) and places
//                          its shots, which arrive ascending in r.
//
// The scan of a span (pass B) is a hierarchy whose every level is monotone and whose zeros stay
// zeros, so the properties above need no argument about rounding:
//   run    thread T owns the SAMPLE_NS consecutive amplitudes NS T .. NS T + NS - 1 (transposed
//          through LDS from the load order) and sums them sequentially: run[j] <= run[j + 1],
//          equal exactly where p = 0.
//   E[T]   the inclusive scan of the threads' totals: a shuffle scan inside each wave, made
//          monotone by a running maximum (max is exact), the waves' totals added sequentially,
//          so E of a wave's last thread IS the next wave's offset.
//   base   the spans' totals E[255], added sequentially as the block walks.
// A shot belongs to the first span with base + E[255] > r; in it rs = r - base >= 0, its thread
// is the first T with E[T] > rs that has mass (none: the last thread with mass), and inside the
// thread the first j with run[j] > max(rs - E[T - 1], 0) (none: the thread's last increase).  A
// shot past the segment's last partial sum goes to the segment's last index with p > 0, which
// the block tracks as it walks.
#pragma once

#include <algorithm>
#include <utility>
#include <vector>

#include "qdc_paulilayer.hpp"

namespace qdc {

constexpr uint32_t SAMPLE_G = 16;                 // log2(amplitudes of a segment)
constexpr int SAMPLE_NS = PAULI_FU * VEC;         // amplitudes of a thread and span
constexpr uint32_t SAMPLE_SPAN = 1u << PL_L;      // amplitudes of a span
static_assert(SAMPLE_G >= PL_L && SAMPLE_G <= 16, "a segment is whole spans, at most 2^16");
static_assert(SAMPLE_NS * 256 == (int)SAMPLE_SPAN, "a span is the block's runs");

// p of one amplitude, in double, rounded as numpy rounds re^2 + im^2
__device__ __forceinline__ double sample_p(cx a) {
  const double x = (double)a.x, y = (double)a.y;
  return __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y));
}

// The chunks of span sp of a segment that starts at chunk cbase and holds segch chunks (a state
// below one span: the chunks past it read as zeros; below one chunk: namps amplitudes and zeros)
__device__ __forceinline__ void sample_load(const cx* __restrict__ s, uint64_t cbase,
                                            uint32_t segch, uint32_t sp, uint32_t namps,
                                            chunk (&fa)[PAULI_FU]) {
  constexpr uint32_t SPANCH = 256u * PAULI_FU;
  const chunk* sc = reinterpret_cast<const chunk*>(s);
  const uint32_t c0 = sp * SPANCH + threadIdx.x;
  if (c0 - threadIdx.x + SPANCH <= segch) {
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) fa[u] = ldc(sc + cbase + c0 + 256u * u);
  } else {
    const bool part = namps < (uint32_t)VEC;  // below one chunk: segch = 1
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) {
      const uint32_t ci = c0 + 256u * u;
      fa[u] = chunk{};
      if (ci < segch) fa[u] = part ? pauli_ld(s, 0, namps) : ldc(sc + cbase + ci);
    }
  }
}

// Pass A.  sums[g] = sum of p over segment g (segch chunks each), g < nseg: per thread over its
// chunks in load order, xor-shuffle tree over the wave, the four waves in order.
__global__ __launch_bounds__(256) void k_sample_sums(const cx* __restrict__ s, uint32_t segch,
                                                     uint32_t namps, uint64_t nseg,
                                                     double* __restrict__ sums) {
  constexpr uint32_t SPANCH = 256u * PAULI_FU;
  __shared__ double wsum[2][BLOCK / 64];
  const uint32_t nsp = (segch + SPANCH - 1) / SPANCH;
  uint32_t flip = 0;
  for (uint64_t g = blockIdx.x; g < nseg; g += gridDim.x, flip ^= 1u) {
    const uint64_t cbase = g * segch;
    double acc = 0;
    for (uint32_t sp = 0; sp < nsp; ++sp) {
      chunk fa[PAULI_FU];
      sample_load(s, cbase, segch, sp, namps, fa);
#pragma unroll
      for (int u = 0; u < PAULI_FU; ++u)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc = __dadd_rn(acc, sample_p(fa[u].v[v]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, o, 64));
    if ((threadIdx.x & 63u) == 0) wsum[flip][threadIdx.x >> 6] = acc;
    __syncthreads();  // (the buffers alternate: the next segment's writes need no second barrier)
    if (threadIdx.x == 0) {
      double t = wsum[flip][0];
#pragma unroll
      for (int w = 1; w < BLOCK / 64; ++w) t = __dadd_rn(t, wsum[flip][w]);
      sums[g] = t;
    }
  }
}

// Pass B.  Block b places shots [start[b], start[b + 1]) of the sorted order (residuals r
// ascending) in segment segid[b]: out[perm[k]] = the sampled index.  segbits = log2 of the
// segment's amplitudes.
__global__ __launch_bounds__(256) void k_sample_locate(
    const cx* __restrict__ s, uint32_t segbits, uint32_t namps,
    const unsigned long long* __restrict__ segid, const unsigned long long* __restrict__ start,
    const double* __restrict__ r, const unsigned long long* __restrict__ perm,
    unsigned long long* __restrict__ out) {
  constexpr uint32_t SPANCH = 256u * PAULI_FU;
  constexpr int NS = SAMPLE_NS;
  __shared__ double run[SAMPLE_SPAN];  // p in load order, then the threads' runs in index order
  __shared__ double E[256];
  __shared__ double wtot[BLOCK / 64];
  __shared__ int wlast[BLOCK / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint64_t seg = segid[blockIdx.x];
  const uint64_t k1 = start[blockIdx.x + 1];
  uint64_t next = start[blockIdx.x];
  const uint32_t segch = (1u << segbits) < (uint32_t)VEC ? 1u : (1u << segbits) / VEC;
  const uint32_t nsp = (segch + SPANCH - 1) / SPANCH;
  const uint64_t cbase = seg * segch, abase = seg << segbits;
  double base = 0;
  int mylast = -1;  // this thread's last amplitude with an increase, relative to the segment
  double rk = next + t < k1 ? r[next + t] : 0.0;  // the residual of shot next + t
  chunk fa[PAULI_FU], nx[PAULI_FU];
  sample_load(s, cbase, segch, 0, namps, fa);
  for (uint32_t sp = 0; sp < nsp && next < k1; ++sp) {
    if (sp + 1 < nsp) sample_load(s, cbase, segch, sp + 1, namps, nx);  // in flight over the scan
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) run[(256u * u + t) * VEC + v] = sample_p(fa[u].v[v]);
    __syncthreads();
    double a[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) a[j] = run[NS * t + j];
    if (a[0] > 0) mylast = (int)(sp * SAMPLE_SPAN + NS * t);
#pragma unroll
    for (int j = 1; j < NS; ++j) {
      const double q = __dadd_rn(a[j - 1], a[j]);
      if (q > a[j - 1]) mylast = (int)(sp * SAMPLE_SPAN + NS * t + j);
      a[j] = q;
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) run[NS * t + j] = a[j];
    double e = a[NS - 1];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double v = __shfl_up(e, o, 64);
      if (lane >= (uint32_t)o) e = __dadd_rn(e, v);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double v = __shfl_up(e, o, 64);
      if (lane >= (uint32_t)o) e = fmax(e, v);
    }
    if (lane == 63u) wtot[wave] = e;
    __syncthreads();
    double off = 0, etot = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
      if ((uint32_t)w == wave) off = etot;
      etot = __dadd_rn(etot, wtot[w]);
    }
    E[t] = __dadd_rn(off, e);
    const double nb = __dadd_rn(base, etot);  // the next span's base
    __syncthreads();
    // the shots of this span: a prefix of those left
    for (;;) {
      const uint64_t k = next + t;
      const bool mine = k < k1 && rk < nb;
      const int cnt = __syncthreads_count(mine);
      if (mine) {
        const double rs = rk - base;  // >= 0: the shot was not taken before
        uint32_t lo = 0, hi = 256;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (E[mid] > rs) hi = mid; else lo = mid + 1;
        }
        uint32_t T = lo;
        while (T < 256u && !(run[NS * T + NS - 1] > 0)) ++T;
        if (T == 256u) {  // (etot > 0: a thread with mass exists)
          T = 255u;
          while (T > 0 && !(run[NS * T + NS - 1] > 0)) --T;
        }
        const double rr = fmax(rs - (T ? E[T - 1] : 0.0), 0.0);
        int pos = -1, inc = 0;
        double prev = 0;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
          const double q = run[NS * T + j];
          if (q > prev) inc = j;
          if (pos < 0 && q > rr) pos = j;
          prev = q;
        }
        if (pos < 0) pos = inc;
        out[perm[k]] = abase + (uint64_t)sp * SAMPLE_SPAN + NS * T + (uint32_t)pos;
      }
      if (cnt > 0) {
        next += (uint64_t)cnt;
        rk = next + t < k1 ? r[next + t] : 0.0;
      }
      if (cnt < BLOCK) break;
    }
    base = nb;
#pragma unroll
    for (int u = 0; u < PAULI_FU; ++u) fa[u] = nx[u];
    __syncthreads();  // the next span overwrites the scan
  }
  if (next < k1) {  // residuals at or past the segment's last partial sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mylast = max(mylast, __shfl_xor(mylast, o, 64));
    if (lane == 0) wlast[wave] = mylast;
    __syncthreads();
    int last = wlast[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) last = max(last, wlast[w]);
    const uint64_t idx = abase + (uint64_t)(last < 0 ? 0 : last);
    for (uint64_t k = next + t; k < k1; k += BLOCK) out[perm[k]] = idx;
  }
}

// ---- host ----------------------------------------------------------------------------------
struct SamplePlan {
  uint32_t segbits;   // log2(amplitudes of a segment) = min(G, n)
  uint64_t segments;  // 2^(n - segbits)
};
inline SamplePlan sample_plan(size_t n) {
  SamplePlan P;
  P.segbits = (uint32_t)std::min<size_t>(SAMPLE_G, n);
  P.segments = (uint64_t)1 << (n - P.segbits);
  return P;
}

inline const char* sample_check_uniforms(const double* u, size_t shots) {
  if (shots > 0 && !u) return fail("The sample has no uniforms.");
  for (size_t k = 0; k < shots; ++k)
    if (!(u[k] >= 0.0 && u[k] < 1.0)) return fail("uniforms must be in [0, 1).");
  return nullptr;
}

// The step between the passes.  seg[k], resid[k] in the caller's order; perm = the processing
// order (segments ascending, residuals ascending within one); *total = N.  The norm's errors
// are raised only when there are shots to place.
inline const char* sample_assign(const double* seg_sums, size_t segments, const double* u,
                                 size_t shots, unsigned long long* seg, double* resid,
                                 unsigned long long* perm, double* total) {
  if (!seg_sums || segments == 0) return fail("The sample has no segment sums.");
  QDC_TRY(sample_check_uniforms(u, shots));
  if (shots > 0 && (!seg || !resid || !perm)) return fail("The sample has no output buffers.");
  std::vector<long double> incl(segments);
  long double acc = 0;
  size_t lastnz = segments;
  for (size_t s = 0; s < segments; ++s) {
    acc += (long double)seg_sums[s];
    incl[s] = acc;
    if (seg_sums[s] > 0) lastnz = s;
  }
  const double N = (double)acc;
  if (total) *total = N;
  if (shots == 0) return nullptr;
  if (!std::isfinite(N)) return fail("The state is not finite.");
  if (N == 0 || lastnz == segments) return fail("The state has zero norm.");
  // t = u N is monotone in u: the order of the uniforms (ties by shot number) is the order of
  // (segment, residual)
  std::vector<std::pair<double, unsigned long long>> ord(shots);
  for (size_t k = 0; k < shots; ++k) ord[k] = {u[k], k};
  std::sort(ord.begin(), ord.end());
  for (size_t k = 0; k < shots; ++k) perm[k] = ord[k].second;
  size_t s = 0;
  for (size_t i = 0; i < shots; ++i) {
    const size_t k = (size_t)perm[i];
    const double t = u[k] * N;
    while (s < segments && !(incl[s] > (long double)t)) ++s;
    const size_t g = s < segments ? s : lastnz;
    const long double ex = g > 0 ? incl[g - 1] : 0.0L;
    seg[k] = g;
    resid[k] = std::max(0.0, (double)((long double)t - ex));
  }
  return nullptr;
}

// The tables of pass B: blocks (segid, start) over the sorted residuals rs.
struct SampleTables {
  std::vector<unsigned long long> segid, start;
  std::vector<double> rs;
};
inline void sample_tables(const unsigned long long* seg, const double* resid,
                          const unsigned long long* perm, size_t shots, SampleTables& T) {
  T.segid.clear();
  T.start.clear();
  T.rs.resize(shots);
  for (size_t i = 0; i < shots; ++i) {
    const size_t k = (size_t)perm[i];
    T.rs[i] = resid[k];
    if (T.segid.empty() || T.segid.back() != seg[k]) {
      T.segid.push_back(seg[k]);
      T.start.push_back(i);
    }
  }
  T.start.push_back(shots);
}

// Every index the kernel reads from the tables, checked before the launch: the segments exist
// and ascend, the shot ranges partition [0, shots) in order, perm is a permutation of the shots,
// the residuals are non-negative and ascend inside a block.
inline const char* sample_check_tables(const SampleTables& T, const unsigned long long* perm,
                                       size_t shots, uint64_t segments) {
  const size_t nb = T.segid.size();
  if (nb == 0 || T.start.size() != nb + 1 || T.rs.size() != shots || nb > shots)
    return fail("sample tables: inconsistent sizes");
  if (T.start[0] != 0 || T.start[nb] != shots) return fail("sample tables: the ranges do not cover the shots");
  for (size_t b = 0; b < nb; ++b) {
    if (T.segid[b] >= segments || (b > 0 && T.segid[b] <= T.segid[b - 1]))
      return fail("sample tables: segment %zu out of range or out of order", b);
    if (T.start[b] >= T.start[b + 1]) return fail("sample tables: empty or reversed range %zu", b);
    for (size_t i = (size_t)T.start[b]; i < (size_t)T.start[b + 1]; ++i)
      if (!(T.rs[i] >= 0.0) || (i > T.start[b] && T.rs[i] < T.rs[i - 1]))
        return fail("sample tables: residuals of block %zu not ascending", b);
  }
  std::vector<uint8_t> seen(shots, 0);
  for (size_t i = 0; i < shots; ++i) {
    if (perm[i] >= shots || seen[(size_t)perm[i]]) return fail("sample tables: perm is not a permutation");
    seen[(size_t)perm[i]] = 1;
  }
  return nullptr;
}

// device scratch of one device's sampling calls (grown, never shrunk; guarded by the ABI mutex)
struct SampleScratch {
  char* dev = nullptr;
  size_t cap = 0;
  const char* ensure(size_t bytes) {
    if (bytes <= cap) return nullptr;
    if (dev) QDC_HIP(hipFree(dev));
    dev = nullptr;
    cap = 0;
    QDC_HIP(hipMalloc(reinterpret_cast<void**>(&dev), bytes));
    cap = bytes;
    return nullptr;
  }
};

// out[k] = the index sampled by u[k]; *norm2 = N.  The uniforms are checked by the caller.
inline const char* sample(Ctx& c, const cx* s, uint32_t n, const double* u, size_t shots,
                          unsigned long long* out, double* norm2, SampleScratch& S) {
  const SamplePlan P = sample_plan(n);
  const uint32_t segch = std::max<uint32_t>(1u, (1u << P.segbits) / VEC);
  const uint32_t namps = (uint32_t)std::min<uint64_t>((uint64_t)1 << n, VEC);
  const size_t nb_max = (size_t)std::min<uint64_t>(P.segments, shots);
  // [sums | r | perm | out | segid | start], every part a multiple of 8 bytes
  const size_t o_r = sizeof(double) * P.segments, o_perm = o_r + 8 * shots,
               o_out = o_perm + 8 * shots, o_seg = o_out + 8 * shots, o_start = o_seg + 8 * nb_max,
               bytes = o_start + 8 * (nb_max + 1);
  QDC_TRY(S.ensure(bytes));
  double* d_sums = reinterpret_cast<double*>(S.dev);
  const uint32_t grid = (uint32_t)std::min<uint64_t>(P.segments, 1u << 20);
  QDC_TRY(c.launch_block("sample_sums", state_bytes(n), k_sample_sums, grid, 256u, s, segch, namps,
                         P.segments, d_sums));
  std::vector<double> sums(P.segments);
  QDC_HIP(hipMemcpyAsync(sums.data(), d_sums, sizeof(double) * P.segments, hipMemcpyDeviceToHost,
                         c.stream));
  QDC_HIP(hipStreamSynchronize(c.stream));
  std::vector<unsigned long long> seg(shots), perm(shots);
  std::vector<double> resid(shots);
  double N = 0;
  QDC_TRY(sample_assign(sums.data(), sums.size(), u, shots, seg.data(), resid.data(), perm.data(),
                        &N));
  if (norm2) *norm2 = N;
  if (shots == 0) return nullptr;
  SampleTables T;
  sample_tables(seg.data(), resid.data(), perm.data(), shots, T);
  QDC_TRY(sample_check_tables(T, perm.data(), shots, P.segments));
  const size_t nb = T.segid.size();
  auto* d_r = reinterpret_cast<double*>(S.dev + o_r);
  auto* d_perm = reinterpret_cast<unsigned long long*>(S.dev + o_perm);
  auto* d_out = reinterpret_cast<unsigned long long*>(S.dev + o_out);
  auto* d_seg = reinterpret_cast<unsigned long long*>(S.dev + o_seg);
  auto* d_start = reinterpret_cast<unsigned long long*>(S.dev + o_start);
  QDC_HIP(hipMemcpyAsync(d_r, T.rs.data(), 8 * shots, hipMemcpyHostToDevice, c.stream));
  QDC_HIP(hipMemcpyAsync(d_perm, perm.data(), 8 * shots, hipMemcpyHostToDevice, c.stream));
  QDC_HIP(hipMemcpyAsync(d_seg, T.segid.data(), 8 * nb, hipMemcpyHostToDevice, c.stream));
  QDC_HIP(hipMemcpyAsync(d_start, T.start.data(), 8 * (nb + 1), hipMemcpyHostToDevice, c.stream));
  const double read = (double)nb * (double)((uint64_t)1 << P.segbits) * sizeof(cx);
  QDC_TRY(c.launch_block("sample_locate", read, k_sample_locate, (uint32_t)nb, 256u, s, P.segbits,
                         namps, (const unsigned long long*)d_seg, (const unsigned long long*)d_start,
                         (const double*)d_r, (const unsigned long long*)d_perm, d_out));
  QDC_HIP(hipMemcpyAsync(out, d_out, 8 * shots, hipMemcpyDeviceToHost, c.stream));
  QDC_HIP(hipStreamSynchronize(c.stream));  // (the host tables live until here)
  return nullptr;
}

}  // namespace qdc

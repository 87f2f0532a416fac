// qdc_primitives.hpp — the 18 reference C-ABI entry points (src/primitives_bind.rs:15-119,
// implemented for CUDA in src/primitives.cu:141-953) on the HIP kernels.
//
// Every call runs on a context of the device that is current for the calling thread (as the
// reference launches on the current device's legacy default stream): one non-blocking stream
// per device, ordered exactly like that default stream; host results (copies, densities,
// gradients) synchronise it.  A host that switches devices (hipSetDevice) between calls, or
// drives one GPU per thread, gets each device's own stream and scratch.  A mutex makes
// concurrent callers safe (the reference's are not, README.md:13).
#pragma once

#include "qdc/circuit.h"
#include "qdc/dense.h"
#include "qdc/overlap.h"
#include "qdc/pauli.h"
#include "qdc/sample.h"
#include "qdc_device.hpp"
#include "qdc_qk.hpp"
#include "qdc_qkgrad.hpp"
#include "qdc_pauli.hpp"
#include "qdc_overlap.hpp"
#include "qdc_paulirot.hpp"
#include "qdc_paulilayer.hpp"
#include "qdc_paulixlayer.hpp"
#include "qdc_sample.hpp"

namespace qdc {

inline std::mutex& abi_mutex() {
  static std::mutex m;
  return m;
}

constexpr int ABI_MAX_DEVICES = 64;

inline const char* abi_ctx(Ctx*& out) {
  static Ctx* ctx[ABI_MAX_DEVICES] = {};
  int dev = 0;
  QDC_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= ABI_MAX_DEVICES) return fail("device %d is out of the supported range", dev);
  if (!ctx[dev]) {
    Ctx* c = new Ctx();
    const char* e = c->init(dev);
    if (e) {
      delete c;
      return e;
    }
    ctx[dev] = c;
  }
  out = ctx[dev];
  return nullptr;
}

inline const char* check_n(size_t n) {
  if (n > 40) return fail("qubits_number %zu is out of the supported range (<= 40).", n);
  return nullptr;
}

// one reduction → host `out[0..K)` += result (the reference's `+=`, primitives.cu:281-288)
inline const char* abi_finish_reduction(Ctx& c, qdc_complex* out, int K) {
  QDC_TRY(c.flush());
  QDC_HIP(hipMemcpyAsync(c.host_results, c.results, sizeof(cx) * RED, hipMemcpyDeviceToHost,
                         c.stream));
  QDC_HIP(hipStreamSynchronize(c.stream));
  for (int k = 0; k < K; ++k) {
    out[k].re += c.host_results[k].x;
    out[k].im += c.host_results[k].y;
  }
  return nullptr;
}

// per-kernel sums of a context's profiled launches (qdc_circuit_profile_collect,
// qdc_abi_profile_collect)
inline size_t prof_collect(const std::vector<Ctx*>& xs, qdc_kernel_stat* out, size_t cap) {
  std::vector<qdc_kernel_stat> agg;
  for (Ctx* x : xs) {
    (void)x->sync();
    for (auto& r : x->prof.recs) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) ms = 0.f;
      qdc_kernel_stat* s = nullptr;
      for (auto& a : agg)
        if (strncmp(a.name, r.name, sizeof(a.name)) == 0) s = &a;
      if (!s) {
        agg.push_back({});
        s = &agg.back();
        strncpy(s->name, r.name, sizeof(s->name) - 1);
      }
      s->launches += 1;
      s->total_ms += ms;
      s->algo_bytes += r.bytes;
      s->algo_flops += r.flops;
    }
  }
  for (size_t i = 0; i < agg.size() && i < cap; ++i) out[i] = agg[i];
  return agg.size();
}
inline size_t prof_collect(Ctx& x, qdc_kernel_stat* out, size_t cap) {
  return prof_collect(std::vector<Ctx*>{&x}, out, cap);
}

}  // namespace qdc

#define QDC_ABI_BEGIN                                   \
  std::lock_guard<std::mutex> qdc_lock_(qdc::abi_mutex()); \
  qdc::Ctx* ctxp = nullptr;                             \
  QDC_TRY(qdc::abi_ctx(ctxp));                          \
  qdc::Ctx& ctx = *ctxp;

#define QDC_VOID(expr)                                                  \
  do {                                                                  \
    const char* qdc_v_ = (expr);                                        \
    if (qdc_v_) fprintf(stderr, "qdc: %s\n", qdc_v_);                   \
  } while (0)

static const char* set2standard_impl(qdc_complex* state, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  return qdc::set_standard(ctx, reinterpret_cast<qdc::cx*>(state), (uint32_t)n);
}

static const char* check_q2(size_t pos2, size_t pos1, size_t n) {
  if (pos1 == pos2) return qdc::fail("pos1 and pos2 must be different.");
  if (pos1 >= n) return qdc::fail("pos1 is out of the bound.");
  if (pos2 >= n) return qdc::fail("pos2 is out of the bound.");
  return nullptr;
}

template <int OP>
static const char* elementwise_impl(const qdc_complex* src, qdc_complex* dst, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  return qdc::elementwise<OP>(ctx, reinterpret_cast<const qdc::cx*>(src),
                              reinterpret_cast<qdc::cx*>(dst), (uint32_t)n);
}

extern "C" {

__attribute__((visibility("default"))) void set2standard(qdc_complex* state, size_t n) {
  QDC_VOID(set2standard_impl(state, n));
}

__attribute__((visibility("default"))) const char* get_state(qdc_complex** state, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  (void)ctx;
  QDC_HIP(hipMalloc(reinterpret_cast<void**>(state), ((size_t)1 << n) * sizeof(qdc_complex)));
  return nullptr;
}

__attribute__((visibility("default"))) const char* drop_state(qdc_complex* state) {
  QDC_ABI_BEGIN
  QDC_HIP(hipStreamSynchronize(ctx.stream));
  QDC_HIP(hipFree(state));
  return nullptr;
}

__attribute__((visibility("default"))) const char* copy_to_host(const qdc_complex* state,
                                                                qdc_complex* host, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_HIP(hipMemcpyAsync(host, state, ((size_t)1 << n) * sizeof(qdc_complex),
                         hipMemcpyDeviceToHost, ctx.stream));
  QDC_HIP(hipStreamSynchronize(ctx.stream));
  return nullptr;
}

__attribute__((visibility("default"))) const char* set_from_host(qdc_complex* dev,
                                                                 const qdc_complex* host,
                                                                 size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_HIP(hipMemcpyAsync(dev, host, ((size_t)1 << n) * sizeof(qdc_complex),
                         hipMemcpyHostToDevice, ctx.stream));
  QDC_HIP(hipStreamSynchronize(ctx.stream));
  return nullptr;
}

__attribute__((visibility("default"))) const char* q1gate(qdc_complex* state,
                                                          const qdc_complex* gate, size_t pos,
                                                          size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  if (pos >= n) return qdc::fail("pos is out of the bound.");
  return qdc::apply_dense<2>(ctx, reinterpret_cast<qdc::cx*>(state), qdc::to_mat<2>(gate),
                             (uint32_t)pos, (uint32_t)pos, (uint32_t)n, "q1gate");
}

__attribute__((visibility("default"))) const char* q1gate_inv(qdc_complex* state,
                                                              const qdc_complex* gate,
                                                              size_t pos, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  if (pos >= n) return qdc::fail("pos is out of the bound.");
  qdc::mat<2> inv;
  QDC_TRY(qdc::inverse<2>(qdc::to_mat<2>(gate), inv));
  return qdc::apply_dense<2>(ctx, reinterpret_cast<qdc::cx*>(state), inv, (uint32_t)pos,
                             (uint32_t)pos, (uint32_t)n, "q1gate");
}

__attribute__((visibility("default"))) const char* q2gate(qdc_complex* state,
                                                          const qdc_complex* gate, size_t pos2,
                                                          size_t pos1, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_q2(pos2, pos1, n));
  return qdc::apply_dense<4>(ctx, reinterpret_cast<qdc::cx*>(state), qdc::to_mat<4>(gate),
                             (uint32_t)pos2, (uint32_t)pos1, (uint32_t)n, "q2gate");
}

__attribute__((visibility("default"))) const char* q2gate_inv(qdc_complex* state,
                                                              const qdc_complex* gate,
                                                              size_t pos2, size_t pos1,
                                                              size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_q2(pos2, pos1, n));
  qdc::mat<4> inv;
  QDC_TRY(qdc::inverse<4>(qdc::to_mat<4>(gate), inv));
  return qdc::apply_dense<4>(ctx, reinterpret_cast<qdc::cx*>(state), inv, (uint32_t)pos2,
                             (uint32_t)pos1, (uint32_t)n, "q2gate");
}

__attribute__((visibility("default"))) const char* q2gate_diag(qdc_complex* state,
                                                               const qdc_complex* gate,
                                                               size_t pos2, size_t pos1,
                                                               size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_q2(pos2, pos1, n));
  return qdc::apply_diag(ctx, reinterpret_cast<qdc::cx*>(state), qdc::to_diag(gate),
                         (uint32_t)pos2, (uint32_t)pos1, (uint32_t)n, "q2gate_diag");
}

__attribute__((visibility("default"))) const char* get_q1density(const qdc_complex* state,
                                                                 qdc_complex* density,
                                                                 size_t pos, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  if (pos >= n) return qdc::fail("pos is out of the bound.");
  QDC_TRY(qdc::density<2>(ctx, reinterpret_cast<const qdc::cx*>(state), (uint32_t)pos,
                          (uint32_t)pos, (uint32_t)n, ctx.results, 0, 0));
  return qdc::abi_finish_reduction(ctx, density, 4);
}

__attribute__((visibility("default"))) const char* get_q2density(const qdc_complex* state,
                                                                 qdc_complex* density,
                                                                 size_t pos2, size_t pos1,
                                                                 size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_q2(pos2, pos1, n));
  QDC_TRY(qdc::density<4>(ctx, reinterpret_cast<const qdc::cx*>(state), (uint32_t)pos2,
                          (uint32_t)pos1, (uint32_t)n, ctx.results, 0, 0));
  return qdc::abi_finish_reduction(ctx, density, 16);
}

__attribute__((visibility("default"))) const char* q1grad(const qdc_complex* fwd,
                                                          const qdc_complex* bwd,
                                                          qdc_complex* grad, size_t pos,
                                                          size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  if (pos >= n) return qdc::fail("pos out of range.");
  QDC_TRY(qdc::grad_dense<2>(ctx, reinterpret_cast<const qdc::cx*>(fwd),
                             reinterpret_cast<const qdc::cx*>(bwd), (uint32_t)pos, (uint32_t)pos,
                             (uint32_t)n, ctx.results, 0, 0));
  return qdc::abi_finish_reduction(ctx, grad, 4);
}

__attribute__((visibility("default"))) const char* q2grad(const qdc_complex* fwd,
                                                          const qdc_complex* bwd,
                                                          qdc_complex* grad, size_t pos2,
                                                          size_t pos1, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_q2(pos2, pos1, n));
  QDC_TRY(qdc::grad_dense<4>(ctx, reinterpret_cast<const qdc::cx*>(fwd),
                             reinterpret_cast<const qdc::cx*>(bwd), (uint32_t)pos2,
                             (uint32_t)pos1, (uint32_t)n, ctx.results, 0, 0));
  return qdc::abi_finish_reduction(ctx, grad, 16);
}

__attribute__((visibility("default"))) const char* q2grad_diag(const qdc_complex* fwd,
                                                               const qdc_complex* bwd,
                                                               qdc_complex* grad, size_t pos2,
                                                               size_t pos1, size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_q2(pos2, pos1, n));
  QDC_TRY(qdc::grad_diag(ctx, reinterpret_cast<const qdc::cx*>(fwd),
                         reinterpret_cast<const qdc::cx*>(bwd), (uint32_t)pos2, (uint32_t)pos1,
                         (uint32_t)n, ctx.results, 0, 0));
  return qdc::abi_finish_reduction(ctx, grad, 4);
}

__attribute__((visibility("default"))) void conj_and_double(const qdc_complex* src,
                                                             qdc_complex* dst, size_t n) {
  QDC_VOID(elementwise_impl<1>(src, dst, n));
}

__attribute__((visibility("default"))) void add(const qdc_complex* src, qdc_complex* dst,
                                                size_t n) {
  QDC_VOID(elementwise_impl<2>(src, dst, n));
}

__attribute__((visibility("default"))) void copy(const qdc_complex* src, qdc_complex* dst,
                                                 size_t n) {
  QDC_VOID(elementwise_impl<0>(src, dst, n));
}

// ---- extensions beyond the reference's 18 entry points (include/qdc/dense.h) ----------------

}  // extern "C"

static const char* check_qk(const size_t* pos, size_t k, size_t n) {
  if (k < 1 || k > (size_t)qdc::QK_MAX)
    return qdc::fail("k = %zu qubits is out of the supported range (1..%d).", k, qdc::QK_MAX);
  if (k > n) return qdc::fail("k = %zu exceeds qubits_number %zu.", k, n);
  for (size_t b = 0; b < k; ++b) {
    if (pos[b] >= n) return qdc::fail("pos is out of the bound.");
    for (size_t c = 0; c < b; ++c)
      if (pos[c] == pos[b]) return qdc::fail("positions must be different.");
  }
  return nullptr;
}

extern "C" {

__attribute__((visibility("default"))) const char* qdc_qkgate(qdc_complex* state,
                                                              const qdc_complex* gate,
                                                              const size_t* pos, size_t k,
                                                              size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_qk(pos, k, n));
  static qdc::QkRing rings[qdc::ABI_MAX_DEVICES];  // guarded by the ABI mutex
  return qdc::apply_qk(ctx, reinterpret_cast<qdc::cx*>(state), gate, pos, (uint32_t)k,
                       (uint32_t)n, rings[ctx.device]);
}

__attribute__((visibility("default"))) const char* qdc_qkgrad(const qdc_complex* fwd,
                                                              const qdc_complex* bwd,
                                                              qdc_complex* grad,
                                                              const size_t* pos, size_t k,
                                                              size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_qk(pos, k, n));
  const qdc::cx* f = reinterpret_cast<const qdc::cx*>(fwd);
  const qdc::cx* b = reinterpret_cast<const qdc::cx*>(bwd);
  if (k <= 2) {  // q1grad / q2grad(pos[0], pos[1]), bit for bit
    const uint32_t p2 = (uint32_t)pos[0], p1 = (uint32_t)pos[k - 1];
    QDC_TRY(k == 1 ? qdc::grad_dense<2>(ctx, f, b, p2, p1, (uint32_t)n, ctx.results, 0, 0)
                   : qdc::grad_dense<4>(ctx, f, b, p2, p1, (uint32_t)n, ctx.results, 0, 0));
    return qdc::abi_finish_reduction(ctx, grad, k == 1 ? 4 : 16);
  }
  static qdc::QkgScratch scratch[qdc::ABI_MAX_DEVICES];  // guarded by the ABI mutex
  return qdc::reduce_qk(ctx, f, b, grad, pos, (uint32_t)k, (uint32_t)n, scratch[ctx.device]);
}

__attribute__((visibility("default"))) const char* qdc_qkdensity(const qdc_complex* state,
                                                                 qdc_complex* density,
                                                                 const size_t* pos, size_t k,
                                                                 size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(check_qk(pos, k, n));
  const qdc::cx* s = reinterpret_cast<const qdc::cx*>(state);
  if (k <= 2) {  // get_q1density / get_q2density(pos[0], pos[1]), bit for bit
    const uint32_t p2 = (uint32_t)pos[0], p1 = (uint32_t)pos[k - 1];
    QDC_TRY(k == 1 ? qdc::density<2>(ctx, s, p2, p1, (uint32_t)n, ctx.results, 0, 0)
                   : qdc::density<4>(ctx, s, p2, p1, (uint32_t)n, ctx.results, 0, 0));
    return qdc::abi_finish_reduction(ctx, density, k == 1 ? 4 : 16);
  }
  static qdc::QkgScratch scratch[qdc::ABI_MAX_DEVICES];  // guarded by the ABI mutex
  return qdc::reduce_qk(ctx, s, nullptr, density, pos, (uint32_t)k, (uint32_t)n,
                        scratch[ctx.device]);
}

// ---- Pauli-sum observables (include/qdc/pauli.h, qdc_pauli.hpp) ------------------------------

__attribute__((visibility("default"))) const char* qdc_pauli_energy(
    const qdc_complex* state, const unsigned long long* xmask, const unsigned long long* zmask,
    const double* coeff, size_t terms, size_t n, double* energy) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::PauliPlan plan;
  QDC_TRY(qdc::pauli_plan(xmask, zmask, coeff, terms, n, plan));
  return qdc::pauli_energy(ctx, reinterpret_cast<const qdc::cx*>(state), plan, (uint32_t)n, energy);
}

__attribute__((visibility("default"))) const char* qdc_pauli_inject(
    const qdc_complex* fwd, qdc_complex* bwd, const unsigned long long* xmask,
    const unsigned long long* zmask, const double* coeff, size_t terms, size_t n, double weight,
    int accumulate) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::PauliPlan plan;
  QDC_TRY(qdc::pauli_plan(xmask, zmask, coeff, terms, n, plan));
  if (!std::isfinite(weight)) return qdc::fail("Pauli coefficients must be finite.");
  if (fwd == bwd) return qdc::fail("fwd and bwd must be different states.");
  return qdc::pauli_inject(ctx, reinterpret_cast<const qdc::cx*>(fwd),
                           reinterpret_cast<qdc::cx*>(bwd), plan, (uint32_t)n, weight,
                           accumulate != 0);
}

// ---- overlaps and transition elements <a|H|b> (include/qdc/overlap.h, qdc_overlap.hpp) ---------

__attribute__((visibility("default"))) const char* qdc_overlap(const qdc_complex* a,
                                                               const qdc_complex* b, size_t n,
                                                               double out[2]) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  return qdc::overlap(ctx, reinterpret_cast<const qdc::cx*>(a),
                      reinterpret_cast<const qdc::cx*>(b), (uint32_t)n, out);
}

__attribute__((visibility("default"))) const char* qdc_pauli_overlap(
    const qdc_complex* a, const qdc_complex* b, const unsigned long long* xmask,
    const unsigned long long* zmask, const double* coeff, size_t terms, size_t n, double out[2]) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::PauliPlan plan;
  QDC_TRY(qdc::pauli_plan(xmask, zmask, coeff, terms, n, plan));
  return qdc::pauli_overlap(ctx, reinterpret_cast<const qdc::cx*>(a),
                            reinterpret_cast<const qdc::cx*>(b), plan, (uint32_t)n, out);
}

__attribute__((visibility("default"))) const char* qdc_overlap_inject(
    const qdc_complex* src, qdc_complex* bwd, size_t n, double g_re, double g_im,
    int accumulate) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  if (!std::isfinite(g_re) || !std::isfinite(g_im))
    return qdc::fail("Pauli coefficients must be finite.");
  if (src == bwd) return qdc::fail("fwd and bwd must be different states.");
  return qdc::overlap_inject(ctx, reinterpret_cast<const qdc::cx*>(src),
                             reinterpret_cast<qdc::cx*>(bwd), (uint32_t)n, g_re, g_im,
                             accumulate != 0);
}

__attribute__((visibility("default"))) const char* qdc_pauli_overlap_inject(
    const qdc_complex* src, qdc_complex* bwd, const unsigned long long* xmask,
    const unsigned long long* zmask, const double* coeff, size_t terms, size_t n, double g_re,
    double g_im, int accumulate) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::PauliPlan plan;
  QDC_TRY(qdc::pauli_plan(xmask, zmask, coeff, terms, n, plan));
  if (!std::isfinite(g_re) || !std::isfinite(g_im))
    return qdc::fail("Pauli coefficients must be finite.");
  if (src == bwd) return qdc::fail("fwd and bwd must be different states.");
  return qdc::pauli_overlap_inject(ctx, reinterpret_cast<const qdc::cx*>(src),
                                   reinterpret_cast<qdc::cx*>(bwd), plan, (uint32_t)n, g_re, g_im,
                                   accumulate != 0);
}

// ---- Pauli rotations exp(-i theta/2 P) (include/qdc/pauli.h, qdc_paulirot.hpp) ----------------

__attribute__((visibility("default"))) const char* qdc_pauli_rot(
    qdc_complex* state, unsigned long long xmask, unsigned long long zmask, double theta,
    size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::prot T;
  QDC_TRY(qdc::prot_make(xmask, zmask, theta, n, false, T));
  return qdc::pauli_rot(ctx, reinterpret_cast<qdc::cx*>(state), T, (uint32_t)n);
}

__attribute__((visibility("default"))) const char* qdc_pauli_rot_reverse(
    qdc_complex* fwd, qdc_complex* bwd, unsigned long long xmask, unsigned long long zmask,
    double theta, size_t n, double* dtheta) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::prot T;
  QDC_TRY(qdc::prot_make(xmask, zmask, theta, n, true, T));
  if (fwd == bwd) return qdc::fail("fwd and bwd must be different states.");
  if (!bwd && dtheta) return qdc::fail("A gradient needs a bwd state.");
  return qdc::pauli_rot_reverse(ctx, reinterpret_cast<qdc::cx*>(fwd),
                                reinterpret_cast<qdc::cx*>(bwd), T, (uint32_t)n, dtheta);
}

// host only: no context, no device
__attribute__((visibility("default"))) size_t qdc_pauli_plan(
    const unsigned long long* xmask, const unsigned long long* zmask, size_t terms, size_t n,
    unsigned* out, unsigned long long* group_x, size_t cap) {
  qdc::PauliPlan plan;
  if (!out || n > 40 || qdc::pauli_plan(xmask, zmask, nullptr, terms, n, plan)) return SIZE_MAX;
  const size_t ng = plan.win_x.size() + plan.far_x.size();
  if (ng > cap || (ng > 0 && !group_x)) return SIZE_MAX;
  const unsigned v[6] = {qdc::PAULI_W, (unsigned)plan.merged, (unsigned)plan.win_x.size(),
                         (unsigned)plan.far_x.size(), (unsigned)plan.launches(),
                         (unsigned)plan.launches()};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  size_t w = 0;
  for (uint64_t x : plan.win_x) group_x[w++] = x;
  for (uint64_t x : plan.far_x) group_x[w++] = x;
  return ng;
}

// ---- diagonal Pauli layers exp(-i/2 sum_k theta_k Z^{z_k}) (qdc_paulilayer.hpp) ---------------

__attribute__((visibility("default"))) const char* qdc_pauli_layer(
    qdc_complex* state, const unsigned long long* zmask, const double* theta, size_t terms,
    size_t n) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(qdc::pl_check(zmask, theta, terms, n));
  if (!theta) return qdc::fail("The layer has no angles.");
  return qdc::pauli_layer(ctx, reinterpret_cast<qdc::cx*>(state), zmask, theta, terms,
                          (uint32_t)n);
}

__attribute__((visibility("default"))) const char* qdc_pauli_layer_reverse(
    qdc_complex* fwd, qdc_complex* bwd, const unsigned long long* zmask, const double* theta,
    size_t terms, size_t n, double* dtheta) {
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  QDC_TRY(qdc::pl_check(zmask, theta, terms, n));
  if (!theta) return qdc::fail("The layer has no angles.");
  if (fwd == bwd) return qdc::fail("fwd and bwd must be different states.");
  if (!bwd && dtheta) return qdc::fail("A gradient needs a bwd state.");
  return qdc::pauli_layer_reverse(ctx, reinterpret_cast<qdc::cx*>(fwd),
                                  reinterpret_cast<qdc::cx*>(bwd), zmask, theta, terms,
                                  (uint32_t)n, dtheta);
}

// host only: no context, no device
__attribute__((visibility("default"))) size_t qdc_pauli_layer_plan(
    const unsigned long long* zmask, size_t terms, size_t n, unsigned* out) {
  if (!out || n > 40 || qdc::pl_check(zmask, nullptr, terms, n)) return SIZE_MAX;
  const qdc::PauliLayerPlan P = qdc::pl_plan(zmask, terms);
  const unsigned v[6] = {qdc::PL_L, P.groups, P.high, P.fwd, P.rev, P.rev_grad};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  return P.groups;
}

// ---- Pauli layers with a shared X/Y footprint (qdc_paulixlayer.hpp) ----------------------------

__attribute__((visibility("default"))) const char* qdc_pauli_xlayer(
    qdc_complex* state, unsigned long long xmask, const unsigned long long* zmask,
    const double* theta, size_t terms, size_t n) {
  if (xmask == 0) return qdc_pauli_layer(state, zmask, theta, terms, n);
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::PxLayer P;
  QDC_TRY(qdc::pxl_make(xmask, zmask, theta, terms, n, P));
  if (!theta) return qdc::fail("The layer has no angles.");
  return qdc::pauli_xlayer(ctx, reinterpret_cast<qdc::cx*>(state), P, theta, (uint32_t)n);
}

__attribute__((visibility("default"))) const char* qdc_pauli_xlayer_reverse(
    qdc_complex* fwd, qdc_complex* bwd, unsigned long long xmask,
    const unsigned long long* zmask, const double* theta, size_t terms, size_t n,
    double* dtheta) {
  if (xmask == 0) return qdc_pauli_layer_reverse(fwd, bwd, zmask, theta, terms, n, dtheta);
  QDC_ABI_BEGIN
  QDC_TRY(qdc::check_n(n));
  qdc::PxLayer P;
  QDC_TRY(qdc::pxl_make(xmask, zmask, theta, terms, n, P));
  if (!theta) return qdc::fail("The layer has no angles.");
  if (fwd == bwd) return qdc::fail("fwd and bwd must be different states.");
  if (!bwd && dtheta) return qdc::fail("A gradient needs a bwd state.");
  return qdc::pauli_xlayer_reverse(ctx, reinterpret_cast<qdc::cx*>(fwd),
                                   reinterpret_cast<qdc::cx*>(bwd), P, theta, (uint32_t)n, dtheta);
}

// host only: no context, no device
__attribute__((visibility("default"))) size_t qdc_pauli_xlayer_plan(
    unsigned long long xmask, const unsigned long long* zmask, size_t terms, size_t n,
    unsigned* out) {
  if (!out || n > 40) return SIZE_MAX;
  if (xmask == 0) {
    const size_t k = qdc_pauli_layer_plan(zmask, terms, n, out);
    if (k == SIZE_MAX) return k;
    const unsigned v[6] = {out[0], ~0u, out[1], out[3], out[4], out[5]};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
    return k;
  }
  qdc::PxLayer P;
  if (qdc::pxl_make(xmask, zmask, nullptr, terms, n, P)) return SIZE_MAX;
  const qdc::PauliLayerPlan L = qdc::pl_plan(P.zr.data(), terms, P.lv);
  const unsigned v[6] = {qdc::pl_span_bits(P.lv), P.self ? ~0u : P.hb, L.groups, L.fwd, L.rev,
                         L.rev_grad};
  for (int i = 0; i < 6; ++i) out[i] = v[i];
  return L.groups;
}

// ---- sampling from |psi|^2 (include/qdc/sample.h, qdc_sample.hpp) ----------------------------

__attribute__((visibility("default"))) const char* qdc_sample(
    const qdc_complex* state, size_t n, const double* u, size_t shots, unsigned long long* out,
    double* norm2) {
  QDC_ABI_BEGIN
  if (n > 40) return qdc::fail("pos is out of the bound.");
  QDC_TRY(qdc::sample_check_uniforms(u, shots));
  if (shots > 0 && !out) return qdc::fail("The sample has no output buffers.");
  static qdc::SampleScratch scratch[qdc::ABI_MAX_DEVICES];  // guarded by the ABI mutex
  return qdc::sample(ctx, reinterpret_cast<const qdc::cx*>(state), (uint32_t)n, u, shots, out,
                     norm2, scratch[ctx.device]);
}

// host only: no context, no device
__attribute__((visibility("default"))) size_t qdc_sample_plan(size_t n, unsigned* out) {
  if (!out || n > 40) return SIZE_MAX;
  const qdc::SamplePlan P = qdc::sample_plan(n);
  const unsigned v[4] = {qdc::SAMPLE_G, (unsigned)P.segments, qdc::SAMPLE_SPAN,
                         (unsigned)P.segments};
  for (int i = 0; i < 4; ++i) out[i] = v[i];
  return (size_t)P.segments;
}

// host only: no context, no device
__attribute__((visibility("default"))) const char* qdc_sample_assign(
    const double* seg_sums, size_t segments, const double* u, size_t shots,
    unsigned long long* seg, double* resid, unsigned long long* perm, double* total) {
  return qdc::sample_assign(seg_sums, segments, u, shots, seg, resid, perm, total);
}

__attribute__((visibility("default"))) const char* qdc_abi_sync(void) {
  QDC_ABI_BEGIN
  QDC_HIP(hipStreamSynchronize(ctx.stream));
  return nullptr;
}

__attribute__((visibility("default"))) const char* qdc_abi_profile(int on) {
  QDC_ABI_BEGIN
  if (on) {
    QDC_HIP(hipStreamSynchronize(ctx.stream));
    ctx.prof.reset();
  }
  ctx.prof.on = on != 0;
  return nullptr;
}

__attribute__((visibility("default"))) size_t qdc_abi_profile_collect(qdc_kernel_stat* out,
                                                                      size_t cap) {
  std::lock_guard<std::mutex> lock(qdc::abi_mutex());
  qdc::Ctx* c = nullptr;
  if (qdc::abi_ctx(c)) return 0;
  return qdc::prof_collect(*c, out, cap);
}

}  // extern "C"

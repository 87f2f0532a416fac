/*
 * qdc/sample.h — bitstrings sampled from |psi|^2 by a two-pass inverse CDF over the state on
 * the device (csrc/qdc_sample.hpp).  Conventions of qdc/pauli.h: a state is a device buffer of
 * 2^n interleaved {re, im} amplitudes, every other pointer is HOST memory read or written before
 * the call returns, NULL = success, otherwise a library-owned message.
 *
 * For a state that need not be normalised, with p_i = re_i^2 + im_i^2 computed in double from
 * the stored amplitudes (both precisions), N = sum_i p_i and C_i = sum_{j <= i} p_j, a uniform
 * u in [0, 1) samples
 *     min { i : C_i > u * N }
 * (strict: u on a boundary goes to the upper index).  The sums are floating point, in fixed
 * orders; what every call guarantees:
 *   - the sampled index has p > 0 (u = 0 gives the first such index, a target at or past the
 *     last partial sum the last one);
 *   - C_{out-1} - tol <= u * N < C_out + tol, tol = (2^n + 4) * 2^-52 * N, against exact sums;
 *   - u[a] <= u[b] gives out[a] <= out[b] within one call;
 *   - the same call returns the same bits every time, and out[k] belongs to u[k].
 * The library holds no random generator: the caller supplies the uniforms.
 *
 * The state is cut into segments of 2^G amplitudes.  Pass A sums p over every segment; the host
 * prefix-sums the segment sums in long double, assigns every shot its segment and the residual
 * inside it, and orders the shots; pass B reads only the segments that were hit.
 *
 * Errors: "uniforms must be in [0, 1)." (a NaN, a negative value or one >= 1), "The state has
 * zero norm.", "The state is not finite." (N is inf or NaN; both only when shots > 0), "pos is
 * out of the bound." (n > 40), "The sample has no uniforms." / "The sample has no output
 * buffers." / "The sample has no segment sums." (NULL arguments that are needed).
 */
#ifndef QDC_SAMPLE_H
#define QDC_SAMPLE_H

#include <stddef.h>

#include "qdc/primitives.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[k] = the index sampled by u[k] (definition above); *norm2 = N when norm2 != NULL.
 * shots == 0 is a no-op that still returns N.  Two stream synchronisations. */
const char* qdc_sample(const qdc_complex* state, size_t n, const double* u, size_t shots,
                       unsigned long long* out, double* norm2);

/* Host only, no GPU: out[0..3] = {G, segments, amplitudes per span, locate blocks upper bound}.
 * Returns segments, SIZE_MAX for n > 40. */
size_t qdc_sample_plan(size_t n, unsigned* out);

/* Host only, no GPU: the step between the passes.  seg[k], resid[k] for every shot in the caller's
 * order, perm[] the processing order (segments ascending, residuals ascending within one), *total = N. */
const char* qdc_sample_assign(const double* seg_sums, size_t segments, const double* u, size_t shots,
                              unsigned long long* seg, double* resid, unsigned long long* perm,
                              double* total);

#ifdef __cplusplus
}
#endif

#endif /* QDC_SAMPLE_H */

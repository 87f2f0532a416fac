/*
 * qdc/overlap.h — overlaps and transition elements between two states, with their cotangent
 * (csrc/qdc_overlap.hpp).  Conventions of qdc/pauli.h: a state is a device buffer of 2^n
 * interleaved {re, im} amplitudes, every other pointer is HOST memory read before the call
 * returns, NULL = success, otherwise a library-owned message; a term is (coeff, xmask, zmask)
 * with (P psi)[i] = i^nY (-1)^popcount(j & z) psi[j], j = i ^ x, nY = popcount(x & z).
 *
 * With H = sum_t coeff[t] * P_t (real coefficients: H is Hermitian)
 *     o = <a|H|b> = sum_i conj(a[i]) (H b)[i],
 * a complex number; neither state need be normalised.  The plain overlap <a|b> is H = I.
 *
 * Cotangent.  In this library dL/dtheta = Re sum_i bwd[i] (dpsi/dtheta)[i] (qdc_pauli_rot_reverse;
 * qdc_pauli_inject's 2 w conj(H psi) is an instance).  For a real loss L of o = <t|H|psi>, the
 * target t a constant and psi the circuit's state, let g = dL/dRe o + i dL/dIm o.  Since
 * o = sum_j conj((H t)[j]) psi[j] is holomorphic in psi, dL = Re(conj(g) do) =
 * Re sum_j conj(g (H t)[j]) dpsi[j], and the injection is
 *     bwd (+)= conj(g * (H t)).
 * F = |o|^2 gives g = 2 o.  E = <psi|H|psi> with the bra frozen at a copy of psi gives g = 2 w:
 * the injection 2 w conj(H psi) that qdc_pauli_inject writes.
 *
 * Errors: "pos is out of the bound." (a mask bit at or above n), "The observable has no terms.",
 * "Pauli coefficients must be finite." (a non-finite coefficient or part of g), "fwd and bwd must
 * be different states." (src == bwd).  The same call returns the same bits every time; a reading
 * call synchronises the stream once per 32 launches.
 */
#ifndef QDC_OVERLAP_H
#define QDC_OVERLAP_H

#include <stddef.h>

#include "qdc/primitives.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[0] += Re <a|b>, out[1] += Im <a|b>; one pass over both states.  a == b is allowed. */
const char* qdc_overlap(const qdc_complex* a, const qdc_complex* b, size_t n, double out[2]);

/* out[0] += Re <a|H|b>, out[1] += Im <a|H|b>: one pass over both states for all the terms whose
 * partners lie inside a tile, one per far-reaching X/Y footprint (qdc_pauli_plan).  a == b is
 * allowed. */
const char* qdc_pauli_overlap(const qdc_complex* a, const qdc_complex* b,
                              const unsigned long long* xmask, const unsigned long long* zmask,
                              const double* coeff, size_t terms, size_t n, double out[2]);

/* bwd (+)= conj(g * src), g = g_re + i g_im; accumulate == 0 overwrites bwd (every amplitude,
 * without reading it). */
const char* qdc_overlap_inject(const qdc_complex* src, qdc_complex* bwd, size_t n, double g_re,
                               double g_im, int accumulate);

/* bwd (+)= conj(g * H src); accumulate as above. */
const char* qdc_pauli_overlap_inject(const qdc_complex* src, qdc_complex* bwd,
                                     const unsigned long long* xmask,
                                     const unsigned long long* zmask, const double* coeff,
                                     size_t terms, size_t n, double g_re, double g_im,
                                     int accumulate);

#ifdef __cplusplus
}
#endif

#endif /* QDC_OVERLAP_H */

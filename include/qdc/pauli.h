/*
 * qdc/pauli.h — Pauli-sum observables: the energy <psi|H|psi> of a weighted sum of Pauli
 * strings and its cotangent injection, each in a few passes over the state
 * (csrc/qdc_pauli.hpp).  Conventions of qdc/dense.h: a state is a device buffer of 2^n
 * interleaved {re, im} amplitudes, every other pointer is HOST memory read before the call
 * returns, NULL = success, otherwise a library-owned message.
 *
 * A term is (coeff, xmask, zmask): bit q of xmask = X or Y on qubit q, bit q of zmask = Z or Y
 * (both: Y = [[0,-i],[i,0]], neither: identity); qubit 0 is the least significant index bit.
 * With nY = popcount(x & z) and j = i ^ x:
 *     (P psi)[i] = i^nY * (-1)^popcount(j & z) * psi[j]
 * H = sum_t coeff[t] * P_t is Hermitian because the coefficients are real.
 *
 * Errors: "pos is out of the bound." (a mask bit at or above n), "The observable has no
 * terms.", "Pauli coefficients must be finite." (a non-finite coefficient or weight),
 * "fwd and bwd must be different states.".
 */
#ifndef QDC_PAULI_H
#define QDC_PAULI_H

#include <stddef.h>

#include "qdc/primitives.h"

#ifdef __cplusplus
extern "C" {
#endif

/* *energy += <state|H|state>, H = sum_t coeff[t] * P(xmask[t], zmask[t]).  The state need not
 * be normalised.  The same call returns the same bits every time. */
const char* qdc_pauli_energy(const qdc_complex* state, const unsigned long long* xmask,
                             const unsigned long long* zmask, const double* coeff,
                             size_t terms, size_t n, double* energy);

/* bwd (+)= 2 * weight * conj(H fwd); accumulate == 0 overwrites bwd (every amplitude, without
 * reading it).  The cotangent of `energy` with upstream weight dL/dE, in the convention of the
 * density route (conj_and_double, the transposed cotangent as a gate, add). */
const char* qdc_pauli_inject(const qdc_complex* fwd, qdc_complex* bwd,
                             const unsigned long long* xmask, const unsigned long long* zmask,
                             const double* coeff, size_t terms, size_t n, double weight,
                             int accumulate);

/* Host only, no GPU: the plan of the two calls above.  out[0..5] = {W (the tile width in
 * qubits), merged terms, window groups, far groups, energy launches, injection launches};
 * group_x[] (cap entries): the distinct x masks, window groups first, each class ascending.
 * Returns the number of groups, SIZE_MAX on invalid arguments or a too small cap. */
size_t qdc_pauli_plan(const unsigned long long* xmask, const unsigned long long* zmask,
                      size_t terms, size_t n, unsigned* out, unsigned long long* group_x,
                      size_t cap);

#ifdef __cplusplus
}
#endif

#endif /* QDC_PAULI_H */

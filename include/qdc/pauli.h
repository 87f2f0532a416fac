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

/* Pauli rotations (csrc/qdc_paulirot.hpp): R(theta; P) = exp(-i theta/2 P) = cos(theta/2) I -
 * i sin(theta/2) P for the string P(xmask, zmask), one pass over the state at any weight.
 * cos(theta/2) and sin(theta/2) are computed on the host in double and rounded once to the
 * build's precision.  xmask = zmask = 0 is the identity string: the global phase e^{-i theta/2}.
 * Errors: "pos is out of the bound.", "Pauli coefficients must be finite." (a non-finite
 * theta), "fwd and bwd must be different states.". */

/* state <- exp(-i theta/2 P(xmask, zmask)) state */
const char* qdc_pauli_rot(qdc_complex* state, unsigned long long xmask,
                          unsigned long long zmask, double theta, size_t n);

/* One reverse step of that gate, in one pass over both states:
 *   fwd <- R(-theta) fwd                      (uncompute)
 *   *dtheta += dL/dtheta                      (skipped when dtheta == NULL: a constant gate)
 *   bwd <- R(theta)^T bwd                     (pull-back)
 * with dL/dtheta = Re sum_i bwd[i] (dR/dtheta fwd_in)[i] = 1/2 Im sum_i bwd[i] (P fwd_out)[i]:
 * the gate-gradient convention of qdc_qkgrad (grad[r,c] = sum bwd[r] fwd_in[c]) chained to the
 * real angle, fwd_out the state the call receives and fwd_in the one it leaves, bwd the
 * cotangent at the gate's output.  The same call returns the same bits every time (one stream
 * synchronisation when dtheta != NULL).
 * bwd == NULL: only the uncompute (no cotangent yet); dtheta must then be NULL too. */
const char* qdc_pauli_rot_reverse(qdc_complex* fwd, qdc_complex* bwd, unsigned long long xmask,
                                  unsigned long long zmask, double theta, size_t n,
                                  double* dtheta);

/* Diagonal Pauli layers (csrc/qdc_paulilayer.hpp): K rotations about Z-only strings
 * P_k = Z^{zmask[k]} (any weight, zmask = 0 and duplicates allowed) in one pass over the state,
 *     U = exp(-i/2 sum_k theta[k] P_k),  (U psi)[i] = e^{-i phi(i)} psi[i],
 *     phi(i) = 1/2 sum_k theta[k] (-1)^popcount(i & zmask[k]),
 * the product of qdc_pauli_rot(theta[k], 0, zmask[k]) in any order.  The phase is summed exactly
 * in fixed point (theta / 4 pi rounded once to 2^-32 turns in f32, 2^-64 in f64).  A launch
 * carries 128 terms (32 when it reduces gradients); larger layers take several passes.
 * Errors: "The layer has no terms.", "pos is out of the bound.", "Pauli coefficients must be
 * finite." (a non-finite theta), "fwd and bwd must be different states."; for NULL arguments
 * "The layer has no masks.", "The layer has no angles." and "A gradient needs a bwd state."
 * (dtheta without bwd). */

/* state <- U state */
const char* qdc_pauli_layer(qdc_complex* state, const unsigned long long* zmask,
                            const double* theta, size_t terms, size_t n);

/* One reverse step, in one pass over both states: fwd <- e^{+i phi} fwd (uncompute), bwd <-
 * e^{-i phi} bwd (pull-back, U^T = U), dtheta[k] += dL/dtheta_k = 1/2 Im sum_i s_k(i) bwd[i] fwd[i]
 * for k < terms (qdc_pauli_rot_reverse's convention; one stream synchronisation for up to
 * 1024 terms, one more per further 1024).
 * bwd == NULL: uncompute only (dtheta must be NULL).  dtheta == NULL: constant layer.  The same
 * call returns the same bits every time. */
const char* qdc_pauli_layer_reverse(qdc_complex* fwd, qdc_complex* bwd,
                                    const unsigned long long* zmask, const double* theta,
                                    size_t terms, size_t n, double* dtheta);

/* Host only, no GPU: out[0..5] = {L (log2 of the amplitudes of a span), low-mask groups (distinct
 * zmask mod 2^L), terms with a high part (zmask >= 2^L), forward launches, reverse launches
 * without gradient, reverse launches with gradient}.  Returns the number of groups, SIZE_MAX on
 * invalid arguments. */
size_t qdc_pauli_layer_plan(const unsigned long long* zmask, size_t terms, size_t n,
                            unsigned* out);

/* Pauli layers with a shared X/Y footprint (csrc/qdc_paulixlayer.hpp): K rotations about the
 * strings P_k = (xmask, zmask[k]), one xmask for all of them, in one pass over the state,
 *     U = exp(-i/2 sum_k theta[k] P_k),
 * the product of qdc_pauli_rot(theta[k], xmask, zmask[k]) in any order.  The strings must commute:
 * every nY_k = popcount(xmask & zmask[k]) has one parity (a fermionic excitation under
 * Jordan-Wigner, an XX + YY hopping term).  Each pair of amplitudes (i, i ^ xmask) is rotated by
 * one angle, the diagonal layer's fixed-point phase on the pair's index: one sincos per pair.  A
 * launch carries 128 terms (32 when it reduces gradients).  xmask == 0 forwards to the diagonal
 * layer above, bit for bit.
 * Errors: those of the diagonal layer ("pos is out of the bound." for xmask too) and "The
 * strings of a layer must commute." (mixed parity of nY). */

/* state <- U state */
const char* qdc_pauli_xlayer(qdc_complex* state, unsigned long long xmask,
                             const unsigned long long* zmask, const double* theta, size_t terms,
                             size_t n);

/* One reverse step, in one pass over both states: fwd <- U(-theta) fwd (uncompute), bwd <-
 * U^T bwd (pull-back), dtheta[k] += dL/dtheta_k = 1/2 Im sum_i bwd[i] (P_k fwd)[i] for k < terms,
 * fwd and bwd as the call receives them (qdc_pauli_rot_reverse's convention; one stream
 * synchronisation for up to 1024 terms, one more per further 1024).
 * bwd == NULL: uncompute only (dtheta must be NULL).  dtheta == NULL: constant layer.  The same
 * call returns the same bits every time. */
const char* qdc_pauli_xlayer_reverse(qdc_complex* fwd, qdc_complex* bwd, unsigned long long xmask,
                                     const unsigned long long* zmask, const double* theta,
                                     size_t terms, size_t n, double* dtheta);

/* Host only, no GPU: out[0..5] = {L (log2 of the pair indices of a span: the diagonal layer's L,
 * one less in the self-paired form), the deleted bit (the highest set bit of xmask; 0xffffffff
 * where nothing is deleted from the masks' layout: xmask == 0, and the self-paired form, f32 at
 * xmask == 1, which drops bit 0), low-mask groups of the reduced masks, forward launches, reverse
 * launches without gradient, reverse launches with gradient}.  Returns the number of groups,
 * SIZE_MAX on invalid arguments (non-commuting strings among them). */
size_t qdc_pauli_xlayer_plan(unsigned long long xmask, const unsigned long long* zmask,
                             size_t terms, size_t n, unsigned* out);

#ifdef __cplusplus
}
#endif

#endif /* QDC_PAULI_H */

"""Pauli-sum observables: ``H = sum_t c_t P_t`` with real ``c_t`` and Pauli strings ``P_t``.

A ``PauliSum`` holds the terms as the masks of ``include/qdc/pauli.h``: bit q of ``xmask`` means
X or Y on qubit q, bit q of ``zmask`` means Z or Y (both: Y = [[0, -i], [i, 0]], neither: the
identity); qubit 0 is the least significant bit of an amplitude's index.  With
``nY = popcount(x & z)`` and ``j = i ^ x``::

    (P psi)[i] = i^nY * (-1)^popcount(j & z) * psi[j]

``QuantizedTensor.pauli_energy(obs)`` returns ``<psi|H|psi>`` and ``pauli_inject(fwd, bwd, obs,
weight)`` its cotangent ``bwd (+)= 2 weight conj(H fwd)``, each in one pass over the state for
every group of terms that fits a tile plus one pass per far-reaching X/Y footprint
(``csrc/qdc_pauli.hpp``); ``DenseCircuit.get_observable_op[_with_grad]`` puts both into a
differentiable circuit.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from ._native import PanicException

_OP = re.compile(r"^([XYZxyz])(\d+)$")


def _parse_ops(ops):
    """``"X0 Y3 Z12"`` or a sequence of ``(qubit, "X"|"Y"|"Z")`` -> [(qubit, letter)]."""
    if isinstance(ops, str):
        out = []
        for tok in ops.split():
            m = _OP.match(tok)
            if not m:
                raise ValueError(f"cannot read the Pauli operator {tok!r} (expected e.g. 'X0 Y3 Z12')")
            out.append((int(m.group(2)), m.group(1).upper()))
        return out
    out = []
    for q, p in ops:
        p = str(p).upper()
        if p not in ("X", "Y", "Z"):
            raise ValueError(f"a Pauli operator is 'X', 'Y' or 'Z', got {p!r}")
        out.append((int(q), p))
    return out


def _real_coeff(c):
    c = complex(c)
    if c.imag != 0.0:
        raise PanicException("Pauli coefficients must be real.")
    if not np.isfinite(c.real):
        raise PanicException("Pauli coefficients must be finite.")
    return c.real


def pauli_masks(qubits_number: int, ops):
    """``(xmask, zmask)`` of one Pauli string on ``qubits_number`` qubits: ``ops`` is a string
    such as ``"X0 Y3 Z12"`` (``""`` is the identity) or a sequence of ``(qubit, "X"|"Y"|"Z")``."""
    n = int(qubits_number)
    x = z = 0
    for q, p in _parse_ops(ops):
        if q < 0 or q >= n:
            raise PanicException("pos is out of the bound.")
        bit = 1 << q
        if (x | z) & bit:
            raise PanicException("a qubit appears twice in a Pauli term.")
        if p in ("X", "Y"):
            x |= bit
        if p in ("Z", "Y"):
            z |= bit
    return x, z


class PauliSum:
    """``PauliSum(qubits_number, [(coeff, ops), ...])``: ``ops`` is a string such as
    ``"X0 Y3 Z12"`` (``""`` is the identity) or a sequence of ``(qubit, "X"|"Y"|"Z")``.  Terms
    with the same string merge (their coefficients add); the terms are kept sorted by
    ``(xmask, zmask)``."""

    def __init__(self, qubits_number: int, terms):
        n = int(qubits_number)
        merged = {}
        for coeff, ops in terms:
            c = _real_coeff(coeff)
            key = pauli_masks(n, ops)
            merged[key] = merged.get(key, 0.0) + c
        self._set(n, merged)

    @classmethod
    def from_masks(cls, qubits_number, coeffs, xmasks, zmasks):
        n = int(qubits_number)
        coeffs, xmasks, zmasks = list(coeffs), list(xmasks), list(zmasks)
        if not len(coeffs) == len(xmasks) == len(zmasks):
            raise ValueError("coeffs, xmasks and zmasks must have one entry per term")
        merged = {}
        for c, x, z in zip(coeffs, xmasks, zmasks):
            x, z = int(x), int(z)
            if x < 0 or z < 0 or (x | z) >> n:
                raise PanicException("pos is out of the bound.")
            merged[(x, z)] = merged.get((x, z), 0.0) + _real_coeff(c)
        self = cls.__new__(cls)
        self._set(n, merged)
        return self

    def _set(self, n, merged):
        if n < 0 or n > 40:
            raise PanicException(f"qubits_number {n} is out of the supported range (<= 40).")
        keys = sorted(merged)
        self.qubits_number = n
        self.xmasks = np.array([k[0] for k in keys], dtype=np.uint64)
        self.zmasks = np.array([k[1] for k in keys], dtype=np.uint64)
        self.coeffs = np.array([merged[k] for k in keys], dtype=np.float64)

    def __len__(self):
        return int(self.coeffs.size)

    def terms(self):
        """[(coeff, xmask, zmask)], sorted by (xmask, zmask)."""
        return [(float(c), int(x), int(z)) for c, x, z in zip(self.coeffs, self.xmasks, self.zmasks)]

    def _args(self):
        """(xmask*, zmask*, coeff*, terms) of the C entry points (the arrays stay owned here)."""
        ull = C.POINTER(C.c_ulonglong)
        return (self.xmasks.ctypes.data_as(ull), self.zmasks.ctypes.data_as(ull),
                self.coeffs.ctypes.data_as(C.POINTER(C.c_double)), len(self))

    def apply(self, psi):
        """``H psi`` on the host in complex128, by the index rule of the definition."""
        psi = np.asarray(psi, dtype=np.complex128).reshape(-1)
        if psi.size != 1 << self.qubits_number:
            raise PanicException("Size of the given state does not match the size of the tensor.")
        idx = np.arange(psi.size, dtype=np.uint64)
        out = np.zeros_like(psi)
        for c, x, z in self.terms():
            j = idx ^ np.uint64(x)
            sign = 1.0 - 2.0 * (_popcount(j & np.uint64(z)) & 1)
            out += (c * 1j ** (bin(x & z).count("1") % 4)) * sign * psi[j]
        return out

    def to_matrix(self):
        """The dense 2^n x 2^n matrix (complex128), n <= 12."""
        n = self.qubits_number
        if n > 12:
            raise PanicException("to_matrix() is for at most 12 qubits.")
        dim = 1 << n
        idx = np.arange(dim, dtype=np.uint64)
        m = np.zeros((dim, dim), dtype=np.complex128)
        for c, x, z in self.terms():
            j = idx ^ np.uint64(x)
            sign = 1.0 - 2.0 * (_popcount(j & np.uint64(z)) & 1)
            m[idx, j] += (c * 1j ** (bin(x & z).count("1") % 4)) * sign
        return m


def _popcount(a):
    a = a.astype(np.uint64)
    count = np.zeros(a.shape, dtype=np.int64)
    while a.any():
        count += (a & np.uint64(1)).astype(np.int64)
        a = a >> np.uint64(1)
    return count


def plan(obs: PauliSum, precision=None):
    """The launch plan of ``pauli_energy`` / ``pauli_inject`` (qdc_pauli_plan, host only):
    ``{"W", "merged", "window_groups", "far_groups", "energy_launches", "inject_launches",
    "group_x"}``."""
    return plan_masks(obs.qubits_number, obs.xmasks, obs.zmasks, precision)


def plan_masks(qubits_number, xmasks, zmasks, precision=None):
    """``plan`` on raw masks (duplicates allowed); None where the library rejects them."""
    from ._native import default_precision, load
    lib = load(precision or default_precision())
    xs = np.ascontiguousarray(xmasks, dtype=np.uint64)
    zs = np.ascontiguousarray(zmasks, dtype=np.uint64)
    ull = C.POINTER(C.c_ulonglong)
    out = (C.c_uint * 6)()
    cap = max(1, xs.size)
    gx = (C.c_ulonglong * cap)()
    k = lib.qdc_pauli_plan(xs.ctypes.data_as(ull), zs.ctypes.data_as(ull), xs.size,
                           int(qubits_number), out, gx, cap)
    if k == C.c_size_t(-1).value:
        return None
    return {"W": out[0], "merged": out[1], "window_groups": out[2], "far_groups": out[3],
            "energy_launches": out[4], "inject_launches": out[5],
            "group_x": [int(gx[i]) for i in range(k)]}


def layer_masks(qubits_number: int, strings):
    """The zmasks (uint64 array) of a diagonal Pauli layer: ``strings`` is a sequence of Pauli
    strings in the forms ``pauli_masks`` accepts, Z letters only; a uint64 array is taken as the
    masks themselves (the library checks their range)."""
    if isinstance(strings, np.ndarray) and strings.dtype == np.uint64 and strings.ndim == 1:
        return np.ascontiguousarray(strings)
    if isinstance(strings, str):
        raise PanicException("a Pauli layer takes a sequence of strings.")
    zs = []
    for ops in strings:
        x, z = pauli_masks(qubits_number, ops)
        if x:
            raise PanicException("a Pauli layer takes Z strings only.")
        zs.append(z)
    return np.array(zs, dtype=np.uint64)


def layer_angles(thetas, count):
    """The angles of a layer of ``count`` strings: a real 1-D float64 array of that length."""
    t = np.asarray(thetas)
    if t.ndim != 1 or t.size != count:
        raise PanicException("a Pauli layer takes one angle per string.")
    if np.iscomplexobj(t):
        if np.any(t.imag != 0.0):
            raise PanicException("A rotation angle must be real.")
        t = t.real
    return np.ascontiguousarray(t, dtype=np.float64)


def pauli_layer_plan(qubits_number, strings, precision=None):
    """The launch plan of a diagonal Pauli layer (qdc_pauli_layer_plan, host only): ``{"L",
    "groups", "high_terms", "forward_launches", "reverse_launches", "reverse_grad_launches"}``;
    ``strings`` as for ``apply_pauli_layer``, or an integer array of zmasks.  None where the
    library rejects the masks."""
    from ._native import default_precision, load
    lib = load(precision or default_precision())
    if isinstance(strings, np.ndarray) and strings.dtype.kind in "iu":
        zs = np.ascontiguousarray(strings, dtype=np.uint64)
    else:
        zs = layer_masks(qubits_number, strings)
    out = (C.c_uint * 6)()
    k = lib.qdc_pauli_layer_plan(zs.ctypes.data_as(C.POINTER(C.c_ulonglong)), zs.size,
                                 int(qubits_number), out)
    if k == C.c_size_t(-1).value:
        return None
    return {"L": out[0], "groups": out[1], "high_terms": out[2], "forward_launches": out[3],
            "reverse_launches": out[4], "reverse_grad_launches": out[5]}


def _commute_check(x, zs):
    """Strings (x, z_k) with one x commute iff every nY_k = popcount(x & z_k) has one parity."""
    par = {bin(x & int(z)).count("1") & 1 for z in zs}
    if len(par) > 1:
        raise PanicException("The strings of a layer must commute.")


def xlayer_masks(qubits_number: int, strings):
    """``(xmask, zmasks)`` of a Pauli layer whose strings share their X/Y positions and commute
    (``apply_pauli_xlayer``): ``strings`` is a sequence of Pauli strings in the forms
    ``pauli_masks`` accepts; a pair ``(xmask, uint64 array of zmasks)`` is taken as the masks
    themselves (the library checks them)."""
    if isinstance(strings, tuple) and len(strings) == 2 and isinstance(strings[1], np.ndarray) \
            and strings[1].dtype == np.uint64 and strings[1].ndim == 1:
        return int(strings[0]), np.ascontiguousarray(strings[1])
    if isinstance(strings, str):
        raise PanicException("a Pauli layer takes a sequence of strings.")
    x, zs = None, []
    for ops in strings:
        xk, zk = pauli_masks(qubits_number, ops)
        if x is not None and xk != x:
            raise PanicException("The strings of a layer must share their X/Y positions.")
        x = xk
        zs.append(zk)
    _commute_check(x or 0, zs)
    return x or 0, np.array(zs, dtype=np.uint64)


def xevolution_masks(h: PauliSum):
    """``(xmask, zmasks, coeffs)`` of a ``PauliSum`` whose terms share their X/Y positions and
    commute (``add_var_pauli_xevolution``)."""
    if np.any(h.xmasks != h.xmasks[0]):
        raise PanicException("The strings of a layer must share their X/Y positions.")
    x = int(h.xmasks[0])
    _commute_check(x, h.zmasks)
    return x, h.zmasks.copy(), h.coeffs.copy()


def pauli_xlayer_plan(qubits_number, strings, precision=None):
    """The launch plan of a shared-footprint Pauli layer (qdc_pauli_xlayer_plan, host only):
    ``{"L", "deleted_bit", "groups", "forward_launches", "reverse_launches",
    "reverse_grad_launches"}``; ``deleted_bit`` is None for the diagonal (x = 0) and the
    self-paired (f32, x = 1) forms.  ``strings`` as for ``apply_pauli_xlayer``.  None where the
    library rejects the masks."""
    from ._native import default_precision, load
    lib = load(precision or default_precision())
    x, zs = xlayer_masks(qubits_number, strings)
    out = (C.c_uint * 6)()
    k = lib.qdc_pauli_xlayer_plan(x, zs.ctypes.data_as(C.POINTER(C.c_ulonglong)), zs.size,
                                  int(qubits_number), out)
    if k == C.c_size_t(-1).value:
        return None
    return {"L": out[0], "deleted_bit": None if out[1] == 0xffffffff else out[1],
            "groups": out[2], "forward_launches": out[3], "reverse_launches": out[4],
            "reverse_grad_launches": out[5]}


def _string_mul(a, b):
    """(phase, (x, z)) of the product of two strings: with W(x, z) = X^x Z^z the string is
    P = i^nY W, and W(x1, z1) W(x2, z2) = (-1)^popcount(z1 & x2) W(x1 ^ x2, z1 ^ z2)."""
    (x1, z1), (x2, z2) = a, b
    x, z = x1 ^ x2, z1 ^ z2
    ny = bin(x1 & z1).count("1") + bin(x2 & z2).count("1") - bin(x & z).count("1")
    return 1j ** (ny % 4) * (-1) ** (bin(z1 & x2).count("1") & 1), (x, z)


def ladder_terms(qubits_number: int, ops):
    """The product of Jordan-Wigner ladder operators as ``{(xmask, zmask): complex}``: ``ops`` is a
    sequence of ``(mode, dagger)``, leftmost factor first, with
    ``a_q = (prod_{r<q} Z_r) (X_q + i Y_q) / 2`` (qubit value 1 = occupied) and ``a_q^dagger`` its
    adjoint.  Terms whose coefficients cancel are dropped."""
    n = int(qubits_number)
    out = {(0, 0): 1.0 + 0.0j}
    for q, dagger in ops:
        q = int(q)
        if q < 0 or q >= n:
            raise PanicException("pos is out of the bound.")
        bit, low = 1 << q, (1 << q) - 1
        factor = {(bit, low): 0.5, (bit, low | bit): -0.5j if dagger else 0.5j}
        nxt = {}
        for ka, ca in out.items():
            for kb, cb in factor.items():
                ph, key = _string_mul(ka, kb)
                nxt[key] = nxt.get(key, 0.0) + ca * cb * ph
        out = {k: c for k, c in nxt.items() if c != 0}
    return out


def excitation(qubits_number: int, occ, virt) -> PauliSum:
    """The generator ``G = i (tau - tau^dagger)`` of a fermionic excitation under Jordan-Wigner,
    ``tau = prod_{p in virt} a_p^dagger prod_{q in occ} a_q`` (``ladder_terms``): 2 / 8 / 32
    strings for a single / double / triple excitation, with one X/Y footprint, all commuting.
    ``exp(-i theta/2 G) = exp(theta/2 (tau - tau^dagger))``."""
    occ, virt = [int(q) for q in occ], [int(p) for p in virt]
    if len(occ) != len(virt) or not 1 <= len(occ) <= 3:
        raise PanicException("an excitation takes 1, 2 or 3 occupied and as many virtual modes.")
    if len(set(occ + virt)) != len(occ) + len(virt):
        raise PanicException("positions must be different.")
    tau = ladder_terms(qubits_number, [(p, True) for p in virt] + [(q, False) for q in occ])
    # tau^dagger has the conjugate coefficients: i (c - conj c) = -2 Im c
    terms = [(k, -2.0 * c.imag) for k, c in tau.items() if c.imag != 0.0]
    return PauliSum.from_masks(qubits_number, [c for _, c in terms], [k[0] for k, _ in terms],
                               [k[1] for k, _ in terms])

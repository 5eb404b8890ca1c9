// The positional encoding e(x) = [x, sin(2^k x), cos(2^k x)]_k of one point (models/embedder.py:40-46) and its derivatives,
// written once: every kernel that encodes a point, or applies J_pe, J_pe^T or the second derivative, calls these (device only).
//
// Column of sin(2^k x_d): 3 + 6 k + d; the cosine's is 3 columns further; the three columns in front are x itself and stay
// with the caller.  Every operation takes (k0, kstep): it walks the octaves k = k0, k0 + kstep, ... < multires, so that the
// threads of a point can share them.  `x` (and g, v, ge, nt) is anything indexable by d = 0..2, an array or a pointer: a
// pointer is read where it is used, octave by octave, an array once by the caller.
// The floating-point statements are kept as they are (these units compile with contraction on, and the compiler contracts
// per expression): a kernel's bits depend on them.
#pragma once
#include <hip/hip_runtime.h>

namespace rnb {

// The one frequency loop: fn(c, d, f, sin(f x_d), cos(f x_d)) with f = 2^k and c = 3 + 6 k, the sine column of d = 0.
template <class X, class Fn>
__device__ __forceinline__ void pe_octaves(const X& x, int multires, int k0, int kstep, Fn fn) {
  for (int k = k0; k < multires; k += kstep) {
    const float f = (float)(1 << k);
    const int c = 3 + 6 * k;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      float s, co;
      sincosf(x[d] * f, &s, &co);
      fn(c, d, f, s, co);
    }
  }
}

// Encode: put(c, sin, cos) gets the sine's column c = 3 + 6 k + d; the cosine's is c + 3.
template <class X, class Put>
__device__ __forceinline__ void pe_sincos(const X& x, int multires, int k0, int kstep, Put put) {
  pe_octaves(x, multires, k0, kstep, [&](int c, int d, float, float s, float co) { put(c + d, s, co); });
}

// Adjoint: t += J_pe(x)^T g over the walked octaves (g: the adjoint of the encoding, column 0 = x's own).
template <class X, class G>
__device__ __forceinline__ void pe_adjoint(const X& x, const G& g, int multires, int k0, int kstep, float (&t)[3]) {
  pe_octaves(x, multires, k0, kstep, [&](int c, int d, float f, float s, float co) { t[d] += f * (g[c + d] * co - g[c + 3 + d] * s); });
}

// Tangent: the columns of J_pe(x) v: put(c, o_c, o_{c+3}) gets the sine's column c = 3 + 6 k + d and both values.
template <class X, class V, class Put>
__device__ __forceinline__ void pe_tangent(const X& x, const V& v, int multires, int k0, int kstep, Put put) {
  pe_octaves(x, multires, k0, kstep, [&](int c, int d, float f, float s, float co) {
    const float v0 = f * co * v[d], v1 = -f * s * v[d];
    put(c + d, v0, v1);
  });
}

// Adjoint with the Hessian term: acc += J_pe(x)^T g + sum_k ge_k d^2 pe_k / d x^2 . nt, octave by octave and coordinate by
// coordinate in this order.  The second derivative is diagonal: d^2 sin(f x) = -f^2 sin(f x), d^2 cos(f x) = -f^2 cos(f x).
// hess == false: the first term alone (ge and nt are not read).
template <class X, class G, class GE, class NT>
__device__ __forceinline__ void pe_adjoint_hess(const X& x, const G& g, bool hess, const GE& ge, const NT& nt, int multires,
                                                int k0, int kstep, float (&acc)[3]) {
  pe_octaves(x, multires, k0, kstep, [&](int c, int d, float f, float s, float co) {
    acc[d] += f * (g[c + d] * co - g[c + 3 + d] * s);
    if (hess) acc[d] -= f * f * (ge[c + d] * s + ge[c + 3 + d] * co) * nt[d];
  });
}

}  // namespace rnb

// The first hit of ONE ray with a binned triangle mesh, as a device function: the pair test and the walk that
// rnb_mesh_raycast (mesh_raycast.hip) and rnb_mesh_view_votes (mesh_cull.hip) share.  Written once, so that a segment
// cast by the votes kernel gives the bits `MeshIndex.visible` gives.  A file that includes this header must be compiled
// with -ffp-contract=off: every product and difference rounds on its own, as tests/mesh_raycast_ref.py evaluates them.
//
// THE PAIR TEST is the watertight one of Woop, Benthin and Wald (JCGT 2013) in fp64, rc_visit below, a pure function of
// the ray and the three corners: kz = the first largest |d|, (kx, ky) the next two axes cyclically, swapped when
// d[kz] < 0; corners translated by -o and sheared, A' = (A[kx] - Sx A[kz], A[ky] - Sy A[kz]); edge functions
// U = C'x B'y - C'y B'x, V = A'x C'y - A'y C'x, W = B'x A'y - B'y A'x; a hit when none is negative or none is positive
// (ZERO COUNTS AS INSIDE), det = (U + V) + W != 0 and t = ((U Az + V Bz) + W Cz) / det lies in [t_min, t_max].  Two
// products of the same four numbers in the other order round to the same value, so an edge shared by two triangles
// gives both the same edge function up to sign: a ray cannot slip between them.  The result of a ray is the minimum
// under (t as computed, triangle index) over every triangle tested, and testing a triangle twice gives the same bits.
//
// THE WALK goes by layers of cells along the major axis m = kz, in the ray's direction.  With
//     S   = |grid| + max |o|      (|grid| = max |origin| + max dim x cell, the magnitude of every coordinate in the box)
//     pad = 4096 x 2^-52 x S      and      tau = pad / |d_m|   (pad as a ray parameter)
// layer i stands for the m-coordinates [plane(i) - pad, plane(i + 1) + pad], plane(k) = origin + k cell.  Its parameter
// interval [ta, tb] is cut to [t_min - tau, t_max + tau]; the other two coordinates u, v are evaluated at ta and at tb,
// the interval between the two values is widened by pad and mapped to cells with the clamped, monotone mesh_cell of
// mesh_common.hip.h.  |d_u|, |d_v| <= |d_m|: the ray moves at most one cell sideways per layer, so a layer costs
// at most 2 cells per axis, 3 where the widening crosses a face.  Every entry of those cells is tested.
//
// WHY NO HIT IS SKIPPED.  Take a hit as the pair test computes it and let l = (U, V, W) / det as real numbers: l >= 0,
// sum 1, so P = l0 A + l1 B + l2 C is a point of the triangle, inside its box.  The triangle is entered in the cell
// (mesh_cell(P_m), mesh_cell(P_u), mesh_cell(P_v)), because its cell range per axis is that of its box and mesh_cell is
// monotone.
//   * Along m: t is the l-weighted mean of Az = fl(Sz fl(A_m - o_m)) and its kin up to the rounding of three products,
//     two sums and a division, so o_m + t d_m = P_m up to 16 x 2^-52 S, and t* = (P_m - o_m) / d_m is within
//     16 x 2^-52 S / |d_m| of t.  mesh_cell(x) = i implies plane(i) - slack <= x <= plane(i + 1) + slack with
//     slack = 2^-48 |grid| (mesh_eval.hip shows it), so t* lies in the interval of layer i = mesh_cell(P_m), and inside
//     [t_min - tau, t_max + tau] because t is inside [t_min, t_max].
//   * Across: P_u - (o_u + t* d_u) = sum of l_k x (the exact sheared x of corner k) = sum of l_k A'_k,x + 8 x 2^-52 S,
//     and sum of l_k A'_k = (eU A' + eV B' + eW C') / det, where eU .. are the rounding errors of the computed edge
//     functions (with exact ones the sum is the zero vector): at most 3 x 2^-52 r^3 / |det| for corners within r of
//     the ray.  For |det| >= r^3 / (1024 S) — every triangle that is not seen edge-on to within its size over 1024
//     scene sizes — this is below 3072 x 2^-52 S; all of it stays below pad.  u is linear in t, so o_u + t* d_u lies
//     between the values at ta and tb, and P_u inside the widened interval: the cells tested include P's.
//   A hit outside that bound is one whose point sum of bary_k x corner_k is more than pad away from o + t d: the pair
//   test returns it for what it is, the walk does not promise to find it.  The extreme case is a triangle of zero area
//   with three distinct, collinear corners under a ray through its segment: its edge functions are rounding noise.
//   (With two equal corners one edge function is exactly 0 and the other two exactly opposite: det == 0, never a hit.)
//   * The box: with RNB_MESH_BINS_COVER every binned triangle, P with it, lies inside the grid's box up to slack, so a
//     layer whose widened u or v interval misses the box widened by pad holds no hit, and rays that start beyond the
//     box or point away from it test nothing.  Without the flag a triangle outside the box sits in a boundary cell far
//     from where the ray meets it: the call is refused.
//   * The stop: layers are visited in the order of their entry parameter.  A hit in the layer at hand or a later one
//     has t >= ta - tau, so when ta - tau > the best t so far, strictly, nothing nearer and nothing equal is left: a
//     tie is always evaluated and goes to the smaller index.
//
// WHY IT CANNOT HANG OR READ OUT OF BOUNDS.  The layer loop runs over a clamped range of [0, dim_m), the cell loops
// over clamped ranges of [0, dim_u) x [0, dim_v), the entry loop over [cell_start[c], cell_start[c + 1]) cut to
// [0, E), and a triangle index outside [0, T) is passed over: every trip count is fixed by the dims and E before its
// loop starts, and every index is clamped before it is used, whatever the arithmetic in front of it produced (mesh_cell
// maps NaN to cell 0).  A ray with a non-finite origin or direction, a zero direction or a NaN bound leaves before the walk.
#pragma once
#include "mesh_common.hip.h"

namespace rnb {

constexpr double kRcPad = 9.094947017729282e-13;   // 4096 x 2^-52 = 2^-40

// what the pair test needs of a ray: the axis permutation, the translated origin, the shear
struct RcRay {
  int kx, ky, kz;
  double ox, oy, oz;   // o[kx], o[ky], o[kz]
  double Sx, Sy, Sz;
  double t_min, t_max;
};

struct RcBest {
  double t;
  int tri;
  double U, V, W, det;
};

template <class T>
__device__ inline T rc_pick(T a0, T a1, T a2, int k) { return k == 0 ? a0 : (k == 1 ? a1 : a2); }

// every entry of cell c against the ray: tests/mesh_raycast_ref.py's ray_triangle, operation for operation
__device__ inline void rc_visit(const BinnedMesh& a, const RcRay& r, int64_t c, RcBest& best) {
  unsigned long long s = a.cell_start[c], e = a.cell_start[c + 1];
  if (e > (unsigned long long)a.E) e = (unsigned long long)a.E;
  for (; s < e; ++s) {
    const int tri = a.entries[s];
    if (tri < 0 || tri >= a.T) continue;
    const double* __restrict__ p = a.corners + (int64_t)tri * 9;
    const double Akz = p[r.kz] - r.oz, Bkz = p[3 + r.kz] - r.oz, Ckz = p[6 + r.kz] - r.oz;
    const double Ax = (p[r.kx] - r.ox) - r.Sx * Akz, Ay = (p[r.ky] - r.oy) - r.Sy * Akz;
    const double Bx = (p[3 + r.kx] - r.ox) - r.Sx * Bkz, By = (p[3 + r.ky] - r.oy) - r.Sy * Bkz;
    const double Cx = (p[6 + r.kx] - r.ox) - r.Sx * Ckz, Cy = (p[6 + r.ky] - r.oy) - r.Sy * Ckz;
    const double U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    if (!((U >= 0.0 && V >= 0.0 && W >= 0.0) || (U <= 0.0 && V <= 0.0 && W <= 0.0))) continue;
    const double det = (U + V) + W;
    if (det == 0.0) continue;
    const double Az = r.Sz * Akz, Bz = r.Sz * Bkz, Cz = r.Sz * Ckz;
    const double t = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(t >= r.t_min && t <= r.t_max)) continue;
    if (t < best.t || (t == best.t && tri < best.tri)) {
      best.t = t;
      best.tri = tri;
      best.U = U; best.V = V; best.W = W; best.det = det;
    }
  }
}

// The first hit of the ray o + t d, t_min <= t <= t_max, with the mesh: best.t = +inf and best.tri = -1 when nothing is
// met (always so with E == 0), best.t = NaN for a ray that cannot be cast (a non-finite origin or direction, a zero
// direction, a NaN bound).
__device__ inline RcBest rc_first_hit(const BinnedMesh& a, double o0, double o1, double o2, double d0, double d1, double d2,
                                      double t_min, double t_max) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
  RcRay r;
  r.t_min = t_min;
  r.t_max = t_max;
  RcBest best;
  best.t = inf;
  best.tri = -1;
  best.U = best.V = best.W = best.det = nan;
  const bool valid = mesh_finite(o0) && mesh_finite(o1) && mesh_finite(o2) && mesh_finite(d0) && mesh_finite(d1) && mesh_finite(d2) &&
                     (d0 != 0.0 || d1 != 0.0 || d2 != 0.0) && r.t_min == r.t_min && r.t_max == r.t_max;
  if (!valid) {
    best.t = nan;
  } else if (a.E > 0) {
    const double a0 = fabs(d0), a1 = fabs(d1), a2 = fabs(d2);
    int kz = 0;
    if (a1 > a0) kz = 1;
    if (a2 > fmax(a0, a1)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const double dm = rc_pick(d0, d1, d2, kz);
    if (dm < 0.0) {
      const int k = kx;
      kx = ky;
      ky = k;
    }
    const double du = rc_pick(d0, d1, d2, kx), dv = rc_pick(d0, d1, d2, ky);
    r.kx = kx; r.ky = ky; r.kz = kz;
    r.ox = rc_pick(o0, o1, o2, kx); r.oy = rc_pick(o0, o1, o2, ky); r.oz = rc_pick(o0, o1, o2, kz);
    r.Sx = du / dm; r.Sy = dv / dm; r.Sz = 1.0 / dm;
    // the grid along (u, v, m) = (kx, ky, kz)
    const double gu = rc_pick(a.g.o[0], a.g.o[1], a.g.o[2], kx), gv = rc_pick(a.g.o[0], a.g.o[1], a.g.o[2], ky),
                 gm = rc_pick(a.g.o[0], a.g.o[1], a.g.o[2], kz);
    const int nu = rc_pick(a.g.d[0], a.g.d[1], a.g.d[2], kx), nv = rc_pick(a.g.d[0], a.g.d[1], a.g.d[2], ky),
              nm = rc_pick(a.g.d[0], a.g.d[1], a.g.d[2], kz);
    const int64_t st1 = a.g.d[0], st2 = (int64_t)a.g.d[0] * a.g.d[1];
    const int64_t su = rc_pick((int64_t)1, st1, st2, kx), sv = rc_pick((int64_t)1, st1, st2, ky), sm = rc_pick((int64_t)1, st1, st2, kz);
    const double cell = a.g.cell, pad = (a.g.mag + fmax(fabs(o0), fmax(fabs(o1), fabs(o2)))) * kRcPad;
    const double tau = pad * fabs(r.Sz);
    const double tlo = r.t_min - tau, thi = r.t_max + tau;
    const double ulo_box = gu - pad, uhi_box = (gu + (double)nu * cell) + pad;
    const double vlo_box = gv - pad, vhi_box = (gv + (double)nv * cell) + pad;
    const bool up = dm > 0.0;
    // the layers the cut parameter range can reach (the cut inside the loop is what decides; this only shortens it)
    const double m_first = r.oz + tlo * dm, m_last = r.oz + thi * dm;
    const int first = mesh_cell(up ? m_first - 2.0 * pad : m_first + 2.0 * pad, gm, cell, nm);
    const int last = mesh_cell(up ? m_last + 2.0 * pad : m_last - 2.0 * pad, gm, cell, nm);
    const int step = up ? 1 : -1;
    const int trips = (last - first) * step + 1;              // <= nm; none when the range is behind the ray
    for (int k = 0, layer = first; k < trips; ++k, layer += step) {
      const double p0 = (gm + (double)layer * cell) - pad, p1 = (gm + (double)(layer + 1) * cell) + pad;
      double ta = ((up ? p0 : p1) - r.oz) * r.Sz, tb = ((up ? p1 : p0) - r.oz) * r.Sz;
      if (ta - tau > best.t) break;
      ta = fmax(ta, tlo);
      tb = fmin(tb, thi);
      if (!(ta <= tb)) continue;
      const double ua = r.ox + ta * du, ub = r.ox + tb * du, va = r.oy + ta * dv, vb = r.oy + tb * dv;
      const double ulo = fmin(ua, ub) - pad, uhi = fmax(ua, ub) + pad, vlo = fmin(va, vb) - pad, vhi = fmax(va, vb) + pad;
      if (uhi < ulo_box || ulo > uhi_box || vhi < vlo_box || vlo > vhi_box) continue;
      const int cu0 = mesh_cell(ulo, gu, cell, nu), cu1 = mesh_cell(uhi, gu, cell, nu);
      const int cv0 = mesh_cell(vlo, gv, cell, nv), cv1 = mesh_cell(vhi, gv, cell, nv);
      for (int cv = cv0; cv <= cv1; ++cv)
        for (int cu = cu0; cu <= cu1; ++cu) rc_visit(a, r, (int64_t)layer * sm + (int64_t)cv * sv + (int64_t)cu * su, best);
    }
  }
  return best;
}

}  // namespace rnb

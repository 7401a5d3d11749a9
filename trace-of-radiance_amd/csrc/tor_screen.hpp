// tor_screen.hpp -- the conservative FMA screen of the strict float64 object loop (integrate_kernel variants ARITH 2).
// One source for the device (tor_kernels.hip) and the host self test (tor_selftest_screen_host, tests/test_screen.py).
#pragma once
#include "tor_math.hpp"

namespace tor {

// ARITH 2 -- the reference's results behind a conservative FMA SCREEN.  The wave-uniform object loop only decides which
// objects become CANDIDATES; every candidate is re-tested by the deferred pass with the reference's own operations in
// the reference's order (exact_hit in tor_kernels.hip: spheres.nim:29-48 unfused), and a candidate that fails there costs nothing but
// time.  So the loop may use any test that never drops an object the reference's test keeps.  This one evaluates the same
// quadratic with FMAs -- 11 / 12 / 14 float64 instructions for a static / y-only moving / moving sphere instead of
// 17 / 19 / 23 -- and leans it towards "keep" by more than the two evaluations can differ:
//     hb'  = fma(ocz, dz, fma(ocy, dy, fma(ocx, dx, -mu)))            mu = 2^-48 B D1
//     cc'  = fma(ocz, ocz, fma(ocy, ocy, fma(ocx, ocx, -r^2)))
//     t'   = fma(-a, cc', a M)                                        M  = 2^-45 B^2
//     disc'= fma(hb', hb', t')
//     keep = (hb' < 0 or t' >= 0) and disc' >= 0          (sign bits, one v_bitop3)
// with B >= |o| + |c0| + |dc||f| + |r| (|o|_1 from the ray, the rest a per-segment constant from the host: segs[6], segs[7])
// and D1 = |dx| + |dy| + |dz|.  With u = 2^-53, H = oc.d, C = |oc|^2 - r^2, D = H^2 - a C in exact arithmetic on the
// float64 inputs: either evaluation has |hb - H| <= 6.3 u B D1, |cc - C| <= 19 u B^2, |disc - D| <= 48 u B^2 a (the
// centres differ by <= 3.1 u B per component between c0 + dc*f rounded twice and the folded fma; |oc| <= B,
// |H| <= B |d|, D1 <= sqrt(3) |d|).  The reference's hit() can accept a root only if disc_ref > 0 and (hb_ref < 0 or
// cc_ref < 0) -- both roots are <= 0 otherwise.  With mu = 32 u B D1 and M = 256 u B^2:
//   hb_ref < 0  =>  H < 6.3 u B D1 < mu / 2  =>  hb' < 0, and (H - mu)^2 >= H^2, so
//                   disc' >= D + a M - 48 u B^2 a > (256 - 48 - 48) u B^2 a > 0;
//   cc_ref < 0  =>  C < 19 u B^2  =>  cc' < 38 u B^2 < M  =>  t' > 0, and
//                   disc' >= (H - mu)^2 - a C + a M - 48 u B^2 a > (256 - 19 - 48) u B^2 a > 0.
// Nothing the reference accepts is dropped.  Overflowing margins (|o| beyond 1e150) keep everything; a NaN is dropped
// by both tests or re-tested exactly; a = 0 (d = 0) keeps everything and the exact test rejects it (disc = 0).
// (TOR_SCREEN_MUTATE: the mutation check of tools/mutation_check.sh -- every margin of the three screens set to zero; the host
// tests of tests/test_screen.py must then FAIL, which shows that they sit on the decision boundary.  Never defined in a product build.)
#if defined(TOR_SCREEN_MUTATE) && TOR_SCREEN_MUTATE == 1
#define TOR_MARGIN(x) 0.0
#else
#define TOR_MARGIN(x) (x)
#endif
TOR_HD void screen_margins(double B, double d1, double a, double& negmu, double& am) {
  negmu = TOR_MARGIN(-(B * d1) * 0x1p-48);
  am = TOR_MARGIN(a * ((B * B) * 0x1p-45));
}
// returns a word whose SIGN BIT is the decision (set = keep)
TOR_HD int screen_filter(double ocx, double ocy, double ocz, double dx, double dy, double dz, double a, double negmu,
                         double am, double r2) {
  const double hb = fma_(ocz, dz, fma_(ocy, dy, fma_(ocx, dx, negmu)));
  const double cc = fma_(ocz, ocz, fma_(ocy, ocy, fma_(ocx, ocx, -r2)));
  const double t = fma_(-a, cc, am);
  const double disc = fma_(hb, hb, t);
  const unsigned h = (unsigned)(double_to_bits(hb) >> 32), y = (unsigned)(double_to_bits(t) >> 32), z = (unsigned)(double_to_bits(disc) >> 32);
  // f(x, y, z) = (x | ~y) & ~z on the sign bits: one v_bitop3_b32, truth table 0x51
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
  return (int)__builtin_amdgcn_bitop3_b32(h, y, z, 0x51);
#else
  return (int)((h | ~y) & ~z);
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// Screen, second form (round 4): the same conservative decision with the quadratic EXPANDED around the ray, so that the
// per-object work is nothing but fused multiply-adds against the object's record -- no o - c subtractions -- and with the
// direction NORMALISED once per ray, so that `a` drops out of the per-object work:
//     H~ = oc . d~           d~ = d / |d| (float64: sqrt and division correctly rounded, then one product per component)
//     hb'' = (o . d~ - mu~) - c . d~                                        3 fma against {cx, cy, cz}
//     t''  = (M~ - |o|^2) + 2 o . c - K          K = |c|^2 - r^2 (host)    3 fma + 1 add
//     disc''= fma(hb'', hb'', t'')               keep = (hb'' < 0 or t'' >= 0) and disc'' >= 0   (one v_bitop3, 0x51)
// = 8 float64 instructions for a static sphere (11 in the first form).  When the objects of a segment share c0.y bit for bit
// (spheres resting on a plane: 481 of random_scene's 485) the y terms are per-ray constants too:
//     static, uniform y :  hb'' = P - cx d~x - cz d~z ;  t'' = T + 2 ox cx + 2 oz cz - K'          K' = cx^2 + cz^2 - r^2     6 instructions
//     mover along y     :  c.y(f) = Y + f dcy, oc.y = (oy - Y) - f dcy:
//                          hb'' = P - cx d~x - cz d~z - (f d~y) dcy
//                          t''  = T + 2 ox cx + 2 oz cz + (2 f (oy - Y)) dcy - f^2 dcy^2 - K'                                9 instructions (12)
//   with P = ox d~x + oz d~z + (oy - Y) d~y - mu~ and T = M~ - ox^2 - oz^2 - (oy - Y)^2 per ray and segment.
//
// Why it is conservative.  u = 2^-53.  Exact quantities on the float64 inputs (c^ = c0 + f dc exact, oc^ = o - c^):
// H = oc^ . d, A = |d|^2, C = |oc^|^2 - r^2, D = H^2 - A C; normalised H~ = H / sqrt(A), D~ = D / A = H~^2 - C.  From the first
// form's analysis of the REFERENCE's evaluation: it can accept a root only if disc_ref > 0 and (hb_ref < 0 or cc_ref < 0), and
//   hb_ref < 0 => H < 6.3 u B D1 => H~ < 6.3 sqrt(3) u B < 11 u B;   cc_ref < 0 => C < 19 u B^2;   disc_ref > 0 => D~ > -48 u B^2.
// This form computes hb'' = H~ - mu~ + e_h and t'' = M~ - C + e_t, and the sign of fma(hb'', hb'', t'') is the sign of the exact
// hb''^2 + t''.  Error budgets (every bracket (|o_i| + |c_i| + |f dc_i|) <= B, sum |d~_i| <= sqrt(3)(1 + 4u)):
//   e_h: d~ carries a relative error <= 3.1 u per component (|d|^2 as the reference sums it: 2.5 u, sqrt, reciprocal, product);
//        oy - Y, f d~y one rounding each; at most 7 fused operations in the two chains (per-ray part, per-object part):
//        |e_h| <= (3.1 + 1 + 7) u sqrt(3) B + 7 u mu~ < 19.3 u B;
//   e_t: K, K' (host: 3 roundings), f^2, 2 f (oy - Y), g + nf2 dcy (<= 2 roundings each), at most 9 fused operations over terms whose
//        magnitudes sum to <= B^2 + M~:  |e_t| < 16 u B^2.
// With mu~ = 64 u B = 2^-47 B and M~ = 256 u B^2 = 2^-45 B^2:
//   hb_ref < 0 (and D~ > -48 u B^2):  hb'' < 11 u B + 19.3 u B - 64 u B < 0; with m = mu~ - e_h >= 44.7 u B >= 2 H~,
//        hb''^2 = (H~ - m)^2 >= H~^2, so hb''^2 + t'' >= D~ + M~ - |e_t| > (256 - 48 - 16) u B^2 > 0:  kept;
//   cc_ref < 0:  t'' > (256 - 19 - 16) u B^2 > 0, hence disc'' > 0:  kept.
// B >= |o|_1 + |c0| + |r| + |dc||f| as in the first form (segs[6], segs[7] from the host, |o|_1 from the ray).
// Rays outside the ranges this argument needs -- |d|^2 outside [2^-900, 2^900] (the normalisation would lose bits or
// overflow), B^2 not finite -- are WILD: they keep every object (T = +inf, d~ = 0, 2o = 0) and the exact test decides.
// A non-finite time fraction f gives a non-finite centre in the reference, which can never be hit; dropping is correct then.
// Checked from this source on the host (tor_selftest_screen2_host, tests/test_screen.py) and on the GPU (every strict
// brute-force parity test runs through it).
struct ScreenRay {     // per ray and closest-hit query
  double dnx, dny, dnz;  // d~
  double s1;             // |o|_1
  double ox, oy, oz;
  bool wild;
};
// ONE sign per test.  keep = (hb'' < 0 or t'' >= 0) and disc'' >= 0 is the sign of a single value:
//     q = t'' + max(-hb'', 0)^2        hb'' >= 0: q = t'' (and t'' >= 0 implies disc'' = hb''^2 + t'' >= 0);  hb'' < 0: q = disc''
// and max(., 0) is the CLAMP modifier of the instruction that ends the hb chain -- free -- provided the value stays below the clamp's
// upper bound 1.  So the segment's per-ray factors carry a power of two sigma <= 1 / (2 B) (|hb''| <= B (1 + 2^-40): the clamp never
// saturates): the hb chain is evaluated as Nh = clamp(sigma (c.d~ - P)) = sigma max(-hb'', 0), the t chain as -sigma^2 t'' (the `- K`
// becomes one more fma, same count), and q' = fma(-Nh, Nh, -sigma^2 t'') = -sigma^2 q.  Scaling by powers of two is exact, so the
// decision is the three-sign decision above bit for bit except where q is exactly 0, which the proof never needs (every object
// it keeps has q > 0 strictly).  The v_bitop3_b32 is gone: 7 / 9 / 10 instructions per common-height static / static / mover
// instead of 8 / 10 / 11, one of them (the v_alignbit into the mask) not float64.
struct ScreenSeg {     // per ray and segment (s = sigma)
  double hx, hy, hz;     // s d~ (0 for a wild ray)
  double Pn;             // s (mu~ - o.d~)            kinds 11 / 12: with oy - Y for oy
  double a2x, a2y, a2z;  // -s^2 2 o (0 for a wild ray)
  double Tn;             // -s^2 (M~ - |o|^2); -inf for a wild ray: everything is kept
  double ks;             // s^2
  double fdy, gn, f2n;   // kind 12: s f d~y, -s^2 2 f (oy - Y), s^2 f^2
};
TOR_HD ScreenRay screen2_ray(double ox, double oy, double oz, double dx, double dy, double dz, double a_strict) {
  ScreenRay r;
  const double inv = 1.0 / __builtin_sqrt(a_strict);
  r.dnx = dx * inv; r.dny = dy * inv; r.dnz = dz * inv;
  r.s1 = __builtin_fabs(ox) + __builtin_fabs(oy) + __builtin_fabs(oz);
  r.ox = ox; r.oy = oy; r.oz = oz;
  r.wild = !(a_strict >= 0x1p-900 && a_strict <= 0x1p900);
  return r;
}
// clamp(x) to [0, 1] with NaN -> 0: what the hardware's clamp modifier does (compute kernels run with DX10_CLAMP = 1)
TOR_HD double clamp01(double x) { return x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0; }
// fma(a, b, c) clamped to [0, 1]; a is wave-uniform (a scalar register on the device)
TOR_HD double fma_clamp_s(double a_uniform, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r;
  asm("v_fma_f64 %0, %1, %2, %3 clamp" : "=v"(r) : "s"(a_uniform), "v"(b), "v"(c));
  return r;
#else
  return clamp01(fma_(a_uniform, b, c));
#endif
}
// ... the same with every operand in a vector register (stage two of the plane-screened segments: per-lane records)
TOR_HD double fma_clamp_v(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  double r;
  asm("v_fma_f64 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return clamp01(fma_(a, b, c));
#endif
}
// reach, travel: segs[6], segs[7]; y_rel: 0 for the general static form (kind 10), else the segment's common c0.y (kinds 11, 12);
// f: the segment's time fraction (kind 12), else 0
TOR_HD ScreenSeg screen2_seg(const ScreenRay& r, double reach, double travel, double y_rel, double f) {
  ScreenSeg s;
  const double B = r.s1 + reach + travel * __builtin_fabs(f);
  const double mu = TOR_MARGIN(B * 0x1p-47);
  const double M = TOR_MARGIN((B * B) * 0x1p-45);
  // (f * f must stay finite too: f2n = sg2 f^2 below meets dcy = 0 -- a static that rests in a segment of movers along y -- as
  // inf x 0 = NaN otherwise, and the NaN's clear sign bit would DROP a sphere the reference hits.  |f| > 1.3e154 with
  // travel |f| still below the B^2 limit needs travel < 1: random_scene's movers, shutter_close ~ 1e155.  ADVICE r5.)
  const bool wild = r.wild || !((B * B) * 0x1p-45 < __builtin_inf()) || !(f * f < __builtin_inf());
  // sigma = 2^-(e + 2) for B in [2^e, 2^(e+1)): sigma B < 1/2.  (B = 0 or denormal: 2^1020; harmless, every product below is 0 or tiny)
  uint64_t e = (double_to_bits(B) >> 52) & 0x7ffu;
  if (e < 3u) e = 3u;
  if (e > 0x7fbu) e = 0x7fbu;
  const double sg = bits_to_double((uint64_t)(0x7fcu - e) << 52), sg2 = sg * sg;
  const double oy = r.oy - y_rel;
  const double dnx = wild ? 0.0 : r.dnx, dny = wild ? 0.0 : r.dny, dnz = wild ? 0.0 : r.dnz;
  s.hx = sg * dnx; s.hy = sg * dny; s.hz = sg * dnz;
  const double P = fma_(oy, dny, fma_(r.oz, dnz, r.ox * dnx)) - mu;
  const double Q = fma_(oy, oy, fma_(r.oz, r.oz, r.ox * r.ox));
  s.Pn = wild ? 0.0 : -(sg * P);
  s.Tn = wild ? -__builtin_inf() : -(sg2 * (M - Q));
  const double n2 = wild ? 0.0 : -(sg2 + sg2);
  s.a2x = n2 * r.ox; s.a2y = n2 * oy; s.a2z = n2 * r.oz;
  // (a wild ray keeps EVERYTHING: Tn = -inf and every factor 0 -- ks included, with K clamped to a finite value by the host
  // (screen2_K), so that no 0 x inf = NaN of unspecified sign can come out of the chain: ADVICE r4 -- a camera inside a sphere
  // 1e155 from the origin is hit by the reference, |c|^2 overflows, and the `keeps everything` promise must hold for it)
  s.ks = wild ? 0.0 : sg2;
  const double fw = wild ? 0.0 : f;   // (a non-finite f makes B, hence the ray, wild: no inf x 0 in the factors below)
  s.fdy = fw * s.hy;
  s.gn = fw * s.a2y;
  s.f2n = sg2 * (fw * fw);
  return s;
}
// the per-object tests; the returned word's SIGN BIT is the decision (set = keep), as screen_filter's
TOR_HD int screen2_word(double nh, double tn) {
  const double q = fma_(-nh, nh, tn);
  return (int)(unsigned)(double_to_bits(q) >> 32);
}
// kind 10: record {cx, cy, cz, K = |c|^2 - r^2}
// (kLane: the record is the lane's own -- vector registers -- instead of wave-uniform)
template <bool kLane = false>
TOR_HD int screen2_static(const ScreenSeg& s, double cx, double cy, double cz, double K) {
  const double nh = kLane ? fma_clamp_v(cx, s.hx, fma_(cy, s.hy, fma_(cz, s.hz, s.Pn))) : fma_clamp_s(cx, s.hx, fma_(cy, s.hy, fma_(cz, s.hz, s.Pn)));
  const double tn = fma_(s.ks, K, fma_(s.a2x, cx, fma_(s.a2y, cy, fma_(s.a2z, cz, s.Tn))));
  return screen2_word(nh, tn);
}
// kind 11: record {cx, cz, K' = cx^2 + cz^2 - r^2}
template <bool kLane = false>
TOR_HD int screen2_static_y(const ScreenSeg& s, double cx, double cz, double K) {
  const double nh = kLane ? fma_clamp_v(cx, s.hx, fma_(cz, s.hz, s.Pn)) : fma_clamp_s(cx, s.hx, fma_(cz, s.hz, s.Pn));
  const double tn = fma_(s.ks, K, fma_(s.a2x, cx, fma_(s.a2z, cz, s.Tn)));
  return screen2_word(nh, tn);
}
// kind 12: record {cx, cz, K', dcy} -- 32 bytes like the static records (the whole second-form table of random_scene is then
// 15.5 KB and fits the 16 KB scalar cache; with dcy^2 as a fifth field it was 21.7 KB and 4.5 % of the scalar loads missed).
// 2 f (oy - Y) dcy - f^2 dcy^2 = (g + nf2 dcy) dcy: the same two instructions as with a stored dcy^2.
template <bool kLane = false>
TOR_HD int screen2_movy_y(const ScreenSeg& s, double cx, double cz, double K, double dcy) {
  const double nh = kLane ? fma_clamp_v(dcy, s.fdy, fma_(cx, s.hx, fma_(cz, s.hz, s.Pn))) : fma_clamp_s(dcy, s.fdy, fma_(cx, s.hx, fma_(cz, s.hz, s.Pn)));
  const double w = fma_(s.f2n, dcy, s.gn);
  const double tn = fma_(s.ks, K, fma_(w, dcy, fma_(s.a2x, cx, fma_(s.a2z, cz, s.Tn))));
  return screen2_word(nh, tn);
}
// the host's side of the records (tor_scene.cpp build_layout; the self test)
// (clamped to the finite range: +-inf would meet the wild ray's zero factors as NaN; a NaN K -- a NaN centre or radius, which the
// reference can never hit -- becomes -max (fmax skips the NaN): kept by the screen, rejected by the exact test)
TOR_HD double screen2_clampK(double k) { return __builtin_fmin(__builtin_fmax(k, -0x1.fffffffffffffp1023), 0x1.fffffffffffffp1023); }
TOR_HD double screen2_K(double cx, double cy, double cz, double r2) { return screen2_clampK(((cx * cx + cy * cy) + cz * cz) - r2); }
TOR_HD double screen2_Ky(double cx, double cz, double r2) { return screen2_clampK((cx * cx + cz * cz) - r2); }

// ---------------------------------------------------------------------------------------------------------------------
// STAGE ONE in front of the second form (round 4, kinds 11 and 12): the PLANE screen.  A sphere can only be hit by a ray whose
// LINE passes within r of its centre, and the distance from the centre to the line is at least the distance from the centre to
// any plane that contains the line.  For the vertical plane through the ray that distance does not involve y at all:
//     s = n . (c_xz - o_xz)          n = (-d~z, d~x)   (normal of the ray's ground track, NOT normalised: |n|^2 = w2 = d~x^2 + d~z^2)
//     keep  <=>  s^2 < (R^2 + M~) w2      R = the largest |radius| of the segment, M~ = 2^-45 B^2 as above
// = 2 fused multiply-adds against {cx, cz} + 1 for the sign + the v_alignbit: 4 instructions per object -- for a static sphere
// and for a mover along y alike (its cx, cz do not move) -- instead of 7 / 10, and no square root or division per ray.  It keeps
// the spheres in a band of width 2 R along the ray's ground track: 9.2 of random_scene's 481 small spheres for an average query
// (the second form: 0.6).  Those go through the second form PER LANE (kernel/integrate_loop_plane.inc: stage two), and what
// survives that is exactly what the second form alone would have kept, because stage one never drops what the second form's
// PROOF needs kept:
//   the reference accepts a root only if disc_ref > 0, which implies D~ = r^2 - dist(c^, line)^2 > -48 u B^2 (above), so with the
//   exact unit normal n^ of the exact ground track  (n^ . (c_xz - o_xz))^2 <= dist^2 < r^2 + 48 u B^2.  Computed: the components of
//   n carry the relative error of d~ (3.1 u each, so n = n~ + delta with |delta| <= 3.1 u |n~|, n~ the perpendicular of the exactly
//   normalised direction, |n~| = w); the constant n . o_xz (a product and an fma) and the two fused operations of the chain round
//   four times, each by <= u x a magnitude <= 2 sqrt(2) w B:  |s' - n~ . (c_xz - o_xz)| <= (3.1 + 9.9) u w B = 13 u w B, and with
//   |n~ . (..)| = w dist_2D <= w B:   s'^2 < w^2 (r^2 + (48 + 27) u B^2).   w2 as computed is >= w^2 (1 - 8.2 u) (the components'
//   3.1 u twice, the sum's own rounding), the threshold's sum and product round twice more:
//   s'^2 < w^2 (r^2 + 75 u B^2) < (R^2 (1 + 2^-40) + 256 u B^2) w2' (1 - 2 u)   since 2^-40 >> 11 u and 256 (1 - 11 u) > 75.
// c_xz is exact here: statics, and movers whose c1 - c0 has x = z = 0 exactly (group_moves_along_y_only).
// A ray whose ground track has no direction (w2 < 2^-200: vertical), whose threshold leaves the normal range, or that is wild
// keeps everything.
//
// Round 5 -- the test never reads y, so it serves EVERY float64 segment, not only the common-height ones it was built for:
//   xkind 10 (statics at any height) and 14 (movers along y at any height): the same {cx, cz} table, the same 4 instructions;
//   xkind 13 (movers whose centre travels in x or z): c^_xz = c0_xz + f dc_xz is evaluated inside the chain,
//       s' = nx c0x + nz c0z + (f nx) dcx + (f nz) dcz + c0       record {c0x, c0z, dcx, dcz}: 5 float64 instructions + the v_alignbit
//     against the exact c^ = c0 + f dc that the first form's analysis of the reference is stated for (the reference's own centre,
//     c0 + dc*f rounded twice, is within 3.1 u B of it per component, which the 48 u B^2 above already contains).  Two more
//     roundings in the chain and one each in f nx, f nz (|f nx dcx| <= w |f| |dc| <= w B):  |s' - n~ . (c^_xz - o_xz)| <=
//     (3.1 + 6 x 2.83 + 2) u w B < 22.1 u w B, so s'^2 < w^2 (r^2 + (48 + 45) u B^2) -- still far inside the 256 u B^2 of the
//     threshold (256 (1 - 11 u) > 93).  B >= |o|_1 + |c0| + |r| + |dc| |f| as everywhere (segs[6], segs[7]).
// Stage two then runs, per lane, the test the wave-uniform loop would have run on the segment: the second form for 10 / 11 / 12,
// the first form (screen_filter, centre folded into o - c) for 13 / 14 -- both proofs start from disc_ref > 0, which is all stage
// one relies on.
struct PlaneRay {   // per ray and closest-hit query
  double nx, nz;    // (-d~z, d~x)
  double w2;        // nx^2 + nz^2
  bool all;         // no ground track or a wild ray: every object is kept
};
struct PlaneSeg {   // per ray and segment
  double nx, nz;    // normal of the ground track (0 when everything is kept)
  double c0;        // -(n . o_xz)
  double negthr;    // -(R^2 (1 + 2^-40) + M~) w2; -inf: everything is kept
  double fnx, fnz;  // f n (xkind 13); 0 when everything is kept
};
TOR_HD PlaneRay plane_ray(const ScreenRay& r) {
  PlaneRay pr;
  pr.nx = -r.dnz;
  pr.nz = r.dnx;
  pr.w2 = fma_(r.dnz, r.dnz, r.dnx * r.dnx);
  pr.all = r.wild || !(pr.w2 >= 0x1p-200);
  return pr;
}
TOR_HD PlaneSeg plane_seg(const ScreenRay& r, const PlaneRay& pr, double reach, double travel, double f, double rmax2) {
  PlaneSeg s;
  const double B = r.s1 + reach + travel * __builtin_fabs(f);
#if defined(TOR_SCREEN_MUTATE) && TOR_SCREEN_MUTATE <= 2   // (level 2 of the mutation check: only stage one's margins)
  const double M = 0.0;
  const double thr = rmax2 * pr.w2;
#else
  const double M = (B * B) * 0x1p-45;
  const double thr = (fma_(rmax2, 0x1p-40, rmax2) + M) * pr.w2;
#endif
  const bool all = pr.all || !(thr >= 0x1p-900 && thr < __builtin_inf());
  s.nx = all ? 0.0 : pr.nx;
  s.nz = all ? 0.0 : pr.nz;
  s.c0 = all ? 0.0 : -fma_(s.nx, r.ox, s.nz * r.oz);
  s.negthr = all ? -__builtin_inf() : -thr;
  s.fnx = all ? 0.0 : f * s.nx;   // (a non-finite f: B and the threshold are not finite either -> `all`)
  s.fnz = all ? 0.0 : f * s.nz;
  return s;
}
// the returned word's SIGN BIT is the decision (set = keep)
TOR_HD int plane_word(const PlaneSeg& s, double cx, double cz) {
  const double v = fma_(s.nx, cx, fma_(s.nz, cz, s.c0));
  const double q = fma_(v, v, s.negthr);
  return (int)(unsigned)(double_to_bits(q) >> 32);
}
// xkind 13: record {c0x, c0z, dcx, dcz}
TOR_HD int plane_word_mov(const PlaneSeg& s, double c0x, double c0z, double dcx, double dcz) {
  const double v = fma_(s.nx, c0x, fma_(s.nz, c0z, fma_(s.fnx, dcx, fma_(s.fnz, dcz, s.c0))));
  const double q = fma_(v, v, s.negthr);
  return (int)(unsigned)(double_to_bits(q) >> 32);
}
// ---------------------------------------------------------------------------------------------------------------------
// STAGE ONE IN FLOAT32 (xkinds 10, 11, 12, 14: the {cx, cz} table).  The float64 chain above costs 3 float64 fma + the
// v_alignbit = 7 issue slots per object; the same test in float32 costs 2 v_fma_f32 + 1 v_sub_f32 (|v| - T, the abs a free
// modifier) + the v_alignbit = 4.  The record is 8 bytes {cx - Ox, cz - Oz} (xpl32, rounded to nearest): the centre relative to a
// per-segment origin O (the middle of the centres' ground box), so that the float32 offsets stay small against the scene.
//     v = fma32(nx, cx', fma32(nz, cz', c0))        keep  <=>  |v| < T          (the sign bit of |v| - T, as plane_word's)
// Stage one only has to keep a SUPERSET of what the float64 plane screen keeps: everything behind it (stage two, the exact test)
// is unchanged, and the float64 screen's own proof only needs its band to contain every object the second form's proof needs.
// Why it is a superset.  Let n be the float64 normal (plane_seg), S = n . (c_xz - o_xz) exactly, and v64 the float64 chain.
//   The float64 screen keeps iff v64^2 < thr (fma(v, v, -thr) rounds without crossing 0).  Its four roundings are each <= u N1 B
//   (u = 2^-53, N1 = |nx| + |nz|, every partial sum <= N1 (|o|_1 + reach) <= N1 B), so it keeps only if
//   |S| < sqrt(thr) + 4 u N1 B.  Since thr >= 2^-45 B^2 w2 and N1 <= sqrt(2) w, 4 u N1 B < 2^-27 sqrt(thr):  |S| < sqrt(thr)(1 + 2^-27).
//   The float32 chain, with n32 = (float)n (relative 2^-24 per component), o' = o - O (float64), Co = |o'x| + |o'z|, Cm >= every
//   stored |c'| (host), E >= |c' - (c - O)| for every stored coordinate (host, exact differences), c0 = -(n32 . o') in float64
//   rounded to float32:
//     the exact n32 . (c'_32) + c0_32 differs from S by at most
//       2^-24 N1 (Cm + Co + E)          n -> n32 against |c - o| <= Cm + E + Co per component
//     + N1 (1 + 2^-24) E                the stored centres' rounding
//     + 2^-24 N1 Co (1 + 2^-23) + 4 u N1 Co     c0: float64 chain and its rounding to float32
//   and the two float32 fma round by 2^-24 each of a value <= N1 (1 + 2^-24)(Cm + E) + |c0|:  2^-23 N1 (Cm + Co + E) (1 + 2^-22).
//   In all |v32 - S| <= N1 E (1 + 2^-24) + 2^-22 N1 (Cm + Co + E) (1 + 2^-20); subnormal results (conversions and fma below
//   2^-126) add at most 2^-150 each, times a factor <= Cm + Co + E where n is involved: < 2^-140 (1 + Cm + Co + E).
//   So with
//     T >= (1 + 2^-20) (sqrt(thr) + N1 E) + (2^-21 N1 + 2^-140) (Cm + Co + E) + 2^-140
//   the float64 screen's keep implies |v32| < T.  T is summed in float64 (all terms positive; the factor (1 + 2^-40) covers the
//   sums, the products and the square root), then converted to float32 ROUNDED UP.  The comparison is |v32| - T < 0 in float32: a
//   negative exact difference never rounds to +0.
// The band widens by ~N1 E + 2^-21 N1 (Cm + Co): on random_scene (offsets ~11, E ~ 2^-21) ~1e-5 against R = 0.2 -- invisible.
// Keep everything (n = 0, c0 = 0, T = +inf: |0| - inf = -inf) when the float64 screen does, or when Cm, Co or E is above 2^60 or
// not finite, or T is not finite in float32.  The host clamps every stored offset to [-2^100, 2^100] (finite), so 0 x c' is 0;
// a segment with a non-finite or NaN offset gets E = +inf and keeps everything.  Padding slots hold {2^100, 0x1.3c6ef3p99}: no
// ray with a ground track keeps them (|v| ~ 2^100 against T < 2^62 unless n is perpendicular to the padding point to within
// 2^-38), a keep-everything ray keeps them, and stage two drops them as it drops the float64 padding.
// xkind 13 (movers in x / z) keeps the float64 chain plane_word_mov.
// (TOR_SCREEN_MUTATE == 3: the mutation check of this proof -- T = sqrt(thr) rounded to nearest, every margin above dropped; the
// superset test of tests/test_plane32.py must then FAIL.  Never defined in a product build.)
// Stage one's whole-word loop requests its float32 records kPlaneAhead groups of 8 objects (one s_load_dwordx16, 16 floats) ahead
// of the wait that needs them (kernel/integrate_loop_plane.inc), so it reads that far behind a segment's last record: the host
// keeps kPlaneSlackFloats of padding behind the table (tor_scene.cpp).  0: the compiler's own requests, one record ahead.
// (-DTOR_PLANE_AHEAD=0: A/B builds only)
#ifdef TOR_PLANE_AHEAD
constexpr int kPlaneAhead = TOR_PLANE_AHEAD;
#else
constexpr int kPlaneAhead = 1;
#endif
static_assert(kPlaneAhead == 0 || kPlaneAhead == 1, "two groups ahead would need scalar loads to return in order");
constexpr int kPlaneGroupFloats = 16;
constexpr int kPlaneSlackFloats = 16;
static_assert(kPlaneSlackFloats >= kPlaneAhead * kPlaneGroupFloats && kPlaneSlackFloats >= 2, "the plane table's slack must cover stage one's read-ahead");
constexpr float kPlane32PadX = 0x1p100f, kPlane32PadZ = 0x1.3c6ef3p99f;
constexpr double kPlane32Clamp = 0x1p100;
struct PlaneSeg32 {  // per ray and segment
  float nx, nz;      // (float) of the float64 normal; 0 when everything is kept
  float c0;          // -(n32 . (o_xz - O)), float64 rounded to float32
  float T;           // the threshold on |v|; +inf: everything is kept
};
TOR_HD float f32_up(double x) {  // the smallest float32 >= x (x >= 0 and below the float32 range)
  float f = (float)x;
  if ((double)f < x) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + 1u);
  return f;
}
// ps: the float64 plane screen of the same ray and segment; (orx, orz): the segment's origin O; e32, cm: E and Cm (host)
TOR_HD PlaneSeg32 plane_seg32(const ScreenRay& r, const PlaneSeg& ps, double orx, double orz, double e32, double cm) {
  PlaneSeg32 s;
  const double ox = r.ox - orx, oz = r.oz - orz;
  const double co = __builtin_fabs(ox) + __builtin_fabs(oz);
  const double n1 = __builtin_fabs(ps.nx) + __builtin_fabs(ps.nz);
  const double thr = -ps.negthr;
  const float nx = (float)ps.nx, nz = (float)ps.nz;
  const double c0 = -fma_((double)nx, ox, (double)nz * oz);
#if defined(TOR_SCREEN_MUTATE) && TOR_SCREEN_MUTATE == 3
  (void)n1;
  const double T = __builtin_sqrt(thr);
  const float tf = (float)T;
#else
  const double T = (fma_(0x1p-20, __builtin_sqrt(thr) + n1 * e32, __builtin_sqrt(thr) + n1 * e32) +
                    fma_(n1, 0x1p-21, 0x1p-140) * ((cm + co) + e32) + 0x1p-140) * (1.0 + 0x1p-40);
  const float tf = T < 0x1p126 ? f32_up(T) : __builtin_inff();
#endif
  const bool all = !(ps.negthr > -__builtin_inf()) || !(cm <= 0x1p60 && co <= 0x1p60 && e32 <= 0x1p60) || !(tf < __builtin_inff());
  s.nx = all ? 0.0f : nx;
  s.nz = all ? 0.0f : nz;
  s.c0 = all ? 0.0f : (float)c0;
  s.T = all ? __builtin_inff() : tf;
  return s;
}
// the returned word's SIGN BIT is the decision (set = keep); (cx, cz): the stored offsets from the segment's origin
TOR_HD int plane_word32(const PlaneSeg32& s, float cx, float cz) {
  const float v = __builtin_fmaf(s.nx, cx, __builtin_fmaf(s.nz, cz, s.c0));
  const float q = __builtin_fabsf(v) - s.T;
  return (int)__builtin_bit_cast(uint32_t, q);
}
// The host's side of a segment's float32 table (tor_scene.cpp build_layout): the stored offset of one coordinate c from the
// origin coordinate o, and a bound of its error against the exact c - o (err_io: the running maximum; +inf for a non-finite
// offset).  d + t = c - o exactly (two-sum), d - (double)f is exact (f is d rounded to float32: Sterbenz), the sum rounds once.
TOR_HD float plane32_offset(double c, double o, double& err_io) {
  const double d = c - o;
  const double bb = d - c, t = (c - (d - bb)) + (-o - bb);
  const double dc = __builtin_fmin(__builtin_fmax(d, -kPlane32Clamp), kPlane32Clamp);
  const float f = (float)dc;
  const double e = __builtin_fabs((d - (double)f) + t) * (1.0 + 0x1p-50);
  err_io = !(e < __builtin_inf()) ? __builtin_inf() : __builtin_fmax(err_io, e);
  return f;
}

// ---------------------------------------------------------------------------------------------------------------------
// THE REACH PASS in front of stage one's whole words (xkinds 10, 11, 12, 14).  Stage one tests the whole infinite ground LINE of
// a ray against every slot; a sphere can only be a candidate where the RAY -- t >= 0 -- is near it, in y as well.  The host sorts
// a segment's objects by an even top-down split of their ground positions (tor_scene.cpp), so that a word of 32 consecutive slots
// is a small patch of ground, and keeps one record per word of the sorted list (KParams.xwb, kReachRecFloats floats):
//     {xlo, xhi, zlo, zhi}   float32: the box of the word's stored offsets c' (xpl32), grown by G0 = (R + E)(1 + 2^-40) and rounded
//                            outward; R = the segment's largest |radius|, E = the table's rounding bound (plane_seg32)
//     {ylo, yhi}             float64: the heights the SEGMENT's centres take while the time fraction f is in [0, 1], grown by R and
//                            rounded outward (the same two values in every word of a segment)
// A word that is not wholly inside one such segment, or whose segment holds a non-finite centre or radius, is (-inf, +inf)
// throughout: everybody reaches it.  A lane takes the piece of its ray with t >= 0 inside the slab [ylo - S, yhi + S], the xz
// bounding box of that piece relative to the segment's origin O, grows it by S (+ 2^-40 of each end) and rounds it outward to
// float32 (reach_ray: float64, once per segment and pass); a word whose box does not meet it is NOT REACHED (reach_miss: four
// float32 compares against scalar operands).  Words no lane of the wave reaches are not walked at all, and a lane's bits in a
// walked word it does not reach are cleared before the word is stored.
//
// What that needs: a slot in a word the lane does not reach is dropped by the segment's own second-stage test (screen2_* for
// xkinds 10 / 11 / 12, screen_filter for 14) -- then stage two leaves the bits it leaves today, and the candidates and the canvas
// do not change; the reference cannot accept such a slot either, since those tests keep whatever it accepts.
//   Notation as above: c^ the exact centre at f, oc^ = o - c^, d^ the exact unit direction, H~ = oc^ . d^, dist the distance from c^
//   to the ray's LINE, r the radius, B the segment's bound for this ray, u = 2^-53.
//   Second form.  It keeps only if disc'' >= 0 and (t'' >= 0 or hb'' < 0).
//     t'' >= 0:  M~ - C + e_t >= 0 with |e_t| < 16 u B^2, so |oc^|^2 <= r^2 + 272 u B^2: the ORIGIN (t = 0) is within
//       sqrt(r^2 + 2^-44 B^2) <= r + 2^-22 B of c^.
//     hb'' < 0 and disc'' >= 0:  H~ < mu~ + |e_h| < 84 u B, and with m = mu~ - e_h in [44 u B, 84 u B]:
//       0 <= (H~ - m)^2 + M~ - C + e_t, and since C = H~^2 + dist^2 - r^2:  dist^2 <= r^2 + m^2 - 2 H~ m + (256 + 16) u B^2.
//       The foot of the perpendicular is at t_c = -H~ > -84 u B.  Centre ahead (H~ < 0, |H~| <= B): -2 H~ m <= 168 u B^2, so
//       dist^2 <= r^2 + 441 u B^2 < r^2 + 2^-44 B^2 and the foot is ON the ray.  Centre abeam or just behind (0 <= H~ < 84 u B):
//       dist^2 <= r^2 + 273 u B^2 and the origin is within 84 u B of the foot.
//     Either way some point p = o + t d^, 0 <= t <= 2 B, of the ray is within  r + 2^-22 B + 2^-46 B  of c^.
//   First form (xkind 14: screen_filter, margins mu = 2^-48 B D1, M = 2^-45 B^2 a): the same case split on its hb' and t' after
//     dividing by |d|, |d|^2 (mu / |d| <= sqrt(3) 2^-48 B, errors 6.3 u B D1 and 48 u B^2 a as stated at the top of this file)
//     gives dist^2 < r^2 + (256 + 48 + 2 x 6 x 1.8) u B^2 < r^2 + 2^-44 B^2 and the same conclusion.
//   So |p.y - c^.y| and |p_xz - c^_xz| are both <= r + 2^-21.9 B.  c^.y lies between c0.y and c0.y + dcy for f in [0, 1] (a static: dcy =
//   0), hence inside [ylo + R, yhi - R] of the record, and p.y inside [ylo - 2^-21.9 B, yhi + 2^-21.9 B].  The lane's piece:
//     computed with d~ for d^ (3.1 u per component: p moves by <= 2 B x 3.1 u), o - O in float64 (u B), the reciprocal of d~y and two
//     products per end (each relative 2 u of a magnitude <= |end| + B), the slab ends' own sums (u (|y| + B)) -- in all
//     <= 2^-49 B + 2^-50 |end| per coordinate, and the piece contains p up to that.
//     A ray flatter than |d~y| < 2^-30 is not clipped at all (its piece is the whole ray: the far end +-inf).
//   The stored c' is within E of c^_xz - O (plane_seg32), and r <= R, so the grown box of the word holds every point within r of one
//   of its centres' stored offsets + E; with S = 2^-21 B = 2 x 2^-22 B the lane's box, grown by S + 2^-40 |end|, holds p_xz - O with
//   0.9 x 2^-22 B to spare.  The conversions to float32 move each end outward (a further 2^-23 of it + 2^-140, then round to nearest).
//   Hence: second stage keeps the slot  =>  the two boxes meet  =>  the word is reached.
// The slack is the float32 scale of the boxes (2^-21 B against offsets rounded at 2^-24): what stage two's own margin asks for --
// M~ = 2^-45 B^2 lets it keep a small sphere 2^-22.5 B from the line -- and invisible against R unless the scene is 1e5 from the
// origin (at 1e7 the slack is 9 units and stage two's own band 3.4).
// Every lane reaches everything -- the box (-inf, +inf) -- when the float32 plane screen keeps everything (a wild ray, no ground
// track, a threshold out of range: PlaneSeg32.T = +inf), when f is outside [0, 1] or not a number (the slab does not bound the
// centres then), or when an end of the piece is not a number; every compare of reach_miss is false on a NaN.  A piece that is
// EMPTY -- the ray never enters the slab -- reaches only the (-inf, +inf) words.
// (TOR_SCREEN_MUTATE == 4: the mutation check of this proof -- boxes and slab not grown by the radius, no slack, nothing rounded
// outward; tests/test_reach.py must then FAIL.  Never defined in a product build.)
// (-DTOR_REACH=0: A/B builds only -- stage one's word loop as it was, the table unused.)
#ifndef TOR_REACH
#define TOR_REACH 1
#endif
#if defined(TOR_SCREEN_MUTATE) && TOR_SCREEN_MUTATE == 4
constexpr bool kReachMutant = true;
#else
constexpr bool kReachMutant = false;
#endif
// Words nobody reaches are not written at all: the pass keeps a wave-uniform mask of them and the summary's rebuild after stage two
// leaves them out (kernel/integrate_loop_plane.inc, tor_kernels.hip `reach_skip`).  -DTOR_REACH_NOZERO=0: A/B builds only -- they are
// written 0 up front, as they were.  (2: the MUTANT -- no zero stores and no mask; every case of tests/test_gpu_reach_feed.py must
// then FAIL on `candidates`.  Never a product build.)
#ifndef TOR_REACH_NOZERO
#define TOR_REACH_NOZERO 1
#endif
constexpr int kReachNoZero = TOR_REACH_NOZERO;
constexpr int kReachRecFloats = 8;  // {xlo, xhi, zlo, zhi} float32, {ylo, yhi} float64
constexpr int kReachMinWords = 8;       // the host runs the pass on segments of enough objects for this many whole words wherever they start ...
constexpr double kReachSlabRatio = 8.0;  // ... whose height slab, times this, fits the smaller extent of their ground box (tor_scene.cpp)
constexpr int kReachSlackWords = 4; // records behind the table: the reach pass reads them four at a time (kernel/integrate_loop_plane.inc)
struct ReachRay { float xlo, xhi, zlo, zhi; };  // per ray, segment and pass: the piece's box, offsets from the segment's origin
// the largest float32 <= x / the smallest >= x by rounding to nearest a value moved out by more than half an ulp
TOR_HD float reach_f32_down(double x) { return kReachMutant ? (float)x : (float)(fma_(-__builtin_fabs(x), 0x1p-23, x) - 0x1p-140); }
TOR_HD float reach_f32_up(double x) { return kReachMutant ? (float)x : (float)(fma_(__builtin_fabs(x), 0x1p-23, x) + 0x1p-140); }
// all: PlaneSeg32.T == +inf; B: the segment's bound for this ray (|o|_1 + reach + travel |f|); (orx, orz): the segment's origin O
TOR_HD ReachRay reach_ray(const ScreenRay& r, bool all, double B, double orx, double orz, double ylo, double yhi, double f) {
  const double inf = __builtin_inf();
  const double S = kReachMutant ? 0.0 : B * 0x1p-21;
  const double ox = r.ox - orx, oz = r.oz - orz;
  const bool steep = __builtin_fabs(r.dny) >= 0x1p-30, up = r.dny > 0.0;
  const double y0 = ylo - S, y1 = yhi + S;
  // the piece in y: from the origin, or the face the ray enters the slab by, to the face it leaves by
  const double ynear = up ? (r.oy > y0 ? r.oy : y0) : (r.oy < y1 ? r.oy : y1);
  const double yfar = up ? y1 : y0;
  const bool empty = steep && (up ? ynear > yfar : ynear < yfar);
  const double inv = 1.0 / (steep ? r.dny : 1.0);
  const double sa = steep ? (ynear - r.oy) * inv : 0.0, sb = (yfar - r.oy) * inv;  // t at the two ends (units of d~)
  const double xa = fma_(sa, r.dnx, ox), za = fma_(sa, r.dnz, oz);
  const double xb = steep ? fma_(sb, r.dnx, ox) : (r.dnx > 0.0 ? inf : (r.dnx < 0.0 ? -inf : ox));
  const double zb = steep ? fma_(sb, r.dnz, oz) : (r.dnz > 0.0 ? inf : (r.dnz < 0.0 ? -inf : oz));
  const double xl = xa < xb ? xa : xb, xh = xa < xb ? xb : xa, zl = za < zb ? za : zb, zh = za < zb ? zb : za;
  // (x - x is NaN for a NaN and for an infinity: the ends must be numbers, and the near end -- the origin or a slab face -- finite)
  const bool sane = (xa - xa) + (za - za) == 0.0 && xb == xb && zb == zb && f >= 0.0 && f <= 1.0;
  ReachRay b;
  if (all || !sane) {
    b.xlo = b.zlo = -__builtin_inff(); b.xhi = b.zhi = __builtin_inff();
  } else if (empty) {
    b.xlo = b.zlo = __builtin_inff(); b.xhi = b.zhi = -__builtin_inff();
  } else {
    const double g = kReachMutant ? 0.0 : 0x1p-40;
    b.xlo = reach_f32_down(fma_(-__builtin_fabs(xl), g, xl) - S); b.xhi = reach_f32_up(fma_(__builtin_fabs(xh), g, xh) + S);
    b.zlo = reach_f32_down(fma_(-__builtin_fabs(zl), g, zl) - S); b.zhi = reach_f32_up(fma_(__builtin_fabs(zh), g, zh) + S);
  }
  return b;
}
// true: the lane does not reach the word {xlo, xhi, zlo, zhi} (false on every NaN)
TOR_HD bool reach_miss(const ReachRay& b, float xlo, float xhi, float zlo, float zhi) {
  return b.xhi < xlo || b.xlo > xhi || b.zhi < zlo || b.zlo > zhi;
}
// The host's side of a word record (tor_scene.cpp build_layout): grow a box end / slab end by g and round it outward
TOR_HD float reach_box_lo(double c, double g) { return kReachMutant ? (float)c : reach_f32_down(c - g * (1.0 + 0x1p-40)); }
TOR_HD float reach_box_hi(double c, double g) { return kReachMutant ? (float)c : reach_f32_up(c + g * (1.0 + 0x1p-40)); }
TOR_HD double reach_slab_lo(double y, double g) { return kReachMutant ? y : fma_(-(__builtin_fabs(y) + g), 0x1p-40, y - g); }
TOR_HD double reach_slab_hi(double y, double g) { return kReachMutant ? y : fma_(__builtin_fabs(y) + g, 0x1p-40, y + g); }

// Does stage one PAY on this segment for this ray?  It leaves the objects in a band of half-width R around the ground track to a
// per-lane stage that costs ~8 times a wave-uniform test per object, so it only pays when the band is thin against the segment:
// a wall of spheres seen edge-on (every centre on the ray's own ground track) would send everything through both stages.  The
// centres' bounding box in xz has extents (Sx, Sz) (host: xsegs[5], xsegs[6]); its width across the track is at most
// E = (|nx| Sx + |nz| Sz) / |n|, and the share of a uniformly filled box inside the band about 2 R / E.  The plane runs when that
// estimate is below 1 / kPlaneGate; the wave takes the majority's vote (the loop is wave-uniform).  A performance decision only:
// either way every object meets a conservative test and every candidate the exact one.
// (gate2 = 4 kPlaneGate^2 travels in KParams; 0 = no gate -- TOR_PLANE=2, the yardstick of the gate itself)
constexpr double kPlaneGate = 16.0;
TOR_HD bool plane_pays(const PlaneRay& pr, double gate2, double rmax2, double sx, double sz) {
  const double e = fma_(__builtin_fabs(pr.nx), sx, __builtin_fabs(pr.nz) * sz);
  return !pr.all && (gate2 * rmax2) * pr.w2 < e * e;
}

}  // namespace tor

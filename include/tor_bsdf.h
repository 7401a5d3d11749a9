/*
 * tor_bsdf.h -- the BSDF query of libtor_mi355x.so, included by tor_render.h (which defines the types used here).
 *
 * ---- value and density of the reference's scatter -------------------------------------------------------------------------------
 * tor_scatter_device / tor_bounce_device SAMPLE Material.scatter (materials.nim:21-96) bit for bit.  This entry answers the two
 * questions a sample cannot: which solid-angle density that scatter gives a direction, and what the material returns for a
 * direction it did NOT sample -- what next-event estimation and multiple importance sampling at a vertex need.  It rests on the
 * reference's own pieces only: Lambertian.scatter (materials.nim:24-30), Metal.scatter (materials.nim:39-47), reflect
 * (rays.nim:27-28), Vec3's dot, cross and unit_vector (vec3s.nim:96-107), random(UnitVector) and random_in_unit_sphere
 * (sampling.nim:45-55).
 *
 * The densities.  Lambertian scatters along n + U with U uniform on the unit sphere: for a unit n the direction w has the density
 * cos / pi, cos = w . n, and the scatter weights the ray by albedo, so f_r cos = albedo * cos / pi.  Metal scatters along
 * r + f B, r = reflect(unit(d_in), n), B uniform in the unit ball, f = fuzz, and keeps the ray -- weighted by albedo -- where the
 * unnormalised direction has a positive dot product with n.  The direction w = (r + f B) / |r + f B| has the density
 *     p(w) = Int_{t : |t w - r| < f} t^2 dt / (4/3 pi f^3)
 * and |t w - r|^2 = t^2 - 2 t b + r . r with b = w . r; r . r - b^2 = |w x r|^2 = s2 for a unit w, so the interval is
 * [b - q, b + q] with h = f^2 - s2, q = sqrt(h), cut at t > 0.  For b - q > 0 the difference of the cubes factors without
 * cancellation, p = q (3 b^2 + h) / (2 pi f^3); for a ball that holds the origin (only with f >= |r|) the interval starts at 0,
 * p = (b + q)^3 / (4 pi f^3).  f_r cos = albedo * p(w) * [accepted].  Metal with fuzz == 0 and Dielectric are Dirac: no density.
 *
 * tor_bsdf_eval_device.  All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly this order; sums and
 * products of three terms associate from the left ((a + b) + c, (a * b) * c).  dot(u, v) = u.x * v.x + u.y * v.y + u.z * v.z
 * (vec3s.nim:96-98); unit_vector(u) = u * (1.0 / sqrt(dot(u, u))) per component (vec3s.nim:93-94, 106-107, the operations of
 * tor_scatter_device); pi = 3.141592653589793.  Per listed item i the query reads d_in[i].direction, d_hits[i].normal and .object,
 * d_out[i].direction and nothing else of the three records; the normal and the object are taken as given, exactly as
 * tor_scatter_device takes them (a host may have perturbed the normal: nothing is normalised on its behalf), and `out` may have
 * any positive finite length, so the rays of tor_light_sample_device, tor_env_sample_device and tor_scatter_device go straight
 * in.  The cases, in this order:
 *   object outside [0, n_objects)        kind = TOR_BSDF_NONE, value = (0, 0, 0), pdf = 0   (tor_scatter_device: a miss)
 *   Dielectric, or Metal whose stored fuzz == 0 (so -0.0 too)
 *                                        kind = TOR_BSDF_DELTA, value = (0, 0, 0), pdf = 0
 *   otherwise                            kind = TOR_BSDF_DENSITY, pdf as below, value = albedo * pdf per component
 *     oo   = dot(out, out).  If !(oo > 0) or oo is not finite (oo == +inf): pdf = 0.  (A zero, a NaN, an infinite `out`, one so
 *            short that oo underflows to 0 or so long that it overflows: no direction.)
 *     w    = out * (1.0 / sqrt(oo)) per component
 *     gate = dot(out, n) > 0 on the caller's UNNORMALISED out: the very test Metal.scatter applies to `scattered`
 *            (materials.nim:39-47), so a ray the scatter accepted is accepted here and an absorbed one gets 0.  If !gate: pdf = 0.
 *     Lambertian:  c = dot(w, n); pdf = c > 0 ? c / pi : 0
 *     Metal:       ud = unit_vector(in); r = ud - n * (2.0 * dot(ud, n)) per component   (rays.nim:27-28, as the scatter forms them)
 *                  f  = abs(fuzz), the material's stored fuzz (the scatter multiplies B by the stored value; -B is B in law)
 *                  b  = dot(w, r)
 *                  x  = (w.y * r.z - w.z * r.y,  w.z * r.x - w.x * r.z,  w.x * r.y - w.y * r.x)   (vec3s.nim:100-104)
 *                  s2 = dot(x, x); h = f * f - s2
 *                  if !(h > 0): pdf = 0
 *                  else q = sqrt(h); lo = b - q; hi = b + q; f3 = f * f * f
 *                    if lo > 0:       pdf = (q * (3.0 * b * b + h)) / (2.0 * pi * f3)    (3.0 * b * b = (3.0 * b) * b; 2.0 * pi first)
 *                    else if hi > 0:  pdf = (hi * hi * hi) / (4.0 * pi * f3)             (4.0 * pi first)
 *                    else             pdf = 0
 *   A NaN that reaches a comparison makes it false, so a NaN in `out`, `in`, the normal or the fuzz gives pdf = 0 by the rules
 *   above; a NaN that reaches value (a NaN albedo, or an infinite albedo times pdf = 0) is a NaN whose sign and payload are not
 *   defined.  Every other bit is what IEEE 754 gives for these operations; nothing is special-cased.  In particular: f * f
 *   underflows to 0 for f below 1.5e-162 (a denormal fuzz among them), so h = -s2 is never > 0 and pdf = 0; f3 underflows to 0
 *   for f below about 1.7e-108 while f * f does not, so there pdf = +inf wherever h > 0 (and value = albedo * inf, NaN for a
 *   zero albedo).  And since the rounding of w x r can leave s2 of the order 1e-33 even for out == r exactly, a lobe with f below
 *   about 1e-16 is narrower than float64 resolves: the query then returns 0 for the scatter's own direction.  For such a
 *   material the honest treatment is the mirror's (treat it as Dirac); the query does not decide that on the caller's behalf.
 *   The Lambertian density is exact for a unit normal only, the Metal density for any normal (it is the density of r + f B
 *   whatever r is); neither checks it.
 * d_value: 3 float64 per item; d_pdf: one; d_kind (nullable): one int32.  The query draws nothing and changes no state.
 * d_list / n_list exactly as tor_light_pdf_device treats them: NULL = every item (n_list must be n); entries outside [0, n) are
 * skipped; entries must be unique; items that are not listed keep what the outputs hold; n_list == 0 and n == 0 are no-ops.
 * Asynchronous on hip_stream, one stream per context as for the other queries.  tor_last_note(): "bsdf eval".
 * TOR_ERR_INVALID_ARGUMENT (nothing written), tested in this order: NULL ctx, n < 0, n_list < 0, a NULL list with n_list != n;
 * NULL d_in, d_hits, d_out, d_value or d_pdf with work to do; a context without a scene.
 * tor_bsdf_eval_host: the same on host arrays, blocking (every array copied in, the query, the outputs copied out); it waits for
 * the context's last render launch and last query as tor_light_pdf_host does.
 */
#ifndef TOR_BSDF_H
#define TOR_BSDF_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum { TOR_BSDF_NONE = 0, TOR_BSDF_DENSITY = 1, TOR_BSDF_DELTA = 2 };

TOR_API int tor_bsdf_eval_device(TorContext* ctx, int64_t n, const TorRay* d_in, const TorHit* d_hits, const TorRay* d_out,
                                 const int32_t* d_list, int64_t n_list, double* d_value, double* d_pdf, int32_t* d_kind,
                                 void* hip_stream);
TOR_API int tor_bsdf_eval_host(TorContext* ctx, int64_t n, const TorRay* in, const TorHit* hits, const TorRay* out,
                               const int32_t* list, int64_t n_list, double* value, double* pdf, int32_t* kind);

#ifdef __cplusplus
}
#endif

#endif /* TOR_BSDF_H */

/*
 * tor_media.h -- participating-media queries of libtor_mi355x.so, included by tor_render.h (which defines the types used here).
 *
 * ---- fog, smoke and haze: the space between the surfaces ---------------------------------------------------------------------------
 * Every other query treats the space between surfaces as empty.  These entries are the pieces of a volumetric integrator over
 * homogeneous media bounded by spheres -- the book's constant_medium with its isotropic phase function, the chapter after the
 * reference's moving spheres: the march along a ray up to an optical-depth budget, the isotropic scatter at a collision, and plain
 * uniforms from a path's stream (free-flight sampling and Russian roulette need a uniform that no sampler has consumed for a
 * purpose of its own).  The library stays free of log and exp: the caller turns a uniform into the budget tau (-log1p(-u)) and a
 * depth into a transmittance (exp(-depth)), as tor_env.h stays free of atan2.  Everything computed here is + - * /, sqrt and the
 * portable sin / cos of the scatter, so every bit is defined.  They rest on the reference's own pieces only: the sphere test
 * (spheres.nim:29-48, moving_spheres.nim:39-66), the generator and its uniform01 (support/rng.nim:58-74, 129-133) and
 * random_unit_vector (sampling.nim:51-55 as the library evaluates it).
 *
 * tor_scene_media: the media table of the context, from HOST arrays.  objects: n_media indices into the uploaded list, unique,
 * each in [0, n_objects): these spheres and moving spheres are the media's boundaries.  They are ordinary scene objects; a host
 * hides them from the surface queries with visibility groups (tor_scene_groups).  sigma: the extinction per unit length of each
 * medium, finite and >= 0.  albedo: nullable (NULL: 1, 1, 1 for every medium), 3 per medium, finite and >= 0.  n_media == 0 clears
 * the table; so does every tor_scene_upload that replaces the scene (an upload of a byte-identical list is a no-op and keeps it).
 * The call waits for the context's last query.  TOR_ERR_INVALID_ARGUMENT, and nothing changes, for a NULL ctx, a context without a
 * scene, n_media outside [0, n_objects], n_media > TOR_MEDIA_MAX, NULL objects or sigma with n_media > 0, an index outside the
 * list or listed twice, a sigma or an albedo that is NaN, infinite or negative.  The table is packed into one device record per
 * medium at this call (the centre data of the scene's record, radius * radius, sigma, albedo), so a query reads medium m at one
 * wave-uniform address.
 *
 * tor_media_march_device.  All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly this order; sums of
 * three terms associate from the left ((a + b) + c).  Per listed ray i = (o, d, time) with (t_min, t_max) = d_t_range[i] -- NULL
 * d_t_range means (0.0, +inf), NOT the (0.001, +inf) of the surface queries: a scattered ray starts inside the medium, and no
 * surface is there to be hit again -- and tau = d_tau[i]:
 *   ray       a = d.x * d.x + d.y * d.y + d.z * d.z; len = sqrt(a)
 *   per medium m, in table order: has_m, s0_m, s1_m -- the two roots tor_crossings_device computes for that object, bit for bit,
 *             unclipped:  c = center, or center0 + (center1 - center0) * ((time - time0) / (time1 - time0));  oc = o - c;
 *             half_b = oc.x * d.x + oc.y * d.y + oc.z * d.z;  cc = (oc.x * oc.x + oc.y * oc.y + oc.z * oc.z) - radius * radius;
 *             disc = half_b * half_b - a * cc;  has_m = disc > 0 (strict);  root = sqrt(disc);
 *             s0_m = (-half_b - root) / a;  s1_m = (-half_b + root) / a
 *   refusal   if !(tau >= 0) or !(t_min < t_max):  status = -1, t = t_min, depth = 0, active = 0, rho = 0.
 *   march     otherwise t = t_min, D = 0.0, and repeat AT MOST 2 * n_media + 1 times:
 *               rho = 0.0; A = 0.  For m ascending: if has_m && s0_m <= t && t < s1_m:  rho = rho + sigma_m;  A |= 1 << m.
 *               t_next = t_max.  For m ascending with has_m:  if s0_m > t && s0_m < t_next: t_next = s0_m;
 *                                                               if s1_m > t && s1_m < t_next: t_next = s1_m.
 *               step = rho > 0 ? rho * ((t_next - t) * len) : 0.0         (written this way 0 * inf never occurs)
 *               rem = tau - D
 *               if rho > 0 && rem < step (strict): a collision.  t_c = t + (rem / rho) / len; if t_next < t_c: t_c = t_next.
 *                   status = 1, t = t_c, depth = tau, active = A, rho = rho.  Stop.
 *               D = D + step.  If !(t_next < t_max): stop.  Otherwise t = t_next.
 *   escaped   status = 0, t = t_max, depth = D, active = 0, rho = 0.
 *   With tau = +inf nothing collides and depth is the optical depth of the segment: exp(-depth) is its transmittance.
 *   Termination.  t changes only to a t_next with t < t_next < t_max that is one of the 2 * n_media roots, so t rises strictly
 *   through a set of at most 2 * n_media values; the iteration after the last of them finds t_next = t_max and stops.  That is at
 *   most 2 * n_media + 1 iterations, the loop's bound: the bound is never what ends a march, and no comparison that goes wrong
 *   (a NaN anywhere) can make a march run on.  Overlapping media add their densities, in table order -- which is why the bits are
 *   defined, and why the table is capped at TOR_MEDIA_MAX = 64: the active set is returned as one word.
 *   outputs   d_status[i] (int32), d_t[i], d_depth[i], d_active[i] (uint64), d_rho[i] (d_rho nullable).
 * d_list / n_list exactly as tor_light_sample_device treats them: NULL = every ray (n_list must be n_rays); entries outside
 * [0, n_rays) are skipped; entries must be unique; rays that are not listed keep what the outputs hold; n_list == 0 and
 * n_rays == 0 are no-ops.  Asynchronous on hip_stream, one stream per context as for the other queries; a query leaves every
 * render state alone.  tor_last_note(): "media march: 5 media".  TOR_ERR_INVALID_ARGUMENT (nothing written), tested in this order:
 * NULL ctx, n_rays < 0, n_list < 0, a NULL list with n_list != n_rays; NULL d_rays, d_tau, d_status, d_t, d_depth or d_active with
 * work to do; a context without a scene; an empty media table.  tor_media_march_host: the same on host arrays, blocking (every
 * array copied in, the query, the outputs copied out); it waits for the context's last render launch and last query.
 *
 * tor_media_scatter_device: the isotropic scatter at a collision.  Per listed ray i with t = d_t[i], active = d_active[i] and state
 * g = d_rng[i]:
 *   draws     v = random_unit_vector(g) (sampling.nim:51-55): a = uniform01(g) * (2.0 * 3.141592653589793); z = uniform01(g) * 2.0
 *             + -1.0; r = sqrt(1.0 - z * z); (s, c) = the portable sin and cos of a; v = (r * c, r * s, z).  Exactly two outputs
 *             of the generator, always -- also for an entry that gets no sample.  d_rng[i] is the state after them.
 *   mixture   rho = 0.0; n = (0, 0, 0).  For m ascending over the bits of active: rho = rho + sigma_m; n_c = n_c + sigma_m *
 *             albedo_m,c.   att_c = n_c / rho.
 *   point     p_c = o_c + t * d_c.
 *   outputs   d_rays_out[i] = { p, v, time }, d_att[i] = att.  If active == 0, or it has a bit at or above n_media, or !(rho > 0):
 *             att = 0 and the seven words of the out ray are 0 (the state is still advanced).
 * d_rays_out may be d_rays.  Lists, stream and refusals as above (NULL d_rays, d_t, d_active, d_rng, d_rays_out or d_att);
 * tor_last_note(): "media scatter: 5 media".  tor_media_scatter_host: on host arrays, blocking.
 *
 * tor_rng_uniform_device: d_out[i * n_draws + k] = uniform01(g) for k = 0 .. n_draws - 1, g = d_rng[i], for every listed state;
 * d_rng[i] is left as the state after the draws.  It needs no scene.  Lists and stream as above.  tor_last_note(): "rng uniform: 3
 * draws".  TOR_ERR_INVALID_ARGUMENT, in this order: NULL ctx, n_states < 0, n_list < 0, a NULL list with n_list != n_states;
 * n_draws outside [1, TOR_UNIFORM_MAX_DRAWS]; NULL d_rng or d_out with work to do.  tor_rng_uniform_host: on host arrays, blocking.
 */
#ifndef TOR_MEDIA_H
#define TOR_MEDIA_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define TOR_MEDIA_MAX 64
#define TOR_UNIFORM_MAX_DRAWS 16

TOR_API int tor_scene_media(TorContext* ctx, int64_t n_media, const int32_t* objects, const double* sigma, const double* albedo);
TOR_API int tor_media_march_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const double* d_tau,
                                   const int32_t* d_list, int64_t n_list, int32_t* d_status, double* d_t, double* d_depth,
                                   uint64_t* d_active, double* d_rho, void* hip_stream);
TOR_API int tor_media_march_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const double* tau,
                                 const int32_t* list, int64_t n_list, int32_t* status, double* t, double* depth, uint64_t* active,
                                 double* rho);
TOR_API int tor_media_scatter_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t, const uint64_t* d_active,
                                     TorRng* d_rng, const int32_t* d_list, int64_t n_list, TorRay* d_rays_out, double* d_att,
                                     void* hip_stream);
TOR_API int tor_media_scatter_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t, const uint64_t* active,
                                   TorRng* rng, const int32_t* list, int64_t n_list, TorRay* rays_out, double* att);
TOR_API int tor_rng_uniform_device(TorContext* ctx, int64_t n_states, TorRng* d_rng, const int32_t* d_list, int64_t n_list,
                                   int32_t n_draws, double* d_out, void* hip_stream);
TOR_API int tor_rng_uniform_host(TorContext* ctx, int64_t n_states, TorRng* rng, const int32_t* list, int64_t n_list, int32_t n_draws,
                                 double* out);

#ifdef __cplusplus
}
#endif

#endif /* TOR_MEDIA_H */

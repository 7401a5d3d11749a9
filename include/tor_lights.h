/*
 * tor_lights.h -- direct-light sampling queries of libtor_mi355x.so, included by tor_render.h (which defines the types used here).
 *
 * ---- direct-light sampling: the shadow rays of next-event estimation ------------------------------------------------------------
 * A host that treats objects as emitters (Context.trace(emission=...)) finds a lamp only when a scattered ray happens to hit it;
 * with a small lamp that is the noisiest estimator there is.  These entries are the missing step of a direct-lighting integrator:
 * per shading point they choose one light of a table, sample the cone its sphere subtends and return the shadow segment, ready
 * for tor_occluded_device, with the density of the sampled direction.  They rest on the reference's own pieces only: the
 * generator and its uniform01 (support/rng.nim:58-74, 129-133), MovingSphere.center (moving_spheres.nim:39-44), the portable
 * sin / cos of the scatter (sampling.nim:51-55 as the library evaluates it), Vec3's operations (vec3s.nim).
 *
 * tor_scene_lights: the light table of the context, from HOST arrays.  objects: n_lights indices into the uploaded list, unique,
 * each in [0, n_objects).  weights: nullable (NULL: every weight 1), finite and >= 0 with at least one > 0 -- the caller puts the
 * emitted power there, for example luminance * radius^2.  n_lights == 0 clears the table; so does every tor_scene_upload that
 * replaces the scene (an upload of a byte-identical list is a no-op and keeps it).  The call waits for the context's last query.
 * TOR_ERR_INVALID_ARGUMENT, and nothing changes, for a NULL ctx, a context without a scene, n_lights outside [0, n_objects], NULL
 * objects with n_lights > 0, an index outside the list or listed twice, a weight that is NaN, infinite or negative, or no
 * weight > 0.  The table is packed into one device record per light at this call (centre data of the scene's record, R, R * R,
 * the weight and the running sum of the weights), so a query reads light j at one wave-uniform address.
 *
 * tor_light_sample_device.  All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly this order; sums
 * and products of three terms associate from the left ((a + b) + c).  Per listed point i = (p, time) with state g = d_rng[i]:
 *   draws     u0 = uniform01(g), u1 = uniform01(g), u2 = uniform01(g): exactly three, always, in this order -- also for a point
 *             that gets no sample, so a host can predict the stream.  d_rng[i] is the state after them.
 *   per light j, in table order:
 *             c      = center, or center0 + (center1 - center0) * ((time - time0) / (time1 - time0))   (moving_spheres.nim:39-44,
 *                      the arithmetic of tor_nearest_device)
 *             R      = abs(radius); R2 = R * R
 *             w      = c - p (per component); d2 = w.x * w.x + w.y * w.y + w.z * w.z
 *             inside = !(d2 > R2)                  (so a NaN d2 or R2 counts as inside)
 *             s2     = R2 / d2
 *             m_j    = inside ? 2.0 : s2 / (1.0 + sqrt(1.0 - s2))     (1 - cos(theta_max) without the cancellation)
 *   importance  TOR_LIGHT_BY_WEIGHT: I_j = weight_j.   TOR_LIGHT_BY_SOLID_ANGLE: I_j = weight_j * m_j.
 *   pick      T = 0.0; T = T + I_j for j = 0, 1, ... (sequentially, in table order).  If !(T > 0) or T is not finite: no sample --
 *             light = -1, pdf = 0, the seven words of the ray 0, dist = 0 (the state is still advanced).  Otherwise x = u0 * T and
 *             the pick is the first j with I_j > 0 whose running sum (the same additions in the same order) is > x; if rounding
 *             leaves none, the last j with I_j > 0.  P = I_j / T.
 *   cone      with w, d2, R2, inside, m of the picked light:
 *             k = u1 * m; cos_t = 1.0 - k; sin2 = k * (2.0 - k); sin_t = sqrt(sin2)
 *             (s, c) = the portable sin and cos of u2 * (2.0 * 3.141592653589793)
 *             sd = sqrt(d2); a = w * (1.0 / sd) (per component); if d2 == 0: a = (0, 0, 1)
 *             the branchless orthonormal frame around a:  sg = copysign(1.0, a.z); aa = -1.0 / (sg + a.z); bb = a.x * a.y * aa
 *                 b1 = (1.0 + sg * a.x * a.x * aa,  sg * bb,  (-sg) * a.x)        b2 = (bb,  sg + a.y * a.y * aa,  -a.y)
 *             e1 = sin_t * c; e2 = sin_t * s;  dir = b1 * e1 + b2 * e2 + a * cos_t   (per component, from the left)
 *             h = R2 - d2 * sin2; if !(h > 0): h = 0
 *             t = sd * cos_t - sqrt(h) outside the sphere, sd * cos_t + sqrt(h) inside
 *   outputs   d_rays[i] = { origin p, direction dir * t, time }: parameter 1.0 is the sampled surface point, the convention of
 *             shadow segments -- the ray goes straight into tor_occluded_masked_device with range (t_min, 1.0) and a mask that
 *             leaves the lamps' group out, or into tor_occluded_device with a range that stops short of 1.
 *             d_pdf[i] = P / ((2.0 * 3.141592653589793) * m): per unit solid angle at p, the selection probability included.
 *             d_light[i] = the picked light's OBJECT index in the uploaded list.  d_dist[i] (d_dist nullable) = t.
 *   With `inside` the same formulas sample the whole sphere of directions (m = 2, pdf = P / (4 pi)): there is no special case.  A
 *   result that is NaN (a NaN coordinate) is a NaN; its sign and payload are not defined.  TOR_LIGHT_BY_WEIGHT may pick a light
 *   with m = 0 (radius 0, or so far away that s2 underflows): its pdf is +inf, as a point light's.
 * d_list / n_list exactly as tor_bounce_device treats them: NULL = every point (n_list must be n_points); entries outside
 * [0, n_points) are skipped; entries must be unique; points that are not listed keep what the outputs and d_rng hold; n_list == 0
 * and n_points == 0 are no-ops.  Asynchronous on hip_stream, one stream per context as for the other queries; a query leaves every
 * render state alone.  tor_last_note(): "light sample: by weight" | "light sample: by solid angle".  TOR_ERR_INVALID_ARGUMENT
 * (nothing written), tested in this order: NULL ctx, n_points < 0, n_list < 0, a NULL list with n_list != n_points; a strategy
 * that is neither; NULL d_points, d_rng, d_rays, d_pdf or d_light with work to do; a context without a scene; an empty light table.
 * tor_light_sample_host: the same on host arrays, blocking (every array copied in, the query, the outputs copied out); it waits
 * for the context's last render launch and last query as tor_hit_host does.
 *
 * tor_light_pdf_device: the density tor_light_sample_device gives the direction from point i towards the light whose object index
 * is d_object[i] (int32 per point: the object a ray from that point is taken to have reached) -- what multiple importance
 * sampling needs, and what keeps an emitter from being counted twice.  d_pdf[i] = (I_j / T) / ((2.0 * 3.141592653589793) * m_j)
 * with the identical per-light arithmetic and the identical sequential total; 0 if the object is not in the table, if T is not
 * usable or if !(I_j > 0) (the sampler never picks such a light).  It draws nothing.  Hence, for every point, the density of
 * (point, d_light of a sample) is that sample's d_pdf in every bit.  Lists, stream, refusals as above (NULL d_points, d_object or
 * d_pdf); tor_last_note(): "light pdf: by weight" | "light pdf: by solid angle".  tor_light_pdf_host: on host arrays, blocking.
 */
#ifndef TOR_LIGHTS_H
#define TOR_LIGHTS_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum { TOR_LIGHT_BY_WEIGHT = 0, TOR_LIGHT_BY_SOLID_ANGLE = 1 };

TOR_API int tor_scene_lights(TorContext* ctx, int64_t n_lights, const int32_t* objects, const double* weights);
TOR_API int tor_light_sample_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, TorRng* d_rng, const int32_t* d_list,
                                    int64_t n_list, int32_t strategy, TorRay* d_rays, double* d_pdf, int32_t* d_light, double* d_dist,
                                    void* hip_stream);
TOR_API int tor_light_sample_host(TorContext* ctx, int64_t n_points, const TorPoint* points, TorRng* rng, const int32_t* list,
                                  int64_t n_list, int32_t strategy, TorRay* rays, double* pdf, int32_t* light, double* dist);
TOR_API int tor_light_pdf_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, const int32_t* d_object,
                                 const int32_t* d_list, int64_t n_list, int32_t strategy, double* d_pdf, void* hip_stream);
TOR_API int tor_light_pdf_host(TorContext* ctx, int64_t n_points, const TorPoint* points, const int32_t* object, const int32_t* list,
                               int64_t n_list, int32_t strategy, double* pdf);

#ifdef __cplusplus
}
#endif

#endif /* TOR_LIGHTS_H */

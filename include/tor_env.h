/*
 * tor_env.h -- environment-light queries of libtor_mi355x.so, included by tor_render.h (which defines the types used here).
 *
 * ---- the environment map: the sky as an emitter a host integrator can evaluate, importance-sample and weigh ---------------------
 * The reference's only light source is its sky (render.nim:41-45), and tor_sky_device can only return that gradient.  These
 * entries give a context an environment MAP of its own and the three operations a direct-lighting integrator needs of an
 * emitter: the colour a ray's direction sees (tor_env_eval_device: the sky lookup of the rays that missed), a direction drawn
 * in proportion to the map's importance with its solid-angle density (tor_env_sample_device: the shadow ray towards the bright
 * part of the sky), and the density of ANY direction (tor_env_eval_device's d_pdf: what multiple importance sampling needs).
 * The map is OCTAHEDRAL: the unit sphere is projected onto the octahedron |x| + |y| + |z| = 1, whose upper half (y >= 0, y up as
 * in the reference's sky) is the inner diamond |s| + |t| <= 1 of the square [-1, 1]^2 and whose lower half is folded outwards
 * into the four corners.  Both directions of that mapping need only + - * /, abs, copysign and one sqrt -- no atan2 and no acos,
 * of which the library has no portable bit-reproducible versions --, and its Jacobian is closed-form: for the octahedron point
 * p of (s, t), d(omega) = ds dt / |p|^3.
 *
 * All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly this order; sums and products of three
 * terms associate from the left ((a + b) + c).
 *
 * map       n x n texels, 1 <= n <= 2048, indexed by row r and column c.  With h = 2.0 / n, a position (a, b) in [0, 1)^2 inside
 *           texel (r, c) is   s = ((double)c + a) * h - 1.0      t = ((double)r + b) * h - 1.0
 * decode(s, t)
 *           py = (1.0 - |s|) - |t|
 *           if py >= 0: px = s, pz = t;   else: px = copysign(1.0 - |t|, s), pz = copysign(1.0 - |s|, t)
 *           len = sqrt(px * px + py * py + pz * pz); inv = 1.0 / len; d = (px * inv, py * inv, pz * inv)
 * encode(d), for any direction, not necessarily unit
 *           L1 = |dx| + |dy| + |dz|.  If L1 is 0, NaN or infinite the direction is UNUSABLE: colour 0, pdf 0, texel -1.
 *           q = (dx / L1, dy / L1, dz / L1)
 *           if dy >= 0: s = qx, t = qz;   else: s = copysign(1.0 - |qz|, qx), t = copysign(1.0 - |qx|, qz)
 *           c = clamp((int)floor((s + 1.0) * (0.5 * n)), 0, n - 1), and r likewise from t
 *           len = sqrt(qx * qx + qy * qy + qz * qz)
 *
 * tor_scene_environment: the map of the context, from HOST arrays.  rgb: n * n * 3 float64 in [row][col][channel] order, every
 * value finite and >= 0.  importance: nullable, n * n values, finite and >= 0, taken as given per texel.  With NULL importance
 * the default is I = lum * w with   lum = (0.2126 * R + 0.7152 * G) + 0.0722 * B   and   w = 1.0 / ((len * len) * len)   for
 * decode's len at the texel centre a = b = 0.5 (the texel's luminance times, up to the constant h * h, its solid angle).  The
 * running sums within a row are sequential in ascending c: cum[r][c]; the row total is S_r = cum[r][n - 1].  The marginal running
 * sums M_r of the S_r are sequential in ascending r; the total is T = M_(n-1).  TOR_ERR_INVALID_ARGUMENT, and nothing changes,
 * for a NULL ctx, n outside [0, 2048], NULL rgb with n > 0, a value that is not finite or is negative, or a T that is not > 0 and
 * finite.  n == 0 clears the map.  The call waits for the context's last query.  The map does NOT depend on the scene: it
 * survives every tor_scene_upload (an animation uploads a scene per frame), and the queries below need no uploaded scene.
 *
 * tor_env_sample_device.  Per listed point i = (p, time) with state g = d_rng[i]:
 *   draws     u0 = uniform01(g), u1 = uniform01(g), u2 = uniform01(g), u3 = uniform01(g): exactly four, always, in this order
 *             (support/rng.nim:58-74, 129-133); d_rng[i] is the state after them.
 *   row       x = u0 * T.  The row is the first r with M_r > x (such an r has S_r > 0: running sums of non-negatives never
 *             decrease); if rounding leaves none, the last r with S_r > 0.
 *   column    y = u1 * S_row.  The column is the first c with cum[row][c] > y; if none, the last c with I[row][c] > 0.
 *   direction a = u2, b = u3, then (s, t) of texel (row, col) and decode.
 *   density   P = I[row][col] / T;  A = ((double)n * (double)n) * 0.25;  pdf = (P * A) * ((len * len) * len)   (decode's len)
 *   outputs   d_rays[i] = { origin p, direction d (unit), time }: it goes straight into tor_occluded_device with range
 *             (t_min, +inf).  d_pdf[i] = pdf, per unit solid angle.  d_texel[i] = row * n + col (int32).  d_color[i] (d_color
 *             nullable) = the texel's RGB.
 *   A NaN in the point propagates into the origin only: the direction does not depend on the point.
 *
 * tor_env_eval_device.  Per listed ray i: encode(direction), then d_color[i] = the texel's RGB; d_pdf[i] (d_pdf nullable) =
 * (P * A) * ((len * len) * len) with the same P and A and encode's len; d_texel[i] (d_texel nullable) = r * n + c.  An unusable
 * direction gives colour 0, pdf 0 and texel -1.  Nothing is drawn.  This one entry is the sky lookup for the rays that missed
 * and the density of a scattered direction; for a sampled direction it returns the sampler's texel, and the sampler's pdf up to
 * the roundings of the round trip (the two len differ by a few units in the last place).
 *
 * d_list / n_list exactly as tor_bounce_device treats them: NULL = every point (n_list must be n_points); entries outside
 * [0, n_points) are skipped; entries must be unique; points that are not listed keep what the outputs and d_rng hold; n_list == 0
 * and n_points == 0 are no-ops.  Asynchronous on hip_stream, one stream per context as for the other queries; a query leaves
 * every render state alone.  tor_last_note(): "env sample" | "env eval".  TOR_ERR_INVALID_ARGUMENT (nothing written), tested in
 * this order: NULL ctx, n_points < 0, n_list < 0, a NULL list with n_list != n_points; NULL d_points, d_rng, d_rays, d_pdf or
 * d_texel (the sampler), NULL d_rays or d_color (the evaluation) with work to do; a context without a map.
 * tor_env_sample_host / tor_env_eval_host: the same on host arrays, blocking (every array copied in, the query, the outputs
 * copied out); they wait for the context's last render launch and last query as tor_hit_host does.
 */
#ifndef TOR_ENV_H
#define TOR_ENV_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum { TOR_ENV_MAX_SIDE = 2048 };

TOR_API int tor_scene_environment(TorContext* ctx, int64_t n, const double* rgb, const double* importance);
TOR_API int tor_env_sample_device(TorContext* ctx, int64_t n_points, const TorPoint* d_points, TorRng* d_rng, const int32_t* d_list,
                                  int64_t n_list, TorRay* d_rays, double* d_pdf, int32_t* d_texel, double* d_color, void* hip_stream);
TOR_API int tor_env_sample_host(TorContext* ctx, int64_t n_points, const TorPoint* points, TorRng* rng, const int32_t* list,
                                int64_t n_list, TorRay* rays, double* pdf, int32_t* texel, double* color);
TOR_API int tor_env_eval_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const int32_t* d_list, int64_t n_list,
                                double* d_color, double* d_pdf, int32_t* d_texel, void* hip_stream);
TOR_API int tor_env_eval_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const int32_t* list, int64_t n_list, double* color,
                              double* pdf, int32_t* texel);

#ifdef __cplusplus
}
#endif

#endif /* TOR_ENV_H */

/*
 * tor_camera.h -- light-tracing queries of libtor_mi355x.so, included by tor_render.h (which defines the types used here).
 *
 * ---- light tracing: emit from the lights, connect to the camera ------------------------------------------------------------------
 * tor_light_sample_device samples a lamp TOWARDS, from a shading point, and tor_camera_rays_device maps (pixel, draws) to a ray.
 * These two entries are their inverses: tor_light_emit_device starts a path ON a lamp of the light table (tor_lights.h), and
 * tor_camera_connect_device tells for a world point which pixel it lands in, through which lens point, and with what measurement
 * weight -- the splats Film.deposit takes.  They rest on the reference's own pieces only: the camera (cameras.nim:47-57, whose
 * struct TorCamera mirrors), the generator, its uniform01 and random(float64, lo, hi) (support/rng.nim), MovingSphere.center
 * (moving_spheres.nim:39-44), the portable sin / cos of the scatter as the library evaluates it, and the branchless frame of
 * tor_lights.h.
 *
 * All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly the order written; sums and products of
 * three terms associate from the left ((a + b) + c); a . b is (a.x * b.x + a.y * b.y) + a.z * b.z; an operation on vectors is
 * the operation per component.  A result that is NaN is a NaN; its sign and payload are not defined.
 *
 * tor_camera_connect_device.  Per camera and frame, once (H = horizontal, V = vertical, llc = lower_left_corner):
 *   fd = (origin - llc) . w          the focus distance (cameras.nim: llc = origin - H / 2 - V / 2 - w * fd, and u, v are normal to w)
 *   HH = H . H; VV = V . V
 *   K  = fd * fd * (double)(ncols - 1) * (double)(nrows - 1) / (sqrt(HH) * sqrt(VV))
 * Per listed point i = (y, time) with state g = d_rng[i]:
 *   draws     u0 = uniform01(g), u1 = uniform01(g): exactly two, always, in this order -- also for a pinhole camera and for a
 *             point that cannot be connected, so a host predicts the stream without a read-back.  d_rng[i] is the state after them.
 *   lens      r = sqrt(u0); (sn, cs) = the portable sin and cos of u1 * (2.0 * 3.141592653589793)
 *             lr = lens_radius * r; rd = (lr * cs, lr * sn)           uniform over the lens disk (NOT the reference's rejection
 *             x = origin + u * rd.x + v * rd.y                         sampler, whose draw count varies); d_lens[i] = rd (nullable)
 *   geometry  e = y - x; z = -(e . w)                                  the depth along the view direction
 *             k = fd / z; F = x + e * k; q = F - llc                   where the line x -> y meets the focus plane
 *             s = (q . H) / HH; t = (q . V) / VV
 *             a = s * (double)(ncols - 1); b = t * (double)(nrows - 1); col = floor(a); row = floor(b)
 *             -- the exact inverse of tor_camera_rays_device's u = (col + U) / (ncols - 1), v = (row + U) / (nrows - 1), row 0 at
 *             the bottom.
 *             len = sqrt(e . e); z3 = z * z * z; f = K * len / z3
 *   valid     (z > 0) and (a >= 0) and (a < ncols) and (b >= 0) and (b < nrows) and (z3 < +inf) and (f >= 0) and (f < +inf): a
 *             comparison with a NaN fails, so a point on or behind the lens plane, outside the frame, or with anything non-finite
 *             (a, b, z3 or f) is not valid.
 *   outputs   valid: d_pixel[i] = row * ncols + col; d_rays[i] = { origin y, direction x - y, time } -- parameter 1.0 is the
 *             lens point, the convention of shadow segments, so the ray goes straight into tor_occluded_device with range
 *             (t_min, 1.0); d_factor[i] = f.   Not valid: d_pixel[i] = -1, d_factor[i] = 0, the seven words of the ray 0.
 *             d_lens[i] and d_rng[i] are written either way.
 * The factor is a density.  The reference's pixel j averages the radiance arriving along its camera rays: (s, t) uniform over the
 * pixel's cell, of area 1 / ((ncols - 1) (nrows - 1)), and x uniform over the lens, p_lens = 1 / (pi lens_radius^2):
 *     I_j = (ncols - 1) (nrows - 1) Int_cell ds dt Int_lens p_lens dA_x  L(x <- F(s, t)).
 * F = llc + s H + t V lies on the focus plane at distance fd / cos(theta) from x (theta: the angle to -w), so the solid angle at x
 * is d(omega) = |H| |V| cos^3(theta) / fd^2 ds dt, and d(omega) = cos_y dA_y / d^2 for the surface at y (d = |e|).  Hence
 *     I_j = Int dA_x Int dA_y  W_j(x, y) cos(theta) cos_y / d^2  L(y -> x),  W_j cos(theta) = (ncols - 1)(nrows - 1) fd^2 p_lens /
 *     (|H| |V| cos^3(theta)) inside pixel j's cone.  With x drawn by p_lens and cos(theta) = z / d:
 *     W_j cos(theta) / p_lens / d^2 = fd^2 (ncols - 1)(nrows - 1) / (|H| |V|) * d / z^3 = f.
 * A path vertex at y with throughput beta, BSDF value fs and cosine cos_y towards x adds beta * fs * cos_y * f to pixel j's
 * radiance estimate when the segment is free.  The limit lens_radius -> 0 is the pinhole: the same f.
 * The query does not look at the shutter interval: a light path takes its time from the emission below.
 * d_list / n_list exactly as tor_light_sample_device treats them: NULL = every point (n_list must be n_points); entries outside
 * [0, n_points) are skipped; entries must be unique; points that are not listed keep what the outputs and d_rng hold; n_list == 0
 * and n_points == 0 are no-ops.  Asynchronous on hip_stream; it reads no scene and no other state of the context (as
 * tor_camera_rays_device), so it works on a context without a scene.  tor_last_note(): "camera connect: pinhole" (lens_radius
 * == 0) | "camera connect: thin lens".  TOR_ERR_INVALID_ARGUMENT (nothing written), tested in this order: NULL ctx or cam; nrows
 * or ncols below 2; n_points < 0, n_list < 0; a NULL list with n_list != n_points; a camera whose fd, HH or VV is not finite and
 * > 0, or whose lens_radius is negative or not finite; NULL d_points, d_rng, d_rays, d_pixel or d_factor with work to do.
 * tor_camera_connect_host: the same on host arrays, blocking (every array copied in, the query, the outputs copied out).
 *
 * tor_light_emit_device, on the table set by tor_scene_lights.  Per listed path i with state g = d_rng[i]:
 *   draws     exactly six, always, in this order: time = random(float64, time_lo, time_hi) of the reference from one output, as
 *             the camera's rays compute it (d = uniform01; v = d * (time_hi - time_lo) + time_lo; v <= time_lo ? time_lo : v);
 *             then u0 .. u4 = uniform01(g): the pick, two for the position, two for the direction.  The host passes the
 *             camera's shutter interval; time_lo == time_hi is allowed.
 *   pick      by weight only.  T = the table's total (the running sum of the last light, summed sequentially when the table was
 *             set); x = u0 * T; the pick j is the first light whose running sum is > x -- the running sums never decrease, so it
 *             is what a binary search finds, and a light of weight 0 is never the first --; if rounding leaves none, the last
 *             light of weight > 0.  P = weight_j / T.
 *   position  c = center, or center0 + (center1 - center0) * ((time - time0) / (time1 - time0)) at the drawn time
 *             R = abs(radius); R2 = R * R
 *             zc = 1.0 - 2.0 * u1; rr = sqrt(4.0 * u1 * (1.0 - u1))          (no 1 - zc^2: no cancellation at the poles)
 *             (sn, cs) = the portable sin and cos of u2 * (2.0 * 3.141592653589793)
 *             n = (rr * cs, rr * sn, zc); y = c + n * R
 *   direction cosine-weighted about n: sin_t = sqrt(u3); cos_t = sqrt(1.0 - u3)
 *             (s4, c4) = the portable sin and cos of u4 * (2.0 * 3.141592653589793)
 *             the branchless frame of tor_lights.h around n:  sg = copysign(1.0, n.z); aa = -1.0 / (sg + n.z); bb = n.x * n.y * aa
 *                 b1 = (1.0 + sg * n.x * n.x * aa,  sg * bb,  (-sg) * n.x)        b2 = (bb,  sg + n.y * n.y * aa,  -n.y)
 *             e1 = sin_t * c4; e2 = sin_t * s4;  dir = b1 * e1 + b2 * e2 + n * cos_t
 *   outputs   d_rays[i] = { origin y, direction dir, time }; d_normal[i] = n (3 float64); d_light[i] = the picked light's OBJECT
 *             index in the uploaded list; d_pdf[2 i] = P / ((4.0 * 3.141592653589793) * R2): per unit area of the lamp, the
 *             pick included, +inf for R == 0 (the point-light convention); d_pdf[2 i + 1] = cos_t / 3.141592653589793: per unit
 *             solid angle.
 * For a lamp of uniform radiance Le the path leaves with beta = Le * cos_t / (pdf_area * pdf_dir) = Le * pi / pdf_area.
 * Lists and stream as above (one stream per context as for the other queries on the light table).  tor_last_note(): "light emit:
 * by weight".  TOR_ERR_INVALID_ARGUMENT (nothing written), tested in this order: NULL ctx, n_paths < 0, n_list < 0, a NULL list
 * with n_list != n_paths; a time range that is not finite or has time_lo > time_hi; NULL d_rng, d_rays, d_normal, d_light or d_pdf
 * with work to do; a context without a scene; an empty light table.  tor_light_emit_host: on host arrays, blocking.
 */
#ifndef TOR_CAMERA_H
#define TOR_CAMERA_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

TOR_API int tor_camera_connect_device(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int64_t n_points,
                                      const TorPoint* d_points, TorRng* d_rng, const int32_t* d_list, int64_t n_list, TorRay* d_rays,
                                      int32_t* d_pixel, double* d_factor, double* d_lens, void* hip_stream);
TOR_API int tor_camera_connect_host(TorContext* ctx, const TorCamera* cam, int32_t nrows, int32_t ncols, int64_t n_points,
                                    const TorPoint* points, TorRng* rng, const int32_t* list, int64_t n_list, TorRay* rays,
                                    int32_t* pixel, double* factor, double* lens);
TOR_API int tor_light_emit_device(TorContext* ctx, int64_t n_paths, TorRng* d_rng, const int32_t* d_list, int64_t n_list, double time_lo,
                                  double time_hi, TorRay* d_rays, double* d_normal, int32_t* d_light, double* d_pdf, void* hip_stream);
TOR_API int tor_light_emit_host(TorContext* ctx, int64_t n_paths, TorRng* rng, const int32_t* list, int64_t n_list, double time_lo,
                                double time_hi, TorRay* rays, double* normal, int32_t* light, double* pdf);

#ifdef __cplusplus
}
#endif

#endif /* TOR_CAMERA_H */

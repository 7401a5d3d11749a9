/*
 * tor_grid.h -- heterogeneous media of libtor_mi355x.so: density grids marched cell by cell, exactly.  Included by tor_render.h
 * (which defines the types used here) after tor_phase.h.
 *
 * ---- a smoke plume, a cloud, a fog bank that thins with height -------------------------------------------------------------------
 * The media of tor_media.h are balls of one sigma.  A density grid refines ONE medium of the media table: medium m keeps its
 * boundary sphere, sigma_m, albedo and g_m, and the local extinction at a point is sigma_m * density[cell] inside both sphere and box, 0
 * elsewhere.  The march is regular tracking: an exact walk through the piecewise-constant density, one 3-D DDA step at a time, so
 * the library stays free of log, exp and random draws -- + - * /, sqrt, floor and compares, every bit defined.  (Delta tracking
 * would take a logarithm per step and a data-dependent number of draws.)
 *
 * One grid medium is marched per call.  tor_media_scatter_device, tor_phase_sample_device and tor_phase_eval_device weight the
 * active media by their table sigma; a joint march of overlapping heterogeneous media would need local weights, which they do not
 * have.  A path draws an independent free-flight budget per source instead -- the homogeneous table, then each grid medium -- and
 * takes the earliest collision: independent Poisson processes superpose, so this is exact; the winner's active word is 1 << m for a
 * grid medium, or the homogeneous word, and for both the scatter and phase entries are correct as they are.  Optical depths of a
 * shadow segment simply add.
 *
 * A medium that has a grid contributes through tor_media_grid_march_device only: tor_media_march_device answers on a table with
 * grid media exactly as it would if has_m were false for them.  Without a grid every bit of every answer is as before.
 *
 * tor_scene_media_grid: the grid of medium `medium`, from HOST arrays.  nx x ny x nz cells of float64 density, finite and >= 0;
 * cell (ix, iy, iz) is density[(ix * ny + iy) * nz + iz], the C order of an (nx, ny, nz) array.  box: lo[3] then hi[3], lo < hi,
 * finite, given as OFFSETS FROM THE SPHERE'S CENTRE c(time) -- the grid rides a moving boundary; NULL: the sphere's bounding cube,
 * R = sqrt(radius * radius) of the media record, lo = (-R, -R, -R), hi = (R, R, R).  Stored per grid: h_k = (hi_k - lo_k) / n_k,
 * one float64 division.  Every dimension in [1, TOR_GRID_MAX_DIM], nx * ny * nz <= TOR_GRID_MAX_CELLS.  nx = ny = nz = 0 removes the
 * medium's grid (box and density are not read).  The call waits for the context's last query.  TOR_ERR_INVALID_ARGUMENT, and
 * nothing changes, tested in this order: a NULL ctx, a context without a scene, an empty media table, a medium outside the table,
 * dimensions out of range, too many cells, a NULL density, a box that is non-finite or has !(lo < hi), a density that is NaN,
 * infinite or negative.  Lifecycle: every tor_scene_media call drops all grids (as it resets g), and so does every tor_scene_upload
 * that replaces the scene; a byte-identical upload keeps them, as do tor_scene_lights, tor_scene_environment and
 * tor_scene_media_phase.  The context frees the buffers when it is destroyed.
 *
 * tor_media_grid_info: dims[3] (zeros: the medium has no grid), box[6] (nullable; untouched without a grid), *grid_mask (nullable):
 * bit m set for every medium with a grid.  Refusals: NULL ctx or dims, no scene, no table, a medium outside the table.
 *
 * tor_media_grid_march_device.  All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly this order; sums
 * of three terms associate from the left.  Per listed ray i = (o, d, time), (t_min, t_max) = d_t_range[i] (NULL: (0.0, +inf)) and
 * tau = d_tau[i], for medium m with grid (lo, hi, h, n, density):
 *   ray       a = d.x * d.x + d.y * d.y + d.z * d.z; len = sqrt(a)
 *   sphere    c, oc = o - c, half_b, cc, disc, has, s0, s1 exactly as tor_media.h computes them for medium m
 *   refusal   if !(tau >= 0) or !(t_min < t_max):  status = -1, t = t_min, depth = 0, active = 0, rho = 0, cell = -1.
 *   empty     if !has:                              status = 0, t = t_max, depth = 0, active = 0, rho = 0, cell = -1.
 *   clip      t0 = t_min; t1 = t_max;  if s0 > t0: t0 = s0;  if s1 < t1: t1 = s1
 *             for k = x, y, z:  if d_k == 0:  if !(oc_k >= lo_k && oc_k < hi_k): empty
 *                               else ta = (lo_k - oc_k) / d_k; tb = (hi_k - oc_k) / d_k; (near, far) = d_k > 0 ? (ta, tb) : (tb, ta);
 *                                    if near > t0: t0 = near;  if far < t1: t1 = far
 *             if !(t0 < t1): empty
 *   entry     for k: p = oc_k + t0 * d_k;  f = floor((p - lo_k) / h_k);  if !(f >= 0): f = 0;  if f > n_k - 1: f = n_k - 1;
 *                    i_k = (int)f;  dir_k = d_k > 0 ? 1 : d_k < 0 ? -1 : 0
 *                    tk_k = dir_k == 0 ? +inf : ((lo_k + (i_k + (dir_k > 0 ? 1 : 0)) * h_k) - oc_k) / d_k
 *   walk      t = t0; D = 0.0; repeat AT MOST nx + ny + nz times:
 *               ks = x, tn = tk_x;  if tk_y < tn: ks = y, tn = tk_y;  if tk_z < tn: ks = z, tn = tk_z     (ties to the lower axis)
 *               last = !(tn < t1);  if last: tn = t1
 *               if tn < t: tn = t                                                                         (the guard)
 *               cell = (i_x * ny + i_y) * nz + i_z;  rho = sigma_m * density[cell]
 *               step = rho > 0 ? rho * ((tn - t) * len) : 0.0;   rem = tau - D
 *               if rho > 0 && rem < step (strict): a collision.  t_c = t + (rem / rho) / len; if tn < t_c: t_c = tn.
 *                   status = 1, t = t_c, depth = tau, active = 1 << m, rho = rho, cell = cell.  Stop.
 *               D = D + step;  if last: stop
 *               i_ks += dir_ks;  if i_ks < 0 || i_ks >= n_ks: stop
 *               tk_ks = ((lo_ks + (i_ks + (dir_ks > 0 ? 1 : 0)) * h_ks) - oc_ks) / d_ks;   t = tn
 *   escaped   status = 0, t = t_max, depth = D, active = 0, rho = 0, cell = -1.
 *   Planes come from the index each time, lo_k + j * h_k with the integer j converted exactly: they are not accumulated as
 *   tMax += tDelta, so rounding does not drift with the step count.
 *   The guard.  The entry cell comes from a point, the next plane from an index; within an ulp or two of a plane the two can
 *   disagree and tn falls below t.  Without the guard such a step would subtract depth.  (tests/grid_inputs.py's search_guard: of 4000 rays whose
 *   t_min lies within two ulps of a plane of a dyadic 4 x 4 x 4 grid, tn < t on 190 (4.8 %); on 88 (2.2 %) the depth changes.)
 *   Termination.  Every iteration that does not stop moves ONE index by one in a fixed direction (dir_k never changes), inside
 *   [0, n_k - 1]: at most (nx - 1) + (ny - 1) + (nz - 1) moves and one final iteration.  The bound nx + ny + nz is therefore never
 *   what ends a march, and no comparison that goes wrong (a NaN anywhere) can make one run on.
 *   In bounds.  The index of the density load is clamped into [0, n_k - 1] per axis at entry -- !(f >= 0) catches a NaN -- and
 *   checked at every move before it is used again, so cell lies in [0, nx * ny * nz) by construction, whatever the ray holds.  A
 *   wrong compare is a wrong answer; it is never a fault and never a hang.
 *   outputs   d_status[i] (int32), d_t[i], d_depth[i], d_active[i] (uint64), d_rho[i] (d_rho nullable), d_cell[i] (int32, nullable).
 * Lists, the stream rule and the order of the refusals follow tor_media_march_device: NULL ctx, n_rays < 0, n_list < 0, a NULL list
 * with n_list != n_rays; NULL d_rays, d_tau, d_status, d_t, d_depth or d_active with work to do; a context without a scene; an empty
 * media table; then a medium outside the table, and a medium without a grid.  tor_last_note(): "media grid march: medium 3,
 * 16x16x16".  tor_media_grid_march_host: the same on host arrays, blocking.
 *
 * tor_media_grid_density_device: the density lookup.  Per listed point i = (p, time) = d_points[4 * i ..]: q = p - c(time) (c as
 * above).  The point is outside if (q.x * q.x + q.y * q.y + q.z * q.z) - radius * radius < 0 is false, or any
 * !(q_k >= lo_k && q_k < hi_k): then cell = -1, density = 0.  Otherwise i_k by the entry rule's clamped floor of (q_k - lo_k) / h_k,
 * cell = (i_x * ny + i_y) * nz + i_z, density = density[cell] (the grid's value, not multiplied by sigma_m).  Lists, stream and
 * refusals as above (NULL d_points, d_cell or d_density).  tor_last_note(): "media grid density: medium 3, 16x16x16".
 * tor_media_grid_density_host: on host arrays, blocking.
 */
#ifndef TOR_GRID_H
#define TOR_GRID_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define TOR_GRID_MAX_DIM 1024
#define TOR_GRID_MAX_CELLS 16777216

TOR_API int tor_scene_media_grid(TorContext* ctx, int32_t medium, int32_t nx, int32_t ny, int32_t nz, const double* box,
                                 const double* density);
TOR_API int tor_media_grid_info(TorContext* ctx, int32_t medium, int32_t* dims, double* box, uint64_t* grid_mask);
TOR_API int tor_media_grid_march_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range,
                                        const double* d_tau, int32_t medium, const int32_t* d_list, int64_t n_list, int32_t* d_status,
                                        double* d_t, double* d_depth, uint64_t* d_active, double* d_rho, int32_t* d_cell,
                                        void* hip_stream);
TOR_API int tor_media_grid_march_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const double* tau,
                                      int32_t medium, const int32_t* list, int64_t n_list, int32_t* status, double* t, double* depth,
                                      uint64_t* active, double* rho, int32_t* cell);
TOR_API int tor_media_grid_density_device(TorContext* ctx, int64_t n_points, const double* d_points, int32_t medium,
                                          const int32_t* d_list, int64_t n_list, int32_t* d_cell, double* d_density, void* hip_stream);
TOR_API int tor_media_grid_density_host(TorContext* ctx, int64_t n_points, const double* points, int32_t medium, const int32_t* list,
                                        int64_t n_list, int32_t* cell, double* density);

#ifdef __cplusplus
}
#endif

#endif /* TOR_GRID_H */

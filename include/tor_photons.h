/*
 * tor_photons.h -- the photon-map queries of libtor_mi355x.so, included by tor_render.h (which defines the types used here).
 *
 * ---- density estimation over caller points in world space ------------------------------------------------------------------------
 * tor_deposit_device sums exactly into pixels and tor_nearest_device searches objects; these entries sum exactly over POINTS the
 * caller supplies: light-path vertices are stored as photons {position, power, incoming direction} in a context-owned map, and a
 * gather adds up, per query point, the powers of the photons within a radius -- the two operations photon mapping, (stochastic)
 * progressive photon mapping and vertex merging are built from.  The answer is DEFINED BY BRUTE FORCE over the stored photons; the
 * hashed uniform grid the map is kept in is an exact acceleration that never loses and never repeats a photon (the proof is below).
 *
 * All arithmetic is float64, unfused, with correctly rounded `/`, in exactly the order written; a . b = (a.x * b.x + a.y * b.y) +
 * a.z * b.z; quantize36(v) = (v + 98304.0) - 98304.0, the film's rounding to a multiple of 2^-36 (tor_deposit_device).
 *
 * tor_photons_build_device(ctx, n_photons, d_position, d_power, d_direction, d_list, n_list, radius, hip_stream).
 *   d_position, d_power: 3 float64 per photon; d_direction: 3 float64 per photon, or NULL (the map then holds no directions and a
 *   gather with normals is refused -- unless the build had no work to do, n_photons == 0 or n_list == 0, where no array is read).
 *   The map is COPIED into storage the context owns: the caller's arrays may be released once the stream has passed the call.  It
 *   replaces the context's previous map and, like the environment, belongs to the context, not
 *   to the scene: tor_scene_upload, tor_scene_lights and tor_scene_environment leave it alone.  No scene is needed.
 *   List: d_list NULL = every photon (n_list must be n_photons); else n_list int32 entries, an entry outside [0, n_photons) is
 *   skipped (neither stored nor counted), a repeated entry is stored again -- tor_deposit_device's rules.
 *   R = radius, h = R + R * 2^-20 (two roundings: the product, exact unless it underflows, and the sum): the cell size.
 *   A listed photon is VALID iff every component of its position (and of its direction, if given) is finite, every power channel is
 *   finite and >= 0 (-0.0 passes), and its cell is in range: c_a = floor(p_a / h) per axis a, in range iff |c_a| <= 2^30.  Invalid
 *   photons are dropped and counted (tor_photons_info).  Valid photons are stored with their three int32 cell coordinates.
 *   n_buckets = the smallest power of two >= 2 * max(n_list, 1), clipped to [2^4, 2^26]; the bucket of a cell is
 *       ((uint32)cx * 73856093u ^ (uint32)cy * 19349663u ^ (uint32)cz * 83492791u) & (n_buckets - 1)
 *   in wrapping 32-bit arithmetic ((uint32) of a negative coordinate is its two's complement).  The hash is part of the documented
 *   layout so that a test can construct collisions; the ANSWER of a gather does not depend on it.  The order of the photons inside
 *   a bucket is whatever the scatter's atomics gave and is not defined; no answer depends on it within the bound below.
 *   n_list == 0 (or a list without a valid entry) builds an empty map: it is a map, and every gather from it answers zeros.
 *   TOR_ERR_INVALID_ARGUMENT (nothing written, the previous map kept), tested in this order: NULL ctx; n_photons < 0 or n_list < 0,
 *   or either above 2^30; a NULL list with n_list != n_photons; radius not finite or not > 0, or h not finite; NULL d_position or
 *   d_power with work to do (n_photons > 0 and n_list > 0).  Asynchronous on hip_stream, one stream per context as for the other
 *   queries.  tor_last_note(): "photons build: <n_buckets> buckets".
 *
 * tor_photons_gather_device(ctx, n_points, d_point, d_normal, d_radius, d_list, n_list, kernel, max_value, d_sums, d_count,
 *                           hip_stream).
 *   d_point: 3 float64 per point; d_normal: 3 per point or NULL; d_radius: one per point or NULL; d_sums: 3 float64 per point;
 *   d_count: one int32 per point.  d_list / n_list as tor_bsdf_eval_device treats them: NULL = every point (n_list must be
 *   n_points), entries outside [0, n_points) are skipped, entries must be unique, points that are not listed keep what the outputs
 *   hold.  Per listed point i, with x = point i, n = normal i:
 *     r = d_radius ? d_radius[i] : R.  If !(r >= 0) (a negative or NaN radius): nothing is accepted.  Else r = r < R ? r : R and
 *     r2 = r * r.
 *     Per stored photon j:  e = p_j - x per component;  d2 = e . e.
 *       j is ACCEPTED iff d2 < r2 and (d_normal == NULL or dir_j . n < 0.0).  A comparison with a NaN fails, so a non-finite point,
 *       a NaN normal, d2 == r2 and dir . n == 0 all reject.
 *       w = 1.0 for kernel == 0 (the constant disc);  w = 1.0 - d2 / r2 for kernel == 1 (Epanechnikov).  The normalisations
 *       1 / (pi r^2) and 2 / (pi r^2) are the host's.
 *       Per channel: q = quantize36(min(power_j[ch] * w, max_value)) with min(a, b) = a < b ? a : b;  sum[ch] += q;  count += 1.
 *   sums[i] and count[i] are OVERWRITTEN for listed points (zeros where nothing is accepted).  0 < max_value <= 128, as for deposits.
 *   Exactness: every addend is a non-negative multiple of 2^-36 that is <= max_value, so every partial sum is at most the final one;
 *   while count * max_value < 2^17 the sums are integers below 2^53 in units of 2^-36 and EXACT in float64: they do not depend on
 *   the order in which the scatter's atomics filled a bucket, on the bucket count, on the split of the points into calls, or on
 *   the GPU.  Past that bound additions round and the order shows; the library cannot check the bound without a read-back of the
 *   counts, so it does not: the caller does (Python: PhotonGather.check_budget).
 *   TOR_ERR_INVALID_ARGUMENT (nothing written), in this order: NULL ctx; n_points < 0 or n_list < 0 (or above 2^31 - 1 workgroups
 *   of 256); a NULL list with n_list != n_points; kernel not 0 or 1; max_value not in (0, 128]; NULL d_point, d_sums or d_count
 *   with work to do (n_points > 0 and n_list > 0); a context that never built a map; d_normal given for a map built without
 *   directions.  No scene is needed.  Asynchronous on hip_stream.  tor_last_note(): "photons gather".
 *
 * tor_photons_info(ctx, out[4]): blocking (it waits for the context's last query); out = {stored, dropped, n_buckets, the largest
 *   bucket's photon count}.  TOR_ERR_INVALID_ARGUMENT: NULL ctx or out, or a context that never built a map.
 * tor_photons_build_host / tor_photons_gather_host: the same on host arrays, blocking (every array copied in, the call, the outputs
 *   copied out -- the outputs in too, since unlisted points keep what the caller holds), as tor_nearest_host does it.
 *
 * ---- why the 27 neighbouring cells suffice ---------------------------------------------------------------------------------------
 * The gather visits, per query x, the cells c' with |c'_a - floor(x_a / h)| <= 1 on every axis, clipped to [-2^30, 2^30], and in
 * each cell's bucket only the records whose STORED cell equals c'.  A record has one cell, so it is met at most once per query
 * however many of the 27 cells share its bucket; strangers in a bucket (other cells with the same hash) are skipped.  It remains to
 * show that an accepted photon p lies in one of the visited cells.  fl() is rounding to nearest; it is monotone.
 *   1. r <= R, so r2 = fl(r * r) <= fl(R * R).  Each term fl(e_a * e_a) is >= 0 and fl(s + t) >= s for t >= 0, so
 *      fl(e_a * e_a) <= d2 < r2 <= fl(R * R), and by monotonicity |e_a| < R for the COMPUTED e_a = fl(p_a - x_a) -- no slack at all.
 *      e_a = (p_a - x_a)(1 + d) with |d| <= 2^-53 (a difference never underflows), so the TRUE |p_a - x_a| < R (1 + 2^-52).
 *   2. Something was accepted, so fl(R * R) > 0, R >= 2^-538, and R * 2^-20 is exact: h >= R (1 + 2^-20)(1 - 2^-53), hence
 *      h (1 - 2^-21) >= R (1 + 2^-21 - 2^-41)(1 - 2^-53) > R (1 + 2^-52): the true |p_a / h - x_a / h| < 1 - 2^-21.
 *   3. The photon is stored, so |floor(fl(p_a / h))| <= 2^30 and |fl(p_a / h)| < 2^30 + 1; then the true |x_a / h| < 2^30 + 2 and
 *      |fl(x_a / h)| < 2^31.  Below 2^31 a float64 has an ulp of at most 2^-22: each rounded quotient is off by at most 2^-23.
 *   4. So |fl(p_a / h) - fl(x_a / h)| < 1 - 2^-21 + 2^-22 < 1, and the floors differ by at most 1 on every axis.
 *   5. Step 3 also shows that a point with |fl(x_a / h)| >= 2^30 + 3 on some axis, a NaN or an infinity among them, accepts nothing:
 *      the gather answers zeros there without converting the quotient to an integer.  Every other quotient has
 *      |floor| <= 2^30 + 3 < 2^31: the conversion to int32 is exact, and clipping the range loses no stored cell.
 * So a query whose own cell is out of range, yet within R of a photon stored in the outermost cells, gets the brute-force answer.
 */
#ifndef TOR_PHOTONS_H
#define TOR_PHOTONS_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum { TOR_PHOTON_KERNEL_CONSTANT = 0, TOR_PHOTON_KERNEL_EPANECHNIKOV = 1 };

TOR_API int tor_photons_build_device(TorContext* ctx, int64_t n_photons, const double* d_position, const double* d_power,
                                     const double* d_direction, const int32_t* d_list, int64_t n_list, double radius, void* hip_stream);
TOR_API int tor_photons_build_host(TorContext* ctx, int64_t n_photons, const double* position, const double* power,
                                   const double* direction, const int32_t* list, int64_t n_list, double radius);
TOR_API int tor_photons_gather_device(TorContext* ctx, int64_t n_points, const double* d_point, const double* d_normal,
                                      const double* d_radius, const int32_t* d_list, int64_t n_list, int32_t kernel, double max_value,
                                      double* d_sums, int32_t* d_count, void* hip_stream);
TOR_API int tor_photons_gather_host(TorContext* ctx, int64_t n_points, const double* point, const double* normal, const double* radius,
                                    const int32_t* list, int64_t n_list, int32_t kernel, double max_value, double* sums, int32_t* count);
TOR_API int tor_photons_info(TorContext* ctx, int64_t out[4]);

#ifdef __cplusplus
}
#endif

#endif /* TOR_PHOTONS_H */

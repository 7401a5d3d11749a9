/*
 * tor_patches.h -- planar patch queries of libtor_mi355x.so: quads and triangles for host integrators.  Included by tor_render.h
 * (which defines the types used here) after tor_texture.h.
 *
 * ---- a floor, the walls of a room, a lamp panel, a box ---------------------------------------------------------------------------
 * The reference's only geometry is its list of spheres, and so is the library's.  tor_scatter_device, tor_bsdf_eval_device and
 * tor_texture_eval_device already take records "from geometry of its own"; these entries are such geometry: a context-owned TABLE
 * of static planar patches (parallelograms and triangles), a closest-hit query that can merge into the records tor_hit_device wrote
 * and an any-hit query that can merge into tor_occluded_device's bits.  The fused render kernels, tor_hit_device, tor_bounce_device
 * and every other entry never read the table: without it, and for every entry that existed before it, every bit of every answer is
 * as before.
 *
 * All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly this order.
 *   cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *   dot(a, b)   = (a.x*b.x + a.y*b.y) + a.z*b.z
 *
 * TorPatch (88 bytes, asserted on both sides of the ABI).  The surface is q + a*u + b*v:
 *   kind      TOR_PATCH_QUAD (0): 0 <= a <= 1 and 0 <= b <= 1.  TOR_PATCH_TRIANGLE (1): a >= 0, b >= 0, a + b <= 1.
 *   material  the index of the scene object whose material the patch wears, or -1 for none (a lamp panel, a portal).  It goes
 *             into the record's `object` field, so tor_scatter_device, tor_bsdf_eval_device, tor_texture_eval_device and a host's
 *             per-object tables (emission[object], diffuse[object]) serve patch hits unchanged.  A material that no visible sphere
 *             has is carried by a sphere hidden through visibility groups (tor_scene_groups, group word 0): the idiom the media
 *             table uses for its bounding spheres.
 *   groups    the patch's visibility word, tor_scene_groups' rule: the patch takes part for ray i iff groups & mask_i != 0.
 *   reserved  not read
 *   q, u, v   a corner and the two edges from it
 * Patches are two-sided and static: the ray's time is not read.
 *
 * tor_scene_patches: the table of the context, from a HOST array; the library keeps a copy of its own (with the unit normal of
 * every patch, below).  n_patches == 0 clears the table (table is then not read).  The call waits for the context's last query.
 * A host copy (128 bytes per patch) that cannot be allocated is TOR_ERR_OUT_OF_MEMORY, with nothing changed.
 * TOR_ERR_INVALID_ARGUMENT, and nothing changes, tested in this order and all of it before any allocation:
 *   1. a NULL ctx
 *   2. a context without a scene
 *   3. n_patches outside [0, TOR_PATCH_MAX]
 *   4. a NULL table with n_patches > 0
 *   5. per record, in table order, and per record in this order: an unknown kind; material outside [-1, n_objects); a component
 *      of q, u or v that is not finite; n = cross(u, v) with a component that is not finite; nn = dot(n, n) with !(nn > 0) or
 *      infinite; 1.0 / sqrt(nn) not finite
 * Lifecycle, the texture table's: every tor_scene_upload that replaces the scene clears the table (it names objects); a
 * byte-identical upload keeps it; tor_scene_lights, tor_scene_environment, tor_scene_media, tor_scene_media_phase,
 * tor_scene_media_grid, tor_scene_textures, tor_scene_groups and the photon map leave it alone, and it leaves them alone.  The
 * context frees the copy when it is destroyed.
 *
 * tor_patch_info: out[0] = n_patches (0: no table), out[1] = the patches with material >= 0.  Refusals: a NULL ctx or out.
 *
 * tor_patch_hit_device.  Per listed ray i with origin o and direction d (d_rays[i]; time is not read) and range (t_min, t_max) =
 * d_t_range[i], or (0.001, +inf) when d_t_range is NULL, as in tor_hit_device; mask_i = d_mask ? d_mask[i] : mask (a mask of 0:
 * the ray misses every patch).
 *   THE LIMIT.  limit = t_max.  With merge != 0, d_hits[i] is read first: if its object >= 0 and its t < t_max, limit = that t.
 *   A tie with the sphere therefore stays with the sphere.
 *   THE TEST (Moeller-Trumbore, division-free until a patch is accepted), per patch j with groups_j & mask_i != 0:
 *     pv = cross(d, v);  det = dot(u, pv);  if !(|det| > 0): no hit                       (zero and NaN)
 *     tv = o - q;  an = dot(tv, pv);  qv = cross(tv, u);  bn = dot(d, qv);  tn = dot(v, qv)
 *     if det < 0: det, an, bn, tn = -det, -an, -bn, -tn                                    (exact)
 *     QUAD:     an >= 0 && an <= det && bn >= 0 && bn <= det
 *     TRIANGLE: an >= 0 && bn >= 0 && (an + bn) <= det                                     (the sum rounded once)
 *     t = tn / det;  accepted iff t_min < t && t < limit                                   (both strict, spheres.nim:40)
 *   A NaN that reaches a comparison makes it false.
 *   THE WINNER is the accepted patch of the smallest t; ties go to the lower table index.  The t of a patch depends on the ray and
 *   on that patch alone -- not on the limit, not on the patches visited before it -- so the set of accepted (t, index) pairs is a
 *   function of the ray, and its minimum in the order (t, index) is the same whatever order the table is visited in: any visiting
 *   order gives the same winner, the argument DESIGN 4.8 makes for the spheres.
 *   THE RECORD is built for the winner only, t, an, bn, det its values above:
 *     p = o + d * t, per component, as tor_hit_device forms it
 *     n = cross(u, v);  nn = dot(n, n);  N = n * (1.0 / sqrt(nn)), per component
 *     front_face = dot(d, N) < 0;  normal = front_face ? N : -N;  object = material
 *     d_patch[i] = j;  d_uv[i] = (an / det, bn / det) when d_uv is not NULL
 *   NO WINNER.  merge == 0: d_hits[i] is tor_hit_device's miss record (object -1, the rest 0).  merge != 0: d_hits[i] is left
 *   untouched.  Both: d_patch[i] = -1, d_uv[i] = (0, 0).
 *   d_patch is required, d_uv is nullable.
 *   IN BOUNDS.  The winner's index is clamped into [0, n_patches) before any record is read for it: a wrong compare above is a
 *   wrong answer, never a fault.
 *   NOT WATERTIGHT.  Two patches that share an edge are not watertight by construction: on the edge a ray may be accepted by both
 *   (the lower index wins) or, through the rounding of an, bn and det, by neither.
 *
 * tor_patch_occluded_device.  The bit of ray i is "some patch is accepted in (t_min, t_max)": the test above with limit = t_max,
 * whatever merge is.  merge == 0: d_occluded[i] = 0 or 1.  merge != 0: the entry only ever writes 1 -- an OR into
 * tor_occluded_device's answer.  Which patch occludes is not defined; a lane stops at its first accepted patch.
 *
 * d_list / n_list, the stream rule and the order of the refusals are exactly tor_bsdf_eval_device's: NULL = every ray (n_list must
 * be n_rays); entries outside [0, n_rays) are skipped; entries must be unique; rays that are not listed keep what the outputs
 * hold; n_list == 0 and n_rays == 0 are no-ops.  Asynchronous on hip_stream, one stream per context as for the other queries.
 * tor_last_note(): "patch hit", "patch occluded".  TOR_ERR_INVALID_ARGUMENT (nothing written), tested in this order: NULL ctx,
 * n_rays < 0, n_list < 0, a NULL list with n_list != n_rays; NULL d_rays, d_hits or d_patch (d_rays or d_occluded) with work to
 * do; a context without a scene; a context without a patch table.
 * tor_patch_hit_host, tor_patch_occluded_host: the same on host arrays, blocking (every array copied in, the query, the outputs
 * copied out); they wait for the context's last render launch and last query as tor_bsdf_eval_host does.
 */
#ifndef TOR_PATCHES_H
#define TOR_PATCHES_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum { TOR_PATCH_QUAD = 0, TOR_PATCH_TRIANGLE = 1 };
enum { TOR_PATCH_MAX = 16384 };

typedef struct TorPatch {
  int32_t kind, material;
  uint32_t groups;
  int32_t reserved;
  double q[3], u[3], v[3];
} TorPatch;

TOR_API int tor_scene_patches(TorContext* ctx, int64_t n_patches, const TorPatch* table);
TOR_API int tor_patch_info(TorContext* ctx, int64_t* out);
TOR_API int tor_patch_hit_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range, const int32_t* d_list,
                                 int64_t n_list, int32_t merge, TorHit* d_hits, int32_t* d_patch, double* d_uv, void* hip_stream,
                                 const uint32_t* d_mask, uint32_t mask);
TOR_API int tor_patch_hit_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                               int64_t n_list, int32_t merge, TorHit* hits, int32_t* patch, double* uv, const uint32_t* masks,
                               uint32_t mask);
TOR_API int tor_patch_occluded_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t_range,
                                      const int32_t* d_list, int64_t n_list, int32_t merge, int32_t* d_occluded, void* hip_stream,
                                      const uint32_t* d_mask, uint32_t mask);
TOR_API int tor_patch_occluded_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t_range, const int32_t* list,
                                    int64_t n_list, int32_t merge, int32_t* occluded, const uint32_t* masks, uint32_t mask);

#ifdef __cplusplus
}
#endif

#endif /* TOR_PATCHES_H */

/*
 * tor_texture.h -- surface-texture queries of libtor_mi355x.so: checker and octahedral image albedos.  Included by tor_render.h
 * (which defines the types used here) after tor_grid.h.
 *
 * ---- a checkered ground, a painted globe, tinted glass -----------------------------------------------------------------------------
 * The colour of a surface is one constant per object in the reference: the material's albedo.  These entries give a context a TABLE
 * of textures and a BINDING of objects to them, and one query that answers, for a batch of hit records, the colour the surface has
 * at each record: the albedo a host integrator multiplies its throughput by in place of tor_bounce_device's attenuation.  The fused
 * render kernels and tor_bounce_device never read the table: without it, and for every entry that existed before it, every bit of
 * every answer is as before.
 *
 * An image is OCTAHEDRAL, the mapping of tor_env.h applied to the OUTWARD NORMAL of the record: + - * /, abs, copysign and floor
 * only -- no atan2 and no acos, of which the library has no bit-reproducible versions -- so every bit is defined, and
 * tor.environment_directions(n) (the texel-centre directions of that mapping) bakes an image with one call.
 *
 * All arithmetic is float64, unfused, with correctly rounded `/` and sqrt, in exactly this order; sums of three terms associate
 * from the left ((a + b) + c).
 *
 * TorTexture (96 bytes, asserted on both sides of the ABI):
 *   kind     TOR_TEXTURE_CONSTANT (0), TOR_TEXTURE_CHECKER (1) or TOR_TEXTURE_IMAGE (2)
 *   option   a checker's space: TOR_TEXTURE_WORLD (0, the record's p) or TOR_TEXTURE_NORMAL (1, the outward normal);
 *            an image's filter: TOR_TEXTURE_NEAREST (0) or TOR_TEXTURE_BILINEAR (1); a constant's option is not read
 *   side, offset
 *            an image is side x side texels, [row][col], from texel `offset` of the atlas; not read for the other kinds
 *   reserved not read
 *   a, b     the constant's colour is a; the checker's even and odd colours are a and b; an image reads neither
 *   freq     the checker's cells per unit along x, y and z; read for a checker only
 *
 * tor_scene_textures: the table, the binding and the atlas of the context, from HOST arrays; the library keeps copies of its own.
 * table: n_textures records.  binding: n_objects int32, the texture of object j in the ORIGINAL numbering (the uploaded list's), or
 * -1 for none.  texels: n_texels * 3 float64 in [texel][channel] order.  n_textures == 0 clears the table (the other arguments are
 * then checked as far as rules 1-5 go and otherwise not read).  The call waits for the context's last query.  The padded host copy
 * of the atlas (up to 128 MB) that cannot be allocated is TOR_ERR_OUT_OF_MEMORY, with nothing changed.
 * TOR_ERR_INVALID_ARGUMENT, and nothing changes, tested in this order and all of it before any allocation:
 *    1. a NULL ctx
 *    2. a context without a scene
 *    3. n_textures outside [0, TOR_TEXTURE_MAX]
 *    4. n_objects other than the scene's count
 *    5. n_texels outside [0, TOR_TEXTURE_MAX_TEXELS]
 *    6. a NULL table or binding (with n_textures > 0)
 *    7. NULL texels with n_texels > 0
 *    8. per record, in table order: an unknown kind, or an unknown option of a checker or an image; an image with side outside
 *       [1, TOR_TEXTURE_MAX_SIDE], with offset < 0 or with offset + side * side > n_texels; a colour of a constant (a) or a
 *       checker (a, b) that is not finite or is negative; a freq of a checker that is not finite
 *    9. a binding outside [-1, n_textures)
 *   10. a texel (any of the n_texels * 3 values, whether an image covers it or not) that is not finite or is negative
 * Lifecycle, the light table's: every tor_scene_upload that replaces the scene clears the table; a byte-identical upload keeps it;
 * tor_scene_lights, tor_scene_environment, tor_scene_media, tor_scene_media_phase, tor_scene_media_grid, tor_scene_groups and the
 * photon map leave it alone, and it leaves them alone.  The context frees the copies when it is destroyed.
 *
 * tor_texture_info: out[0] = n_textures (0: no table), out[1] = n_texels, out[2] = the objects whose binding is not -1.  Refusals:
 * a NULL ctx or out.
 *
 * tor_texture_eval_device.  Per listed record i the query reads object, p, normal and front_face of d_hits[i] as given (a host may
 * have perturbed the normal or taken the record from geometry of its own; t is not read, as in tor_scatter_device) and writes
 * d_color[i] (3 float64) and, if d_texel is not NULL, d_texel[i] (int32).  The cases, in this order:
 *   no such object   object outside [0, n_objects): colour (0, 0, 0), texel -1.
 *   no texture       binding[object] == -1: the material's albedo for Lambertian and Metal, (1, 1, 1) for Dielectric -- the
 *                    attenuation tor_bounce_device gives a ray that scattered off that object, bit for bit; texel -1.
 *   outward normal   m = front_face != 0 ? normal : -normal (each component negated).  It comes from the record, not from the
 *                    scene: a texture in NORMAL space rides a moving sphere, and for a sphere of negative radius m is whatever
 *                    the record says it is.
 *   CONSTANT         colour a, texel 0.
 *   CHECKER          x = option == WORLD ? p : m.  Per axis k: f_k = floor(x_k * freq_k).  If any !(|f_k| < 2^52) (a NaN, an
 *                    infinity, a product so large that it has no parity to speak of): colour a, texel -1.  Otherwise
 *                    par_k = f_k - 2.0 * floor(f_k * 0.5), exact and 0.0 or 1.0; odd = ((int)par_x + (int)par_y + (int)par_z) & 1;
 *                    colour odd ? b : a, texel odd.
 *   IMAGE            n = side, nd = (double)n.  encode(m) as tor_env.h defines it:
 *                      L1 = |m.x| + |m.y| + |m.z|.  If L1 is 0, NaN or infinite the direction is UNUSABLE: colour 0, texel -1.
 *                      q = (m.x / L1, m.y / L1, m.z / L1)
 *                      if m.y >= 0 (so for -0.0 too): s = q.x, t = q.z;
 *                      else: s = copysign(1.0 - |q.z|, q.x), t = copysign(1.0 - |q.x|, q.z)
 *                      cell(w) = clamp((int)floor((w + 1.0) * (0.5 * nd)), 0, n - 1); cn = cell(s), rn = cell(t)
 *                    The texel output is rn * n + cn for both filters.
 *     NEAREST        colour = texel (rn, cn).
 *     BILINEAR       u = (s + 1.0) * (0.5 * nd) - 0.5; fc = floor(u); al = u - fc
 *                    v = (t + 1.0) * (0.5 * nd) - 0.5; fr = floor(v); be = v - fr
 *                    Each floor f (fc, fr) becomes an int only after !(f >= -1) is mapped to -1 and f > n - 1 to n - 1:
 *                    c0 = (int)fc, c1 = c0 + 1, r0 = (int)fr, r1 = r0 + 1, all in [-1, n].
 *                    Each corner (r, c) of (r0, c0), (r0, c1), (r1, c0), (r1, c1) goes through the SEAM RULE:
 *                      if c < 0 || c > n - 1:  r = (n - 1) - r, then c = clamp(c, 0, n - 1)
 *                      then if r < 0 || r > n - 1:  c = (n - 1) - c, then r = clamp(r, 0, n - 1)
 *                    and loads T00, T01, T10, T11 in that order of corners.  Per channel
 *                      colour = (((1.0 - al) * T00 + al * T01) * (1.0 - be)) + (((1.0 - al) * T10 + al * T11) * be)
 *   The seam rule.  The square's outer edge is a fold: (s = +-1, t) and (s = +-1, -t) are the same direction, and likewise for
 *   t = +-1.  So the neighbour across the right edge of texel (r, n - 1) is texel (n - 1 - r, n - 1), not the texel itself, which
 *   is what plain clamping would interpolate with.  (tests/test_texture_query.py: n = 64, f = 1 + 0.5 sin(3x) cos(2z) + 0.2y baked
 *   at the texel centres, 3e4 directions, half of them within half a texel of the edge: the largest interpolation error in that
 *   band is 1.10x the largest elsewhere with the rule and 1.91x with plain clamping; when the rule was proposed, with another
 *   function and 2e5 directions, the figures were 1.08x and 2.9x.)  At a corner both steps apply.
 *   In bounds.  After the seam rule, r and c are clamped into [0, n - 1] once more as the LAST step before r * n + c is formed,
 *   for the nearest lookup and for each of the four corners, whatever the record holds; offset + n * n <= n_texels was checked
 *   when the table was set, and the binding and the table index were checked then too.  A wrong compare in the lines above is
 *   a wrong answer; it is never a fault.
 *   A NaN that reaches a comparison makes it false.  Nothing is drawn and no state changes.
 *
 * d_list / n_list, the stream rule and the order of the refusals are exactly tor_bsdf_eval_device's: NULL = every record (n_list
 * must be n_hits); entries outside [0, n_hits) are skipped; entries must be unique; records that are not listed keep what the
 * outputs hold; n_list == 0 and n_hits == 0 are no-ops.  Asynchronous on hip_stream, one stream per context as for the other
 * queries.  tor_last_note(): "texture eval".  TOR_ERR_INVALID_ARGUMENT (nothing written), tested in this order: NULL ctx,
 * n_hits < 0, n_list < 0, a NULL list with n_list != n_hits; NULL d_hits or d_color with work to do; a context without a scene;
 * a context without a texture table.
 * tor_texture_eval_host: the same on host arrays, blocking (every array copied in, the query, the outputs copied out); it waits
 * for the context's last render launch and last query as tor_bsdf_eval_host does.
 */
#ifndef TOR_TEXTURE_H
#define TOR_TEXTURE_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

enum { TOR_TEXTURE_CONSTANT = 0, TOR_TEXTURE_CHECKER = 1, TOR_TEXTURE_IMAGE = 2 };
enum { TOR_TEXTURE_WORLD = 0, TOR_TEXTURE_NORMAL = 1 };
enum { TOR_TEXTURE_NEAREST = 0, TOR_TEXTURE_BILINEAR = 1 };
enum { TOR_TEXTURE_MAX = 4096, TOR_TEXTURE_MAX_SIDE = 2048, TOR_TEXTURE_MAX_TEXELS = 1 << 22 };

typedef struct TorTexture {
  int32_t kind, option, side, reserved;
  int64_t offset;
  double a[3], b[3], freq[3];
} TorTexture;

TOR_API int tor_scene_textures(TorContext* ctx, int64_t n_textures, const TorTexture* table, int64_t n_objects, const int32_t* binding,
                               int64_t n_texels, const double* texels);
TOR_API int tor_texture_info(TorContext* ctx, int64_t* out);
TOR_API int tor_texture_eval_device(TorContext* ctx, int64_t n_hits, const TorHit* d_hits, const int32_t* d_list, int64_t n_list,
                                    double* d_color, int32_t* d_texel, void* hip_stream);
TOR_API int tor_texture_eval_host(TorContext* ctx, int64_t n_hits, const TorHit* hits, const int32_t* list, int64_t n_list,
                                  double* color, int32_t* texel);

#ifdef __cplusplus
}
#endif

#endif /* TOR_TEXTURE_H */

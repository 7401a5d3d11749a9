/*
 * tor_phase.h -- phase-function queries of libtor_mi355x.so, included by tor_render.h after tor_media.h (which defines the media
 * table these entries read).
 *
 * ---- haze scatters forward: Henyey-Greenstein sample, value, density ---------------------------------------------------------------
 * tor_media_scatter_device draws an isotropic direction and nothing evaluates one.  These entries give every medium of the table
 * an asymmetry g (tor_scene_media_phase), draw a direction from the Henyey-Greenstein mixture of the active media
 * (tor_phase_sample_device, the twin of tor_media_scatter_device) and evaluate value and density of a direction that was NOT
 * drawn (tor_phase_eval_device, the twin of tor_bsdf_eval_device): what a collision needs to weight the shadow ray of
 * tor_light_sample_device, so that a lamp of the light table lights the fog.  The inversion and the density need only + - * / and
 * sqrt (den^1.5 is den * sqrt(den)); the azimuth goes through the portable sin / cos the isotropic scatter uses; the frame around
 * the incoming direction is the branch-free one of Duff et al. ("Building an Orthonormal Basis, Revisited", JCGT 2017: copysign,
 * one division).  So every bit is defined.  The library still takes neither log, exp nor atan2.
 *
 * Conventions.  Float64, unfused, correctly rounded `/` and sqrt; sums and products of three terms associate from the left;
 * dot(u, v) = u.x * v.x + u.y * v.y + u.z * v.z;  pi = 3.141592653589793;  FOUR_PI = 4.0 * pi;  TWO_PI = 2.0 * pi;
 * clamp1(x):  if x > 1.0: 1.0;  else if x < -1.0: -1.0;  else x   (a NaN stays a NaN).
 *
 * tor_scene_media_phase(ctx, n_media, g): one asymmetry g_m per medium of the context's media table, from a HOST array.  It lives
 * in word [15] of the media record, which tor_scene_media zero-fills: every table starts isotropic, setting the media table again
 * resets g to 0, and a replacing tor_scene_upload clears the table with everything in it.  g == NULL: every medium becomes 0.  The
 * call waits for the context's last query.  TOR_ERR_INVALID_ARGUMENT, and nothing changes, tested in this order: a NULL ctx; a
 * context without a scene; no media table; n_media not equal to the table's count; a g that is not finite; a g with
 * |g| > TOR_PHASE_G_MAX; a g with 0 < |g| < TOR_PHASE_G_MIN.  Why the lower bound: below 2^-20 the inversion's (.) / (2 g) loses
 * its digits, and for a g whose square underflows it returns cosine 0 for every draw; g == 0, -0.0 included, takes the isotropic
 * line of the sampler.  With |g| <= 0.99 and |mu| <= 1, den below is >= 1e-4.
 *
 *   hg(g, mu)          g2 = g * g;  den = (1.0 + g2) - (2.0 * g) * mu;  hg = (1.0 - g2) / (FOUR_PI * (den * sqrt(den))).
 *                      Nothing is special-cased: g = 0 gives 1 / FOUR_PI.
 *   mixture(active, mu)  rho = 0, q = 0, n = (0, 0, 0).  For m ascending over the bits of active:  p = hg(g_m, mu);
 *                      rho = rho + sigma_m;  q = q + sigma_m * p;  n_c = n_c + (sigma_m * albedo_m,c) * p.
 *
 * tor_phase_eval_device: draws nothing, changes no state.  Per listed item i it reads d_in[i].direction (the direction the path was
 * travelling in), active = d_active[i] (the march's word) and d_out[i].direction; both may have any positive finite length.
 *   set-up     ii = dot(in, in);  oo = dot(out, out).
 *   no answer  value = (0, 0, 0), pdf = 0 if !(ii > 0) or ii == +inf, !(oo > 0) or oo == +inf, active == 0, active has a bit at or
 *              above n_media, or !(rho > 0) after the mixture.
 *   otherwise  w = in * (1.0 / sqrt(ii));  v = out * (1.0 / sqrt(oo));  mu = clamp1(dot(w, v));  mixture(active, mu);
 *              pdf = q / rho;  value_c = n_c / rho.
 *   value is the single-scattering albedo times the phase function per channel (as tor_bsdf_eval_device's value is albedo * pdf);
 *   pdf is the solid-angle density with which tor_phase_sample_device draws `out`.
 *   outputs    d_value[i] (3 float64), d_pdf[i].
 *
 * tor_phase_sample_device: the operands of tor_media_scatter_device plus d_pdf (nullable); d_rays_out may be d_rays.  Per listed ray
 * i = (o, d, time) with t = d_t[i], active = d_active[i] and state s = d_rng[i]:
 *   draws      u_sel = uniform01(s); u_cos = uniform01(s); u_phi = uniform01(s): exactly three outputs of the generator, always, in
 *              this order -- also for an entry that gets no sample.  d_rng[i] is the state after them.
 *   set-up     ii = dot(d, d).  rho = 0.0; for m ascending over the bits of active: rho = rho + sigma_m.
 *   refusal    if active == 0, or it has a bit at or above n_media, or !(rho > 0), or !(ii > 0), or ii == +inf:  att = (0, 0, 0), the
 *              seven words of the out ray 0, pdf = 0.
 *   selection  x = u_sel * rho;  acc = 0.0;  chosen = last = -1.  For m ascending over the bits of active:  acc = acc + sigma_m;
 *              if sigma_m > 0: last = m;  if chosen < 0 && x < acc: chosen = m.  Afterwards, if chosen < 0: chosen = last.
 *              (The fallback is for a product that rounds up to rho.  uniform01 keeps 52 bits, u_sel <= 1 - 2^-52, so for a normal
 *              rho the product lies below rho and `x < acc` decides at the last active medium at the latest; for a subnormal rho
 *              below 2^-1023 the product rounds back to rho and the fallback decides.  A medium with sigma = 0 is never chosen:
 *              acc does not move past x at it, and the fallback skips it.)
 *   cosine     g = g_chosen.  If g == 0: mu = 1.0 - 2.0 * u_cos.  Else  gg = g * g;  s = (1.0 - gg) / ((1.0 - g) + (2.0 * g) * u_cos);
 *              mu = ((1.0 + gg) - s * s) / (2.0 * g).  Then mu = clamp1(mu)  (the inversion leaves [-1, 1] by a few ulps at the
 *              extreme uniforms only);  r2 = 1.0 - mu * mu;  if !(r2 > 0): r2 = 0.0;  st = sqrt(r2).
 *   azimuth    phi = u_phi * TWO_PI;  (sp, cp) = the portable sin and cos of phi.
 *   frame      w = d * (1.0 / sqrt(ii));  sg = copysign(1.0, w.z);  a = -1.0 / (sg + w.z);  b = (w.x * w.y) * a;
 *              b1 = (1.0 + ((sg * w.x) * w.x) * a,  sg * b,  -(sg * w.x));   b2 = (b,  sg + (w.y * w.y) * a,  -w.y).
 *   direction  v_c = ((st * cp) * b1_c + (st * sp) * b2_c) + mu * w_c.
 *   weights    mixture(active, mu) with this mu -- the cosine that was drawn, not dot(w, v).  pdf = q / rho;  att_c = n_c / q.
 *              If !(q > 0): the refusal's zeros.
 *   outputs    d_rays_out[i] = { o + t * d, v, time }  (p_c = o_c + t * d_c),  d_att[i] (3 float64),  d_pdf[i].
 *
 * Termination.  Every loop of both entries is counted by n_media <= TOR_MEDIA_MAX: the sampler walks the table at most three times
 * (rho, selection, mixture), the evaluation once.  No comparison that goes wrong (a NaN anywhere) can make either run on; it shows
 * as a wrong answer.
 *
 * d_list / n_list, the stream, the waits and the blocking _host twins are exactly those of tor_media_scatter_device (tor_media.h).
 * TOR_ERR_INVALID_ARGUMENT (nothing written), tested in this order: NULL ctx, n < 0, n_list < 0, a NULL list with n_list != n; NULL
 * arrays with work to do (d_in, d_active, d_out, d_value or d_pdf; d_rays, d_t, d_active, d_rng, d_rays_out or d_att); a context
 * without a scene; an empty media table.  tor_last_note(): "phase eval: 5 media", "phase sample: 5 media".
 */
#ifndef TOR_PHASE_H
#define TOR_PHASE_H

#ifndef TOR_RENDER_H
#include "tor_render.h"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define TOR_PHASE_G_MAX 0.99
#define TOR_PHASE_G_MIN (1.0 / 1048576.0) /* 2^-20 */

TOR_API int tor_scene_media_phase(TorContext* ctx, int64_t n_media, const double* g);
TOR_API int tor_phase_eval_device(TorContext* ctx, int64_t n, const TorRay* d_in, const uint64_t* d_active, const TorRay* d_out,
                                  const int32_t* d_list, int64_t n_list, double* d_value, double* d_pdf, void* hip_stream);
TOR_API int tor_phase_eval_host(TorContext* ctx, int64_t n, const TorRay* in, const uint64_t* active, const TorRay* out,
                                const int32_t* list, int64_t n_list, double* value, double* pdf);
TOR_API int tor_phase_sample_device(TorContext* ctx, int64_t n_rays, const TorRay* d_rays, const double* d_t, const uint64_t* d_active,
                                    TorRng* d_rng, const int32_t* d_list, int64_t n_list, TorRay* d_rays_out, double* d_att,
                                    double* d_pdf, void* hip_stream);
TOR_API int tor_phase_sample_host(TorContext* ctx, int64_t n_rays, const TorRay* rays, const double* t, const uint64_t* active,
                                  TorRng* rng, const int32_t* list, int64_t n_list, TorRay* rays_out, double* att, double* pdf);

#ifdef __cplusplus
}
#endif

#endif /* TOR_PHASE_H */

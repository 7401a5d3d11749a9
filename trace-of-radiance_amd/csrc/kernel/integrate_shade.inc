// integrate_shade.inc -- section (C) of integrate_kernel's bounce iteration: sky (render.nim:41-45) or scatter (materials.nim:21-96),
// depth bookkeeping (render.nim:25,47) and the end of a sample (render.nim:67).  Runs under `if (active)`.
      // ================= (C) shade ====================================================
      // unit_vector(direction) is needed by the sky (render.nim:42), Metal (materials.nim:40) and Dielectric
      // (materials.nim:68): the wave would walk through three copies of the square root and the division -- one
      // copy, in front of the branches, serves all of them (same operations on the same ray: same bits)
      // (ARITH 2: the screen's normalised direction IS unit_vector(d) -- d * (1.0 / sqrt(dx*dx + dy*dy + dz*dz)), the same operations
      // on the same ray (vec3s.nim:19-20,93-94,106-107; tor_screen.hpp screen2_ray) -- so the square root and the division run once per bounce)
      const V3 ud_ray = kScreen ? v3(sray.dnx, sray.dny, sray.dnz) : unit_vector(d);
      if (kResume && p.max_depth <= 0) {
        // render.nim:25: the bounce loop does not run -- the sample is black, and the camera ray's draws (render.nim:63-65,
        // cameras.nim:47-57) were the sample's only draws (a resume pass must leave the stream where the reference leaves it)
        ended = true;
      } else if (best_idx < 0) {
        radiance = sky_unit(ud_ray, get_att());  // render.nim:41-45
        ended = true;
      } else {
        const double* c = p.cold + (size_t)best_idx * 16;
        // (ARITH 2 variants: the fields behind the `moving` flag and behind the material kind are requested with the rest -- one
        // round trip through the vector cache per bounce instead of two or three)
        double e3 = 0.0, e4 = 0.0, e5 = 0.0, e12 = 0.0;
        if constexpr (kScreen) { e3 = c[3]; e4 = c[4]; e5 = c[5]; e12 = c[12]; }
        const double inv_r = c[6], alb_x = c[9], alb_y = c[10], alb_z = c[11];
        const int flags = (int)__double_as_longlong(c[13]);
        V3 center = v3(c[0], c[1], c[2]);
        if (flags & 1) {
          if (kScreen) center = center + v3(e3, e4, e5) * best_f;
          else center = center + v3(c[3], c[4], c[5]) * best_f;
        }
        const V3 hp = o + d * best_t;                       // rays.nim:24-25
        const V3 outward = (hp - center) * inv_r;           // spheres.nim:43 (c[6] = 1.0/radius)
        const bool front = dot(d, outward) < 0.0;           // core.nim:47-49
        const V3 n = front ? outward : -outward;
        const int mat = (flags >> 8) & 0xff;
        const V3 albedo = v3(alb_x, alb_y, alb_z);
        if (mat == kLambertian) {  // materials.nim:24-30
          d = n + random_unit_vector(rng);
          o = hp;
          set_att(mul_att(get_att(), albedo));  // render.nim:35
        } else if (mat == kMetal) {  // materials.nim:39-47
          const V3 reflected = reflect(ud_ray, n);
          const V3 nd = reflected + random_in_unit_sphere(rng) * (kScreen ? e12 : c[12]);
          o = hp;
          d = nd;
          time = 0.0;  // rays.nim:19 default
          if (dot(nd, n) > 0.0) {
            set_att(mul_att(get_att(), albedo));
          } else {
            ended = true;  // render.nim:38: absorbed -> black
          }
        } else {  // materials.nim:62-86
          const double eta = front ? alb_x : (kScreen ? e12 : c[12]);  // 1.0 / ri : ri  (the quotient comes from the host, tor_scene.cpp)
          const V3 ud = ud_ray;
          const double dn = dot(-ud, n);
          const double cos_theta = (dn <= 1.0) ? dn : 1.0;
          const double sin_theta = __builtin_sqrt(1.0 - cos_theta * cos_theta);
          V3 nd;
          if (eta * sin_theta > 1.0) {
            nd = reflect(ud, n);
          } else {
            const double reflect_prob = schlick_r0(cos_theta, front ? alb_y : alb_z);
            if (uniform01(rng) < reflect_prob) nd = reflect(ud, n);
            else nd = refract(ud, n, eta);
          }
          o = hp;
          d = nd;
          time = 0.0;
          // (materials.nim:63 attenuates by (1, 1, 1): x * 1.0 == x for every float64, so the product is not formed)
        }
        if (!ended) {
          depth += 1;
          if (depth >= p.max_depth) ended = true;  // render.nim:25,47: loop exhausted -> black
        }
      }

      if (ended) {
        active = false;
        if (stats_on) atomicAdd(&prof_lds[kStSamples], 1ull);
        if (kProbe) {
          atomicAdd(p.pixel_cost + (unsigned)pix, (unsigned)path_q);
          path_q = 0;
        }
        if (kPixel) {
          if (kAccInLds) acc = v3(pix_acc[0], pix_acc[64], pix_acc[128]);
          acc = acc + radiance;  // render.nim:67
          if (kResMom) {  // the second moments, in sample order: one rounding for the product, one for the sum
            pix_mom[0] = pix_mom[0] + radiance.x * radiance.x; pix_mom[64] = pix_mom[64] + radiance.y * radiance.y;
            pix_mom[128] = pix_mom[128] + radiance.z * radiance.z;
          }
          s += 1;
          if (s >= p.spp) {
            double* out = p.out + (size_t)pix * 3;
            out[0] = acc.x; out[1] = acc.y; out[2] = acc.z;
            if (kResume) {  // the pixel's pass is over: the stream's state behind its last sample (and the moments) go back to the caller
              unsigned long long* st = p.rstate + (size_t)pix * 4;
              st[0] = rng.s0; st[1] = rng.s1; st[2] = rng.s2; st[3] = rng.s3;
              if (kResMom) { double* mo = p.mom + (size_t)pix * 3; mo[0] = pix_mom[0]; mo[1] = pix_mom[64]; mo[2] = pix_mom[128]; }
            }
          } else {
            if (kAccInLds) { pix_acc[0] = acc.x; pix_acc[64] = acc.y; pix_acc[128] = acc.z; }
            have_item = true;  // next sample of the same pixel, same stream
          }
        }
      }

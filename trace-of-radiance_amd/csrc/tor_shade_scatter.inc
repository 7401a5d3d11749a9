// tor_shade_scatter.inc -- rec.material.scatter(r_in, rec, rng, attenuation, scattered) (materials.nim:21-96) for one lane, in the
// reference's operation and draw order: THE text of the scatter, included in the body of radiance_kernel (tor_radiance.hip),
// bounce_kernel and scatter_kernel (tor_bounce.hip).  In scope: c (the object's cold record, tor_kernels.hpp), r (QRay: r_in on entry
// -- only r.time is read --, `scattered` on exit: origin hp, the new direction, Lambertian keeps r.time, Metal and Dielectric write
// 0), hp / n / front (rec.p, rec.normal, rec.front_face), ud (unit_vector(r_in.direction)), g (the lane's Rng), att (V3, multiplied
// by the attenuation: a caller that wants the attenuation itself passes (1, 1, 1) -- 1.0 * x == x) and ended (set for an absorbed
// Metal ray, whose `scattered` is still written as materials.nim:41 writes it before the test).
      const int flags = (int)__double_as_longlong(c[13]);
      const int mat = (flags >> 8) & 0xff;
      const V3 albedo = v3(c[9], c[10], c[11]);
      if (mat == kLambertian) {  // materials.nim:24-30: the scattered ray keeps r_in.time
        set_ray(r, hp, n + random_unit_vector(g));
        att = mul_att(att, albedo);  // render.nim:35
      } else if (mat == kMetal) {  // materials.nim:39-47
        const V3 nd = reflect(ud, n) + random_in_unit_sphere(g) * c[12];
        set_ray(r, hp, nd);
        r.time = 0.0;  // rays.nim:19 default
        if (dot(nd, n) > 0.0) att = mul_att(att, albedo);
        else ended = true;  // render.nim:38: absorbed -> black
      } else {  // materials.nim:62-86
        const double eta = front ? c[9] : c[12];  // 1.0 / ri : ri (tor_scene.cpp fill_material)
        const double dn = dot(-ud, n);
        const double cos_theta = (dn <= 1.0) ? dn : 1.0;
        const double sin_theta = __builtin_sqrt(1.0 - cos_theta * cos_theta);
        V3 nd;
        if (eta * sin_theta > 1.0) {
          nd = reflect(ud, n);
        } else {
          const double reflect_prob = schlick_r0(cos_theta, front ? c[10] : c[11]);
          if (uniform01(g) < reflect_prob) nd = reflect(ud, n);
          else nd = refract(ud, n, eta);
        }
        set_ray(r, hp, nd);
        r.time = 0.0;
        // (the attenuation (1, 1, 1): x * 1.0 == x, the product is not formed)
      }

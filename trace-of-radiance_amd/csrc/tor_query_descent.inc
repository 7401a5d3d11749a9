// tor_query_descent.inc -- the closest hit of ray `r` over the scene of `p` (QParams) into `b` (QBest, starting at {r.t_max,
// INT_MAX, -1}): the wave-uniform slots, then (BLOCKS) the walk of the rays the boxes do not hold for and the block / super-box
// descent of those they do.  Included in the body of hit_kernel (tor_query.hip), radiance_kernel (tor_radiance.hip) and
// bounce_kernel (tor_bounce.hip), with p, r, b, `live`, `vis` and the template parameter BLOCKS in scope.  Every lane of the
// wave runs it, converged (the uniform loops use scalar loads); lanes with live = false take part with r.t_max = 0, which accepts
// nothing.  Textual, as the integrator's kernel/*.inc sections are: a function call in its place changes the hit kernels'
// register allocation.  `vis` (Sees, tor_query.hpp) says whether the lane's ray sees a slot, or anything behind a box: asked
// before the exact test's arithmetic and before a box's slab test, so a ray does not enter a box that holds nothing it sees.
// Every includer declares it as a local; a Sees<false> answers yes and compiles to nothing.
  // wave-uniform: every lane tests the same record
  for (int s = 0; s < p.n_uniform; ++s)
    if (vis.slot_u(s)) exact_test((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)s), s, r, b);
  if constexpr (BLOCKS) {
    const double ex = r.ox - p.org[0], ey = r.oy - p.org[1], ez = r.oz - p.org[2];
    const bool boxed = live && (r.t_min >= 0.0) && (r.time >= p.time_lo) && (r.time <= p.time_hi) &&
                       (ex * ex + ey * ey + ez * ez <= p.reach2) && (r.a >= p.a_min);
    const bool walk = live && !boxed;
    if (__ballot(walk) != 0) {  // rays the boxes do not hold for: every spatial slot, wave-uniform
      for (int s = 0; s < p.n_spatial; ++s) {
        const int slot = p.spatial_base + s;
        if (walk && vis.slot_u(slot)) exact_test((qcdptr)(uintptr_t)(p.cold + 16 * (size_t)slot), slot, r, b);
      }
    }
    if (boxed) {
      const double ix = 1.0 / r.dx, iy = 1.0 / r.dy, iz = 1.0 / r.dz;
      auto test_box = [&](int box) {  // the 8 objects of each block behind block box `box`
        for (int fk = 0; fk < p.fanout; ++fk) {
          const int slot0 = p.spatial_base + 8 * (box * p.fanout + fk);
          for (int k = 0; k < 8; ++k)
            if (vis.slot(slot0 + k)) exact_test((qgdptr)(uintptr_t)(p.cold + 16 * (size_t)(slot0 + k)), slot0 + k, r, b);
        }
      };
      const int n_top = p.two_level ? p.n_super : p.n_boxes;
      const int top0 = p.two_level ? p.super0 : 0;
      // the top-level boxes 64 at a time, wave-uniform (scalar loads); then per lane the ones its ray enters
      for (int c0 = 0; c0 < n_top; c0 += 64) {
        const int cn = n_top - c0 < 64 ? n_top - c0 : 64;
        unsigned long long m = 0;
        for (int j = 0; j < cn; ++j)
          if (vis.box_u(top0 + c0 + j) && slab((qcdptr)(uintptr_t)(p.bnd + 8 * (size_t)(top0 + c0 + j)), r, ix, iy, iz)) m |= 1ull << j;
        while (m != 0) {
          const int top = c0 + __builtin_ctzll(m);
          m &= m - 1;
          if (!p.two_level) {
            test_box(top);
            continue;
          }
          // super box `top`: its 8 block boxes (NaN padding boxes are never entered)
          unsigned m8 = 0;
          for (int k = 0; k < 8; ++k)
            if (vis.box(8 * top + k) && slab((qgdptr)(uintptr_t)(p.bnd + 8 * (size_t)(8 * top + k)), r, ix, iy, iz)) m8 |= 1u << k;
          while (m8 != 0) {
            const int k = __builtin_ctz(m8);
            m8 &= m8 - 1;
            test_box(8 * top + k);
          }
        }
      }
    }
  }

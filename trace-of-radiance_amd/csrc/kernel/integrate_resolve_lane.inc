// integrate_resolve_lane.inc -- per-lane resolve of integrate_kernel (all variants but the cooperative ones): every queued candidate
// through the reference's exact test (spheres.nim:28-49, moving_spheres.nim:39-67, own operation order), closest hit with ties
// to the lowest original index (hittables_lists.nim:48-55).  kWords variants read 32-slot mask words, the others queue entries
// (object masks, block boxes, super boxes: TOR_ACCEL_BLOCKS expands blocks per lane here).
        // ---- resolve the queued candidates exactly as spheres.nim:35-48 does -------------
        // Queue entries are 8-bit masks over 8 consecutive cold slots (direct candidates) or, flagged
        // with bit 31, over 8 block bounds.  A trip of the loop handles one set bit per lane: either
        // one object, or one spatial block of 8 objects (an unrolled discriminant/filter stage over
        // the block's compact records, then exact roots for the few that pass).
        int f_gid = -1;      // time group whose fraction f_val = (time - time0)/(time1 - time0) is cached
        double f_val = 0.0;  // (moving_spheres.nim:42; identical for every member of a time group)
        // exact part of hit(): spheres.nim:35-48 with t_min = 0.001 and the order-independent update
        auto exact_hit = [&](double cx, double cy, double cz, double r2, unsigned idx, double f) {
          const double ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
          const double hb = ocx * dx + ocy * dy + ocz * dz;
          const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
          const double disc = hb * hb - a * cc;
          if (disc > 0.0) {
            const double root = __builtin_sqrt(disc);
            double sol = (-hb - root) / a;
            bool ok = (0.001 < sol) && (sol < __builtin_inf());
            if (!ok) {
              sol = (-hb + root) / a;
              ok = (0.001 < sol) && (sol < __builtin_inf());
            }
            if (ok) {
              const int orig = (int)__double_as_longlong(p.cold[(size_t)idx * 16 + 14]);
              if (sol < best_t || (sol == best_t && orig < best_orig)) {
                best_t = sol;
                best_idx = (int)idx;
                best_orig = orig;
                best_f = f;
              }
            }
          }
        };
        // centre of a spatial object from its compact record {c0 xyz, r^2, dc xyz, group id | -1}
        // HS = float64 per record: 8, or 4 for an all-static set (no dc / group fields)
        auto spatial_center = [&](auto hrec, auto HS, double& cx, double& cy, double& cz, double& f) {
          constexpr int hs = decltype(HS)::value;
          cx = hrec[0]; cy = hrec[1]; cz = hrec[2];
          f = 0.0;
          const int gid = (hs == 8) ? (int)hrec[7] : -1;
          if (gid >= 0) {
            if (gid != f_gid) {
              f_val = (time - p.sgrp[2 * gid]) / p.sgrp[2 * gid + 1];
              f_gid = gid;
            }
            f = f_val;
            cx = cx + hrec[4] * f; cy = cy + hrec[5] * f; cz = cz + hrec[6] * f;
          }
        };
        // exact hit of the object in cold slot `slot` (centre from the cold record).  The whole record is requested up front: the
        // resolve pass is a chain of dependent vector loads and float64 divisions, and flags -> time group -> dc -> original index
        // one after the other cost three round trips through the vector cache per candidate; eleven unconditional loads cost one
        auto exact_cold = [&](unsigned slot) {
          const gdptr c = (gdptr)(uintptr_t)p.cold + (size_t)slot * 16;
          const double c0x = c[0], c0y = c[1], c0z = c[2], dcx = c[3], dcy = c[4], dcz = c[5], ct0 = c[7], cdt = c[8];
          const int flags = (int)__double_as_longlong(c[13]);
          const int orig = (int)__double_as_longlong(c[14]);
          const double r2 = c[15];
          double cx = c0x, cy = c0y, cz = c0z, f = 0.0;
          if (flags & 1) {
            if (double_to_bits(ct0) == fc_t0 && double_to_bits(cdt) == fc_dt) f = fc_f;
            else f = (time - ct0) / cdt;
            cx = cx + dcx * f; cy = cy + dcy * f; cz = cz + dcz * f;   // moving_spheres.nim:42
          }
          const double ocx = ox - cx, ocy = oy - cy, ocz = oz - cz;
          // spheres.nim:29-34, own operation order
          const double hb = ocx * dx + ocy * dy + ocz * dz;
          const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - r2;
          const double disc = hb * hb - a * cc;
          // (r2 >= 0: never a padding slot -- centre 0, r^2 = -1 --, which a `wild` ray of the float32 filter keeps and which the
          // reference's rounding "hits" from origins where |o|^2 + 1 == |o|^2; the words of the screened brute force hold no padding
          // bit for a ray that is not wild by its DIRECTION, and that one the test above rejects)
          if (disc > 0.0 && (kWords || r2 >= 0.0)) {
            const double root = __builtin_sqrt(disc);
            double sol = (-hb - root) / a;
            bool ok = (0.001 < sol) && (sol < __builtin_inf());
            if (!ok) {
              sol = (-hb + root) / a;
              ok = (0.001 < sol) && (sol < __builtin_inf());
            }
            if (ok && (sol < best_t || (sol == best_t && orig < best_orig))) {
              best_t = sol;
              best_idx = (int)slot;
              best_orig = orig;
              best_f = f;
            }
          }
        };
        if constexpr (kWords) {
          // words: bit (31 - j) of word k <-> cold slot (w_base + k) * 32 + j
          unsigned cur_mask = 0, cur_base = 0, nzr = nz;
          const int n_words = __builtin_amdgcn_readfirstlane(w_count), word0 = __builtin_amdgcn_readfirstlane(w_base);
          for (;;) {
            if (cur_mask == 0 && nzr != 0) {
              const int b = 31 - __builtin_clz(nzr);
              nzr &= ~(1u << b);
              const unsigned k = (unsigned)(n_words - 1 - b);
              cur_mask = q[k * 64];
              cur_base = ((unsigned)word0 + k) * 32u;
            }
            const bool has = cur_mask != 0;
            if (ballot64(has) == 0) break;
            if (prof && lane == 0) prof_lds[kSecTrips] += 1;
            if (has) {
              const int b = 31 - __builtin_clz(cur_mask);
              cur_mask &= ~(1u << b);
              if (stats_on) atomicAdd(&prof_lds[kStCand], 1ull);
              exact_cold(cur_base + (unsigned)(31 - b));
            }
          }
        } else {
        unsigned kq = 0, cur_mask = 0, cur_block = 0, cur_is_bound = 0;
        for (;;) {
          if (cur_mask == 0 && kq < qn) {
            const unsigned e = q[kq * 64];
            kq += 1;
            cur_is_bound = e >> 30;  // 0: object mask, 2: block boxes, 1: super boxes
            cur_block = (e >> 8) & 0x3fffffu;
            cur_mask = e & 0xffu;
          }
          const bool has = cur_mask != 0;
          if (ballot64(has) == 0) break;
          if (prof && lane == 0) prof_lds[kSecTrips] += 1;
          if (has) {
            const int b = 31 - __builtin_clz(cur_mask);  // bit (7 - j) <-> record j of the group
            cur_mask &= ~(1u << b);
            const unsigned rec = cur_block * kBlock + (unsigned)(7 - b);
            if (BLOCKS && cur_is_bound) {
              // ---- spatial block `blk_id`: filter its 8 objects, then exact roots for the survivors
              auto expand = [&](auto blk, auto HS, unsigned blk_id) {
                constexpr int hs = decltype(HS)::value;
                unsigned m8 = 0;
                auto test = [&](int j) {
                  double cx, cy, cz, f;
                  spatial_center(blk + hs * j, HS, cx, cy, cz, f);
                  // (& ~sign of r^2: a padding record -- centre 0, r^2 = -1 -- is never kept.  "discriminant <= -|d|^2" holds for it
                  // only while |o|^2 + 1 != |o|^2; a ray beyond the boxes' reach, which enters every block, is far enough for the
                  // reference's own rounding to "hit" the padding sphere at the world origin)
                  m8 = push_bit(m8, disc_filter(ox, oy, oz, dx, dy, dz, a, cx, cy, cz, blk[hs * j + 3]) & ~hi32(blk[hs * j + 3]));
                };
                if constexpr (hs == 4) {  // 32-byte static records: all eight in flight
#pragma unroll
                  for (int j = 0; j < kBlock; ++j) test(j);
                } else {  // 64-byte records: four at a time (eight make the 168-register variants spill inside the bounce loop)
#pragma unroll 4
                  for (int j = 0; j < kBlock; ++j) test(j);
                }
                while (m8 != 0) {
                  const int bb = 31 - __builtin_clz(m8);
                  m8 &= ~(1u << bb);
                  const int j = 7 - bb;
                  double cx, cy, cz, f;
                  spatial_center(blk + hs * j, HS, cx, cy, cz, f);
                  exact_hit(cx, cy, cz, blk[hs * j + 3], (unsigned)p.spatial_base + blk_id * kBlock + (unsigned)j, f);
                }
              };
              using S8 = std::integral_constant<int, 8>;
              using S4 = std::integral_constant<int, 4>;
              // (float32 block records belong to the cooperative resolve above; this per-lane path serves F32 = 0)
              auto expand_block = [&](unsigned blk_id) {
                if (stats_on) atomicAdd(&prof_lds[kStCand], (unsigned long long)kBlock);
                if (p.shot_stride == 8) {  // float64 compact records
                  if (staged) expand(shot_lds + (size_t)blk_id * (8 * kBlock), S8{}, blk_id);            // ds_read
                  else expand((gdptr)(uintptr_t)p.shot + (size_t)blk_id * (8 * kBlock), S8{}, blk_id);  // global_load
                } else {
                  if (staged) expand(shot_lds + (size_t)blk_id * (4 * kBlock), S4{}, blk_id);
                  else expand((gdptr)(uintptr_t)p.shot + (size_t)blk_id * (4 * kBlock), S4{}, blk_id);
                }
              };
              if (cur_is_bound == 2) {
                for (int fk = 0; fk < kBoxFanout; ++fk) expand_block(rec * (unsigned)kBoxFanout + (unsigned)fk);  // a box stands for box_fanout blocks
              } else {
                // super box `rec`: slab-test its 8 block boxes, descend into the ones the ray can touch
                unsigned mc = 0;
                {
                const gdptr cb = (gdptr)(uintptr_t)p.bnd + (size_t)rec * (8 * kBlock);
                const double ix = 1.0 / dx, iy = 1.0 / dy, iz = 1.0 / dz;
#pragma unroll
                for (int j = 0; j < kBlock; ++j) {
                  const double tx0 = (cb[8 * j + 0] - ox) * ix, tx1 = (cb[8 * j + 3] - ox) * ix;
                  const double ty0 = (cb[8 * j + 1] - oy) * iy, ty1 = (cb[8 * j + 4] - oy) * iy;
                  const double tz0 = (cb[8 * j + 2] - oz) * iz, tz1 = (cb[8 * j + 5] - oz) * iz;
                  const double t_in = __builtin_fmax(__builtin_fmax(__builtin_fmin(tx0, tx1), __builtin_fmin(ty0, ty1)),
                                                     __builtin_fmax(__builtin_fmin(tz0, tz1), 0.0));
                  const double t_out = __builtin_fmin(__builtin_fmin(__builtin_fmax(tx0, tx1), __builtin_fmax(ty0, ty1)),
                                                      __builtin_fmax(tz0, tz1));
                  mc = (mc << 1) | ((t_in <= t_out) ? 1u : 0u);
                }
                }
                mc |= box_far;  // (beyond the boxes' reach: all 8 block boxes of a real super box exist, NaN padding included)
                while (mc != 0) {
                  const int cbit = 31 - __builtin_clz(mc);
                  mc &= ~(1u << cbit);
                  for (int fk = 0; fk < kBoxFanout; ++fk) expand_block((rec * kBlock + (unsigned)(7 - cbit)) * (unsigned)kBoxFanout + (unsigned)fk);
                }
              }
            } else {
              if (stats_on) atomicAdd(&prof_lds[kStCand], 1ull);
              exact_cold(rec);
            }
          }
        }
        }  // (queue entries)

// integrate_resolve_coop.inc -- COOPERATIVE resolve of integrate_kernel (variants TOR_ACCEL_BLOCKS | TOR_ACCEL_F32; DESIGN 4.6): the wave
// pools the (ray, block) pairs and (ray, object) survivors of its 64 rays in LDS lists and works through them 64 at a time.
          // ---- cooperative resolve (TOR_ACCEL_BLOCKS | TOR_ACCEL_F32) -------------------------------------------
          // The per-lane version below walks each lane's own boxes: 3.2 block expansions per ray on average but 8
          // for the worst lane of a wave, ~250 instructions per trip, most lanes idle.  Here the wave pools the
          // work: (A) every lane turns its queue entries into (ray, block) PAIRS and direct (ray, object) SURVIVORS
          // in two LDS lists (positions from a DPP prefix sum, the counts stay in scalar registers); (B) whenever
          // 64 pairs are pending, the 64 lanes expand one pair each -- the owner's float32 ray comes over
          // ds_bpermute -- and append the objects the filter keeps to the survivor list; (C) whenever 64 survivors
          // are pending, the 64 lanes run the reference's float64 test (spheres.nim:28-49) for one survivor each --
          // the owner's float64 ray comes over ds_bpermute -- and merge the root into the owner's closest hit in
          // LDS: atomic min on t, ties to the lowest original index (hittables_lists.nim:48-55).
          // Every trip of (B)/(C) has 64 busy lanes; lanes whose own path is dead work for the others.
          const unsigned my_qn = active ? qn : 0u;
          unsigned n_pairs = 0, n_surv = 0;  // pending list entries (wave-uniform)
          // (C) one trip: survivors [base, base + n)
          auto trip_c = [&](unsigned base, unsigned n) {
#ifdef TOR_FINE_PROBE
            TOR_FINE(fine_state)
#endif
            const bool mine = (unsigned)lane < n;
            const unsigned e = mine ? coop_surv[base + (unsigned)lane] : (unsigned)lane;
            const int src = (int)(e & 63u);
            const unsigned slot = e >> 6;
            const double sox = __shfl(ox, src), soy = __shfl(oy, src), soz = __shfl(oz, src);
            const double sdx = __shfl(dx, src), sdy = __shfl(dy, src), sdz = __shfl(dz, src);
            const double sa = __shfl(a, src), stime = __shfl(time, src), sfsp = __shfl(f_sp, src);
            bool ok = false;
            double sol = 0.0;
            int orig = 0;
            if (mine) {
              // (the whole record is requested up front: flags -> time group -> dc -> radius^2 -> original index one after the
              // other were four dependent round trips through the vector cache per trip)
              const gdptr c = (gdptr)(uintptr_t)p.cold + (size_t)slot * 16;
              double cx = c[0], cy = c[1], cz = c[2];
              const double e3 = c[3], e4 = c[4], e5 = c[5], e7 = c[7], e8 = c[8], e15 = c[15];
              const int flags = (int)__double_as_longlong(c[13]);
              const int e_orig = (int)__double_as_longlong(c[14]);
              if (flags & 1) {
                // the owner already divided for the spatial movers' time group: same operands, same quotient
                const double f = (e7 == p.sp_t0 && e8 == p.sp_dt) ? sfsp : (stime - e7) / e8;
                cx = cx + e3 * f; cy = cy + e4 * f; cz = cz + e5 * f;
              }
              const double ocx = sox - cx, ocy = soy - cy, ocz = soz - cz;
              const double hb = ocx * sdx + ocy * sdy + ocz * sdz;
              const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - e15;
              const double disc = hb * hb - sa * cc;
              // (e15 >= 0: never a padding slot -- centre 0, r^2 = -1 -- which a `wild` ray's survivors include and which the
              // reference's rounding "hits" from origins where |o|^2 + 1 == |o|^2)
              if (disc > 0.0 && e15 >= 0.0) {  // spheres.nim:35-48
                const double root = __builtin_sqrt(disc);
                sol = (-hb - root) / sa;
                ok = (0.001 < sol) && (sol < __builtin_inf());
                if (!ok) {
                  sol = (-hb + root) / sa;
                  ok = (0.001 < sol) && (sol < __builtin_inf());
                }
              }
              if (ok) orig = e_orig;
            }
            // Merge into the owner's closest hit {t, (original index, slot)}.  t > 0, so its bit pattern orders like
            // the value.  A lane that LOWERS t knows the (index, slot) word belongs to a larger t and resets it;
            // then every lane whose root equals the owner's t (ties: duplicate objects) competes with its
            // (index << 32 | slot), the lowest original index wins.
            const unsigned long long sb = (unsigned long long)__double_as_longlong(sol);
            unsigned long long old_t = 0;
            if (ok) old_t = atomicMin(&coop_t[src], sb);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            const bool win = ok && coop_t[src] == sb;
            if (win && old_t > sb) coop_w[src] = ~0ull;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (win) atomicMin(&coop_w[src], ((unsigned long long)(unsigned)orig << 32) | (unsigned long long)slot);
            TOR_FINE(kFineC)
          };
          auto drain_c = [&](bool all) {
            while (n_surv != 0 && (all || n_surv >= 64)) {
              const unsigned n = n_surv < 64 ? n_surv : 64;
              n_surv -= n;
              if (stats_on && lane == 0) prof_lds[kStCand] += (unsigned long long)n;
              if (prof && lane == 0) prof_lds[kSecTrips] += 1;
              trip_c(n_surv, n);
            }
          };
          // appends cnt entries per lane (cnt <= 8) to a list: returns this lane's first position, bumps the count
          auto reserve = [&](unsigned cnt, unsigned& total) {
            unsigned incl, sum;
            wave_scan_u32(cnt, incl, sum);
            const unsigned at = total + incl - cnt;
            total += sum;
            return at;
          };
          // (B) one trip: pairs [base, base + n)
          auto trip_b = [&](unsigned base, unsigned n) {
            if constexpr (BLOCKS != 0) {
#ifdef TOR_FINE_PROBE
            TOR_FINE(kFineA)
            fine_state = kFineB;
#endif
            const bool mine = (unsigned)lane < n;
            const unsigned e = mine ? coop_pair[base + (unsigned)lane] : (unsigned)lane;
            const int src = (int)(e & 63u);
            const unsigned blk_id = e >> 6;
            RayF32 r;
            r.ox = __shfl(r32.ox, src); r.oy = __shfl(r32.oy, src); r.oz = __shfl(r32.oz, src);
            r.dx = __shfl(r32.dx, src); r.dy = __shfl(r32.dy, src); r.dz = __shfl(r32.dz, src);
            r.gma = __shfl(r32.gma, src); r.g = __shfl(r32.g, src);
            r.ro = 0.f; r.ro2 = 0.f; r.sa = 0.f; r.wild = 0u;
            SegF32 s;
            s.nmbl = splat2(__shfl(sp32.nmbl.x, src)); s.gk = splat2(__shfl(sp32.gk.x, src)); s.nf = splat2(__shfl(sp32.nf.x, src));
            s.wild = (unsigned)__shfl((int)sp32.wild, src);
            // a pair is (ray, BOX); a box stands for box_fanout consecutive blocks of 8 objects (tor_scene.hpp): the owner's ray
            // has travelled once, the blocks are filtered one after the other, the survivor list is drained in between so that it
            // never holds more than 64 + 512 entries
            const int fanout = kBoxFanout;
            for (int fk = 0; fk < fanout; ++fk) {
            const unsigned block_id = blk_id * (unsigned)fanout + (unsigned)fk;
            unsigned m8 = 0;
            if (mine) {
              auto filter_block = [&](auto blk, auto ST) {
                constexpr int st = decltype(ST)::value;
                // two pairs at a time: with all four in flight the 168-register variants spill inside the bounce loop
                // (and every spill store shows up as HBM write traffic: 20 GB per C2 frame, measured)
#pragma unroll 2
                for (int j = 0; j < kBlock / 2; ++j) {
                  auto rr = blk + st * j;
                  const f2v c0x = {rr[0], rr[1]}, c0y = {rr[2], rr[3]}, c0z = {rr[4], rr[5]};
                  f2v ocx, ocy, ocz;
                  if (st == 16) {
                    ocx = oc_moving32(r.ox, c0x, (f2v){rr[10], rr[11]}, s.nf);
                    ocy = oc_moving32(r.oy, c0y, (f2v){rr[12], rr[13]}, s.nf);
                    ocz = oc_moving32(r.oz, c0z, (f2v){rr[14], rr[15]}, s.nf);
                  } else {
                    ocx = oc_static32(r.ox, c0x);
                    ocy = (st == 12) ? oc_moving32(r.oy, c0y, (f2v){rr[10], rr[11]}, s.nf) : oc_static32(r.oy, c0y);
                    ocz = oc_static32(r.oz, c0z);
                  }
                  m8 = filter_pair32(r, s, ocx, ocy, ocz, (f2v){rr[6], rr[7]}, (f2v){rr[8], rr[9]}, m8);
                }
              };
              using T10 = std::integral_constant<int, 10>;
              using T12 = std::integral_constant<int, 12>;
              using T16 = std::integral_constant<int, 16>;
              const size_t off = (size_t)block_id * (size_t)p.shot32_block_stride;
              if (p.shot32_lds_floats > 0) {
                if (p.shot32_stride == 12) filter_block(shot32_lds + off, T12{});
                else if (p.shot32_stride == 10) filter_block(shot32_lds + off, T10{});
                else filter_block(shot32_lds + off, T16{});
              } else {
                const gfptr g32 = (gfptr)(uintptr_t)p.shot32;
                if (p.shot32_stride == 12) filter_block(g32 + off, T12{});
                else if (p.shot32_stride == 10) filter_block(g32 + off, T10{});
                else filter_block(g32 + off, T16{});
              }
              m8 |= s.wild;
            }
            // append the kept objects to the survivor list
            unsigned at = reserve((unsigned)__builtin_popcount(m8), n_surv);
            while (m8 != 0) {
              const int bb = 31 - __builtin_clz(m8);
              m8 &= ~(1u << bb);
              coop_surv[at++] = (unsigned)src | (((unsigned)p.spatial_base + block_id * kBlock + (unsigned)(7 - bb)) << 6);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (fk + 1 < fanout) drain_c(false);
            }  // blocks of the box
#ifdef TOR_FINE_PROBE
            TOR_FINE(kFineB)
            fine_state = kFineA;
#endif
            }
          };
          auto drain_b = [&](bool all) {
            if constexpr (BLOCKS != 0)
            for (;;) {
              // A trip appends up to 8 survivors per lane: the list has room for them only on top of FEWER THAN 64 pending ones, so
              // the survivors are drained BEFORE every trip as well as after the last one.  (Round 6: the list-building step (A) can
              // leave up to kCoopList direct survivors behind; scenes of nearly coincident spheres -- 8 direct survivors per ray and 8
              // kept objects per pair -- overran the list into the pending pairs.  One call site: trip_c is inlined here.)
              drain_c(false);
              if (!(n_pairs != 0 && (all || n_pairs >= 64))) break;
              const unsigned n = n_pairs < 64 ? n_pairs : 64;
              n_pairs -= n;
              if (stats_on && lane == 0) {
                prof_lds[kStCand] += (unsigned long long)n * kBlock * (unsigned)kBoxFanout;
                prof_lds[kStBlock] += (unsigned long long)n * kBlock * (unsigned)kBoxFanout;
              }
              if (prof && lane == 0) prof_lds[kSecTrips] += 1;
              trip_b(n_pairs, n);
            }
          };
          // (A) queue entries -> pairs / direct survivors.  One 'unit' per lane and trip: a whole entry of object
          // bits or block-box bits, or ONE bit of a super-box entry (its 8 child boxes are slab-tested here) --
          // at most 8 list entries per lane and trip, so the lists (< 64 carried over + 512) cannot overflow.
          unsigned kq = 0, sup_mask = 0, sup_block = 0;
          if constexpr (kSuper) {
            // Two-level scenes (more than 96 blocks): the slab loop left one bit per SUPER box (8 blocks) in box_mask, and
            // the 8 child boxes of every super box a ray entered still have to be slab-tested for that ray.  Pooled like
            // (B) and (C): every round packs up to 64 (ray, super box) units -- a prefix sum over the lanes' bit counts,
            // the first lanes in scan order give as many as fit -- into the free space above the pending pairs, the 64
            // lanes expand one unit each (the owner's box ray over ds_bpermute, the child boxes from LDS) and append
            // the (ray, block) pairs: at most 512 on top of fewer than 64 carried over, the list holds 576.  Rounds =
            // all the wave's units / 64 instead of the worst lane's count (measured on the 1601-object animation
            // frames: 8+ per-lane trips of ~300 instructions before).
            // (box_kind is set under `if (active)`: the test has to be made wave-uniform by hand, the block below is full
            // of cross-lane operations)
            const bool sup_lane = active && box_kind == 4;
            if (ballot64(sup_lane) != 0) {
              unsigned long long sm = sup_lane ? box_mask : 0ull;
              if (sup_lane) box_mask = 0;
              while (ballot64(sm != 0) != 0) {
#ifdef TOR_FINE_SUPER
                TOR_FINE(kFineA)
#endif
                const unsigned c = (unsigned)__builtin_popcountll(sm);
                unsigned incl, total;
                wave_scan_u32(c, incl, total);
                const unsigned excl = incl - c;
                unsigned take = excl >= 64u ? 0u : (c < 64u - excl ? c : 64u - excl);
                const unsigned n_round = total < 64u ? total : 64u;
                unsigned pos = n_pairs + excl;
                for (; take != 0; --take) {
                  const int b = __builtin_clzll(sm);  // super box b of the segment
                  sm &= ~(0x8000000000000000ull >> b);
                  coop_pair[pos++] = (unsigned)lane | ((box_group0 * kBlock + (unsigned)b) << 6);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#ifdef TOR_FINE_SUPER
                TOR_FINE(kFineSetup)
#endif
                {
                  const bool mine = (unsigned)lane < n_round;
                  const unsigned e = mine ? coop_pair[n_pairs + (unsigned)lane] : (unsigned)lane;
                  const int src = (int)(e & 63u);
                  const unsigned rec = e >> 6;  // super box `rec`: its block boxes are rec*8 .. rec*8+7
                  BoxRay32 ob;
                  ob.ix = __shfl(b32.ix, src); ob.iy = __shfl(b32.iy, src); ob.iz = __shfl(b32.iz, src);
                  ob.ax = __shfl(b32.ax, src); ob.ay = __shfl(b32.ay, src); ob.az = __shfl(b32.az, src);
                  { const float hx = __shfl(b32.hx.y, src), hy = __shfl(b32.hy.y, src), hz = __shfl(b32.hz.y, src);
                    ob.hx = (f2v){-hx, hx}; ob.hy = (f2v){-hy, hy}; ob.hz = (f2v){-hz, hz}; }
                  const unsigned owild = (unsigned)__shfl((int)r32.wild, src);
                  unsigned mc = 0;
                  if (mine) {
                    // (cs: floats between child j and child j + 1 -- 8 in the table, 6 x n_super in the transposed LDS copy)
                    auto child32 = [&](auto cb, const int cs) {
#pragma unroll 4
                      for (int j = 0; j < kBlock; ++j)
                        mc = push_cond(mc, slab_bit32(ob, (f2v){cb[cs * j + 0], cb[cs * j + 1]}, (f2v){cb[cs * j + 2], cb[cs * j + 3]},
                                                    (f2v){cb[cs * j + 4], cb[cs * j + 5]}) != 0u);
                    };
                    if (p.bnd32_lds_floats > 0) child32(bnd32_lds + (size_t)rec * 6, 6 * (p.bnd32_lds_floats / (8 * kBlock)));
                    else child32((gfptr)(uintptr_t)p.bnd32 + (size_t)rec * (8 * kBlock), 8);
                    mc |= owild;
                  }
                  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // every lane has read its unit: the space is free again
#ifdef TOR_FINE_SUPER
                  TOR_FINE(kFineF32)
#endif
                  if (prof && lane == 0) prof_lds[kSecTrips] += 1;
                  unsigned at = reserve((unsigned)__builtin_popcount(mc), n_pairs);
                  while (mc != 0) {
                    const int bb = 31 - __builtin_clz(mc);
                    mc &= ~(1u << bb);
                    coop_pair[at++] = (unsigned)src | ((rec * kBlock + (unsigned)(7 - bb)) << 6);
                  }
                  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#ifdef TOR_FINE_SUPER
                  TOR_FINE(kFineHdr)
#endif
                }
                drain_b(false);
                drain_c(false);
              }
            }
          }
          {
            // Fast path (no super-box entries in the wave, everything fits the lists): count the bits of all
            // entries, ONE prefix sum for both lists (the two counts share a word), then write.
            if (!active) box_mask = 0;
            bool has_super = kSuper && box_kind == 4 && box_mask != 0;
            unsigned cnt2 = has_super ? 0u : (unsigned)__builtin_popcountll(box_mask);  // pairs | direct survivors << 16
            for (unsigned k = 0; k < my_qn; ++k) {
              const unsigned e = q[k * 64];
              const unsigned k3 = e >> 30;
              const unsigned bits = (unsigned)__builtin_popcount(e & 0xffu);
              cnt2 += (k3 == 2) ? bits : ((k3 == 0) ? (bits << 16) : 0u);
              has_super = has_super || (kSuper && k3 == 1);
            }
            unsigned incl, total;
            wave_scan_u32(cnt2, incl, total);
            const unsigned tot_p = total & 0xffffu, tot_s = total >> 16;
            if (ballot64(has_super) == 0 && n_pairs + tot_p <= (unsigned)kCoopList && n_surv + tot_s <= (unsigned)kCoopList) {
              unsigned at_p = n_pairs + (incl & 0xffffu) - (cnt2 & 0xffffu);
              unsigned at_s = n_surv + (incl >> 16) - (cnt2 >> 16);
              n_pairs += tot_p;
              n_surv += tot_s;
              while (box_mask != 0) {
                const int b = __builtin_clzll(box_mask);  // box b of the segment
                box_mask &= ~(0x8000000000000000ull >> b);
                coop_pair[at_p++] = (unsigned)lane | ((box_group0 * kBlock + (unsigned)b) << 6);
              }
              for (; kq < my_qn; ++kq) {
                const unsigned e = q[kq * 64];
                const unsigned blk = (e >> 8) & 0x3fffffu;
                unsigned m = e & 0xffu;
                if ((e >> 30) == 2) {
                  while (m != 0) {
                    const int b = 31 - __builtin_clz(m);
                    m &= ~(1u << b);
                    coop_pair[at_p++] = (unsigned)lane | ((blk * kBlock + (unsigned)(7 - b)) << 6);
                  }
                } else {
                  while (m != 0) {
                    const int b = 31 - __builtin_clz(m);
                    m &= ~(1u << b);
                    coop_surv[at_s++] = (unsigned)lane | ((blk * kBlock + (unsigned)(7 - b)) << 6);
                  }
                }
              }
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
          }
          for (;;) {
            unsigned kind = 3, m = 0, blk = 0;  // 3: nothing this trip
            if (kSuper && sup_mask != 0) {
              const int b = 31 - __builtin_clz(sup_mask);
              sup_mask &= ~(1u << b);
              const unsigned rec = sup_block * kBlock + (unsigned)(7 - b);  // super box `rec`: its block boxes are rec*8 .. rec*8+7
              unsigned mc = 0;
              auto child32 = [&](auto cb, const int cs) {
#pragma unroll 4
                for (int j = 0; j < kBlock; ++j)
                  mc = push_cond(mc, slab_bit32(b32, (f2v){cb[cs * j + 0], cb[cs * j + 1]}, (f2v){cb[cs * j + 2], cb[cs * j + 3]},
                                              (f2v){cb[cs * j + 4], cb[cs * j + 5]}) != 0u);
              };
              if (p.bnd32_lds_floats > 0) child32(bnd32_lds + (size_t)rec * 6, 6 * (p.bnd32_lds_floats / (8 * kBlock)));
              else child32((gfptr)(uintptr_t)p.bnd32 + (size_t)rec * (8 * kBlock), 8);
              mc |= r32.wild;
              kind = 2; m = mc; blk = rec;
            } else if (box_mask != 0) {
              const int g = __builtin_clzll(box_mask) >> 3;  // group of 8 boxes
              const unsigned mm = (unsigned)(box_mask >> (56 - 8 * g)) & 0xffu;
              box_mask &= ~(0xffull << (56 - 8 * g));
              if (kSuper && box_kind == 4) { sup_mask = mm; sup_block = box_group0 + (unsigned)g; kind = 4; }
              else { kind = 2; m = mm; blk = box_group0 + (unsigned)g; }
            } else if (kq < my_qn) {
              const unsigned e = q[kq * 64];
              kq += 1;
              const unsigned k3 = e >> 30;  // 0: object mask, 2: block boxes, 1: super boxes
              if (kSuper && k3 == 1) { sup_mask = e & 0xffu; sup_block = (e >> 8) & 0x3fffffu; kind = 4; }  // expanded bit by bit from the next trip on
              else { kind = k3; m = e & 0xffu; blk = (e >> 8) & 0x3fffffu; }
            }
            if (ballot64(kind != 3) == 0) break;
            const unsigned n_bits = (unsigned)__builtin_popcount(m);
            unsigned at_p = reserve(kind == 2 ? n_bits : 0u, n_pairs);
            unsigned at_s = reserve(kind == 0 ? n_bits : 0u, n_surv);
            if (kind != 0 && kind != 2) m = 0;
            while (m != 0) {
              const int b = 31 - __builtin_clz(m);
              m &= ~(1u << b);
              const unsigned id = blk * kBlock + (unsigned)(7 - b);  // block id, or cold slot of a direct candidate
              if (BLOCKS != 0 && kind == 2) coop_pair[at_p++] = (unsigned)lane | (id << 6);
              else coop_surv[at_s++] = (unsigned)lane | (id << 6);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            drain_b(false);
            drain_c(false);
          }
          drain_b(true);
          drain_c(true);

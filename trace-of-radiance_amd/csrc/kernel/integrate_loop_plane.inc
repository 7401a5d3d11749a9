// integrate_loop_plane.inc -- object loop of integrate_kernel, ARITH 2, every segment that carries a plane table (xkind 10-14;
// KParams.xpl -- TOR_PLANE=0 and segments the plane would not thin out take the wave-uniform loops instead: see the gate in
// tor_kernels.hip).
//   STAGE ONE, wave-uniform: every object through the PLANE screen (tor_screen.hpp: plane_word / plane_word_mov) -- the distance
//     of its centre's ground projection from the ray's ground track, from {cx', cz'} alone (float32 offsets from the segment's
//     origin, 8 bytes through the scalar data path -- the whole words' requests by hand, a group of 8 ahead, the blocks' one record
//     ahead; plane_word32: 2 v_fma_f32 + 1 v_sub_f32 + the v_alignbit per object)
//     for statics and movers along y at ANY height, from
//     {c0x, c0z, dcx, dcz} (32 bytes, 5 + 1 instructions) for movers whose centre travels in x or z.  Keeps the spheres within R of
//     the ground track: ~9 of random_scene's 481 per query.  Whole words (32 slots) run without the per-block bookkeeping.
//   STAGE TWO, per lane: the bits stage one left in the segment's words (LDS, and the running word) go through the test the
//     wave-uniform loop would have run on every object of that segment -- the screen's second form for xkind 10 / 11 / 12
//     (32-byte records), its first form for xkind 13 / 14 (64-byte records {c0, r^2, dc}) -- on records read per lane; a
//     candidate that fails has its bit cleared.  What is left is what that test alone leaves (its proof covers stage one:
//     tor_screen.hpp), so the resolve pass and the canvas do not change.
// In scope: sray, pray, seg, i, seg_count, seg_real, seg_block0, xkind, time, segs, q / mw / nz / w_count / w_base / gb_next
// (TOR_WORDS_END_BLOCK), full, plane_ran, xstaged / stage, a, scr_d1 (first-form margins).
            if constexpr (kWords) {
            const int x_first = h_xfirst;
            const int pl_first = h_plfirst;
            const bool mover = xkind >= 12;  // the segment's centres depend on the ray's time (wave-uniform)
            double f = 0.0;
            if (mover) {
              f = (time - SEG_T0) / SEG_DT;  // moving_spheres.nim:42
              fc_f = f; fc_t0 = double_to_bits(SEG_T0); fc_dt = double_to_bits(SEG_DT);
            }
            const int i_begin = i;  // first object of the segment this pass tests (wave-uniform)
            {
              const PlaneSeg ps = plane_seg(sray, pray, SEG_REACH, SEG_TRAVEL, f, h_rmax2);
              // (generic over the record: PW = 2 float32 {cx', cz'} relative to the segment's origin -- plane_word32 -- or 4 float64
              // {c0x, c0z, dcx, dcz} for xkind 13; the header's last four slots: the first float32 record, Ox, Oz, {E, Cm} (tor_scene.hpp)
              // or the first float64 record)
              auto stage_one = [&](auto PWc) {
                constexpr int PW = decltype(PWc)::value;
                using Rec = std::conditional_t<PW == 2, float, double>;
                using RecPtr = std::conditional_t<PW == 2, cfptr, cdptr>;
                RecPtr rec = (RecPtr)(uintptr_t)(PW == 2 ? (const void*)p.xpl32 : (const void*)p.xpl) + ((long)pl_first + PW * (long)i);
                PlaneSeg32 ps32{};
                Rec n0, n1, n2 = 0, n3 = 0;
                if constexpr (PW == 2) {
                  ps32 = plane_seg32(sray, ps, h_r1, h_r2, (double)__int_as_float(__double2loint(h_r3)), (double)__int_as_float(__double2hiint(h_r3)));
                  n0 = __int_as_float(__double2loint(h_r0)); n1 = __int_as_float(__double2hiint(h_r0));
                } else {
                  n0 = h_r0; n1 = h_r1; n2 = h_r2; n3 = h_r3;
                }
                // the first record: from the segment's header (already here) at the segment's start, from the table when a pass
                // resumes inside the segment (wave-uniform)
                if (i != 0) {
                  n0 = rec[0]; n1 = rec[1];
                  if constexpr (PW == 4) { n2 = rec[2]; n3 = rec[3]; }
                }
                auto one = [&](unsigned m, int j) {  // object j of the block at rec; requests object j + 1 (one record of slack behind the table)
                  const Rec c0 = n0, c1 = n1, c2 = n2, c3 = n3;
                  n0 = rec[PW * (j + 1) + 0]; n1 = rec[PW * (j + 1) + 1];
                  if constexpr (PW == 4) {
                    n2 = rec[PW * (j + 1) + 2]; n3 = rec[PW * (j + 1) + 3];
                    return push_bit(m, plane_word_mov(ps, c0, c1, c2, c3));
                  } else {
                    (void)c2; (void)c3;
                    return push_bit(m, plane_word32(ps32, c0, c1));
                  }
                };
                // Three phases, so that the whole words -- 15 of random_scene's 16 -- run in a loop whose scalar side is a counter, the
                // table pointer and the record requests (the single loop that decided "word or block?" per trip spent ~45 scalar
                // instructions per word on that decision and on values both arms kept alive; a wave alone on its SIMD issues vector
                // instructions only 41 % of the time, the rest goes to scalar instructions and waits: profiles/r5_occupancy.txt):
                //   blocks of 8 up to the next word boundary of the sorted list, whole words, blocks of 8 to the segment's end.
                int gb = seg_block0 + (int)((unsigned)i / (unsigned)kBlock);  // block index of object i in the sorted list
                for (;;) {
                  // (the segment's last block runs over its padding too: at 4 instructions per slot the padding -- centres at 1e300 (2^100 in float32),
                  // kept by no ray that has a ground track -- is cheaper than a loop over the real objects, whose requests cannot
                  // run ahead; a ray that keeps everything keeps the padding too and stage two, or the exact test, drops it)
                  while (i < seg_count && ((gb & 3) != 0 || seg_count - i < 4 * kBlock)) {
                    unsigned m = mw;
                    if (seg_real - i <= kBlock / 2) {  // the segment's last block, at most half of it real: the first four slots only
#pragma unroll
                      for (int j = 0; j < kBlock / 2; ++j) m = one(m, j);
                      m <<= (unsigned)(kBlock / 2);
                    } else {
#pragma unroll
                      for (int j = 0; j < kBlock; ++j) m = one(m, j);
                    }
                    rec += PW * kBlock;
                    mw = m;
                    gb_next = gb + 1;
                    i += kBlock;
                    if ((gb & 3) == 3) {
                      q[(unsigned)w_count * 64] = m;
                      nz = push_cond(nz, m != 0u);
                      w_count += 1;
                      if (w_count == kQCap) { full = true; break; }
                    }
                    gb += 1;
                  }
                  if (full || i >= seg_count) break;
                  // whole words -- of real objects or of the padding behind them (the host pads a long tail to a word: tor_scene.cpp) --
                  // as many as the segment holds and the pass has slots for
                  int nw = (seg_count - i) / (4 * kBlock);
                  nw = nw < kQCap - w_count ? nw : kQCap - w_count;
                  unsigned m = 0;
                  int w = 0;
                  if constexpr (PW == 2 && kPlaneAhead == 1) {
                    // The float32 records by hand: one s_load_dwordx16 per group of 8 objects, requested a whole group ahead of
                    // the wait that needs it (two 16-dword buffers in turn; left to the compiler the request sits one object
                    // ahead, and the first one of a trip right in front of its wait).  A request is in flight only inside
                    // straight-line code: every trip begins and ends with `ra` landed, so no register the scalar cache still
                    // writes crosses a branch, where the compiler may copy it.  The running mask goes through every statement: the
                    // v_alignbit chain pins a group's objects between its two statements.  The last request of a segment reads
                    // the group behind it: the next segment's records or the table's slack (kPlaneSlackFloats), used by nobody.
#if TOR_REACH
                    // THE REACH PASS (tor_screen.hpp reach_ray): which of the nw words can a ray of this wave be near at all?  The
                    // lane's piece of ray inside the segment's height slab, as a box in xz, against the words' boxes (KParams.xwb:
                    // one 32-byte record per word through the scalar path, four float32 compares each).  reach_l: the lane's bits
                    // (bit w <-> word w of this phase), the ONE register the word loop carries for it; reach_w: the wave's.
                    // Words nobody reaches are not walked: no record request, no object instruction, no store; their summary bits
                    // are shifted in clear, and reach_skip keeps them out of the summary's rebuild after stage two (a stale word
                    // of an earlier query would come back as candidates).  A walked word costs what it
                    // cost, one word per trip: its four requests a whole group ahead of their waits, the fourth one being the first
                    // group of the NEXT word to walk (the group behind this word when there is none, as before), `ra` landed at
                    // both ends of a trip, so no request crosses a branch.  A lane's bits in a word it does not reach itself are
                    // cleared before the word is stored: stage two would drop them one by one.
                    // (kReach: the ARITH 3 builds, launched for layouts with a segment that asks for the pass; h_rpass: the host's word for
                    // this segment -- tor_scene.cpp: a thin height slab over a wide field and enough whole words to pay for the pass;
                    // the other segments of such a layout walk every word, one per trip; the ARITH 2 builds run the two-word trips below)
                    if constexpr (kReach) {
                    if (nw > 0) {
                      typedef float __attribute__((ext_vector_type(16))) f16v;
                      f16v ra, rb;
                      unsigned reach_l = ~0u, reach_w = (2u << (unsigned)(nw - 1)) - 1u;
                      if (h_rpass) {
                        reach_l = 0; reach_w = 0;
                        const cfptr wb = (cfptr)(uintptr_t)p.xwb + (long)kReachRecFloats * (long)((unsigned)(seg_block0 * kBlock + i) >> 5);
                        const cdptr wy = (cdptr)(wb + 4);
                        const ReachRay rr = reach_ray(sray, !(ps32.T < __builtin_inff()), sray.s1 + SEG_REACH + SEG_TRAVEL * __builtin_fabs(f), h_r1, h_r2, wy[0], wy[1], f);
                        // (four records per trip: their requests go out together, one wait for the four; the last trip may read up to
                        // three records behind the pass's words -- the next words' or the table's slack, kReachSlackWords -- whose bits
                        // are masked off below)
#pragma unroll 1
                        for (int k = 0; k < nw; k += 4) {
#pragma unroll
                          for (int j = 0; j < 4; ++j) {
                            const cfptr b = wb + kReachRecFloats * (k + j);
                            const bool hit = !reach_miss(rr, b[0], b[1], b[2], b[3]);
                            reach_l |= hit ? 1u << (unsigned)(k + j) : 0u;
                            reach_w |= ballot64(hit) != 0 ? 1u << (unsigned)(k + j) : 0u;
                          }
                        }
                        reach_w &= (2u << (unsigned)(nw - 1)) - 1u;
                      }
                      // The words nobody reaches are NOT written: what they hold is a word of an earlier query.  Their summary bits
                      // are shifted in clear below, and the summary's rebuild after stage two (tor_kernels.hip, `plane_ran`) leaves
                      // them out by this mask, kept across the segments of a pass and begun afresh with every pass.  Nobody else
                      // reads such a word: the resolve and stage two's walk go by the summary; `shared_word` / `sat_out` touch the
                      // first word of a segment's stretch when it began in the block phase, `partial` the running word -- words
                      // the block phases of this pass stored, never a whole word of this loop.
                      if constexpr (kReachNoZero == 1) {
                        reach_skip |= (~reach_w & ((2u << (unsigned)(nw - 1)) - 1u)) << (unsigned)w_count;
                      } else if constexpr (kReachNoZero == 0) {
                        for (unsigned z = ~reach_w & ((2u << (unsigned)(nw - 1)) - 1u); z != 0u; z &= z - 1u)
                          q[(unsigned)(w_count + __builtin_ctz(z)) * 64] = 0u;
                      }
                      if (stats_on && lane == 0) {  // debug counters (tor_debug_last_reach): whole words walked, whole words met
                        atomicAdd(p.stats + 11, (unsigned long long)__builtin_popcount(reach_w));
                        atomicAdd(p.stats + 12, (unsigned long long)nw);
                      }
#define TOR_FEEDP_REQ(nxt, ptr, off) asm volatile("s_load_dwordx16 %0, %3, %4" : "=&s"(nxt), "+v"(m), "+v"(mp) : "s"(ptr), "i"(off))
#define TOR_FEEDP_WAIT(cur) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(cur), "+v"(m), "+v"(mp))
#define TOR_FEEDP_WAITREQ(cur, nxt, ptr, off) \
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_load_dwordx16 %1, %4, %5" : "+s"(cur), "=&s"(nxt), "+v"(m), "+v"(mp) : "s"(ptr), "i"(off))
                      auto grp = [&](const f16v& b) {
#pragma unroll
                        for (int j = 0; j < kBlock; ++j) m = push_bit(m, plane_word32(ps32, b[2 * j], b[2 * j + 1]));
                      };
                      unsigned mp = 0;
                      unsigned left = reach_w;  // the words still to walk
                      int cur = -1;             // the last word walked
                      if (left != 0u) {
                        cur = __builtin_ctz(left);
                        left &= left - 1u;
                        RecPtr rc = rec + PW * 4 * kBlock * cur;
                        TOR_FEEDP_REQ(ra, rc, 0);
                        TOR_FEEDP_WAIT(ra);
#pragma unroll 1
                        for (;;) {
                          const int nxt = left != 0u ? __builtin_ctz(left) : cur + 1;
                          const RecPtr rn = rec + PW * 4 * kBlock * nxt;
                          m = 0;
                          TOR_FEEDP_REQ(rb, rc, 64); grp(ra);
                          TOR_FEEDP_WAITREQ(rb, ra, rc, 128); grp(rb);
                          TOR_FEEDP_WAITREQ(ra, rb, rc, 192); grp(ra);
                          TOR_FEEDP_WAITREQ(rb, ra, rn, 0); grp(rb);
                          mp = m & (unsigned)((int)(reach_l << (unsigned)(31 - cur)) >> 31);
                          // (a finished word is stored BEHIND the wait, not in front of it: the wait counts LDS writes too)
                          TOR_FEEDP_WAIT(ra);
                          q[(unsigned)(w_count + cur) * 64] = mp;
                          nz = push_cond(nz << (unsigned)(cur - w), mp != 0u);
                          w = cur + 1;
                          if (left == 0u) break;
                          left &= left - 1u;
                          cur = nxt;
                          rc = rn;
                        }
                      }
                      nz <<= (unsigned)(nw - w);
                      w = nw;
                      rec += PW * 4 * kBlock * nw;
#undef TOR_FEEDP_REQ
#undef TOR_FEEDP_WAIT
#undef TOR_FEEDP_WAITREQ
                      // the first record behind the words, for the blocks that follow: in `ra` when the last word was walked
                      if (cur == nw - 1) { n0 = ra[0]; n1 = ra[1]; }
                      else { n0 = rec[0]; n1 = rec[1]; }
                      m = mp;
                    }
                    } else
#endif
                    if (nw > 0) {
                      typedef float __attribute__((ext_vector_type(16))) f16v;
                      f16v ra, rb;
#define TOR_FEED_REQ(nxt, off) asm volatile("s_load_dwordx16 %0, %3, %4" : "=&s"(nxt), "+v"(m), "+v"(mp) : "s"(rec), "i"(off))
#define TOR_FEED_WAIT(cur) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(cur), "+v"(m), "+v"(mp))
#define TOR_FEED_WAIT_REQ(cur, nxt, off) \
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_load_dwordx16 %1, %4, %5" : "+s"(cur), "=&s"(nxt), "+v"(m), "+v"(mp) : "s"(rec), "i"(off))
                      auto grp = [&](const f16v& b) {
#pragma unroll
                        for (int j = 0; j < kBlock; ++j) m = push_bit(m, plane_word32(ps32, b[2 * j], b[2 * j + 1]));
                      };
                      // (a finished word is stored BEHIND the next wait, not in front of it: the wait counts LDS writes too)
                      unsigned mp = 0;
                      auto store = [&]() {
                        q[(unsigned)(w_count + w) * 64] = mp;
                        nz = push_cond(nz, mp != 0u);
                        w += 1;
                      };
                      TOR_FEED_REQ(ra, 0);
                      TOR_FEED_WAIT(ra);
#pragma unroll 1
                      while (w + 2 <= nw) {
                        m = 0;
                        TOR_FEED_REQ(rb, 64); grp(ra);
                        TOR_FEED_WAIT_REQ(rb, ra, 128); grp(rb);
                        TOR_FEED_WAIT_REQ(ra, rb, 192); grp(ra);
                        TOR_FEED_WAIT_REQ(rb, ra, 256); grp(rb);
                        mp = m;
                        m = 0;
                        TOR_FEED_WAIT_REQ(ra, rb, 320); store(); grp(ra);
                        TOR_FEED_WAIT_REQ(rb, ra, 384); grp(rb);
                        TOR_FEED_WAIT_REQ(ra, rb, 448); grp(ra);
                        TOR_FEED_WAIT_REQ(rb, ra, 512); grp(rb);
                        mp = m;
                        TOR_FEED_WAIT(ra); store();
                        rec += PW * 8 * kBlock;
                      }
                      if (w < nw) {
                        m = 0;
                        TOR_FEED_REQ(rb, 64); grp(ra);
                        TOR_FEED_WAIT_REQ(rb, ra, 128); grp(rb);
                        TOR_FEED_WAIT_REQ(ra, rb, 192); grp(ra);
                        TOR_FEED_WAIT_REQ(rb, ra, 256); grp(rb);
                        mp = m;
                        TOR_FEED_WAIT(ra); store();
                        rec += PW * 4 * kBlock;
                      }
#undef TOR_FEED_REQ
#undef TOR_FEED_WAIT
#undef TOR_FEED_WAIT_REQ
                      n0 = ra[0]; n1 = ra[1];  // the first record behind the words, for the blocks that follow
                    }
                  } else {
                  auto word = [&]() {
                    m = 0;
#pragma unroll
                    for (int j = 0; j < 4 * kBlock; ++j) m = one(m, j);
                    rec += PW * 4 * kBlock;
                    q[(unsigned)(w_count + w) * 64] = m;
                    nz = push_cond(nz, m != 0u);
                    w += 1;
                  };
                  // (two words per trip: the loop's own counter, compare and branch are a seventh of a word's scalar instructions)
#pragma unroll 1
                  while (w + 2 <= nw) { word(); word(); }
                  if (w < nw) word();
                  }
                  mw = m;
                  i += nw * 4 * kBlock;
                  gb += 4 * nw;
                  gb_next = gb;
                  w_count += nw;
                  if (w_count == kQCap) { full = true; break; }
                }
              };
              if (xkind == 13) stage_one(std::integral_constant<int, 4>{});
              else stage_one(std::integral_constant<int, 2>{});
            }
            // ---- stage two: slots [slot_a, slot_b) of the sorted list, in words k_a .. k_b of this pass
            {
              const int slot0 = seg_block0 * kBlock;                   // the segment's first slot
              const int slot_a = slot0 + i_begin, slot_b = slot0 + i;  // (i: behind the last object tested, also after `full`)
              const int nb = gb_next & 3;                              // blocks in the running word
              const bool partial = !full && nb != 0;                   // (after `full` the last word has just been stored)
              unsigned nzl = nz;  // bit (k_b - k) <-> word k of this pass is not empty
              if (partial) {      // the running word joins the stored ones for the walk below
                const unsigned placed = mw << (unsigned)(8 * (4 - nb));
                q[(unsigned)w_count * 64] = placed;
                nzl = push_cond(nzl, placed != 0u);
              }
              const int k_a = (slot_a >> 5) - w_base, k_b = ((slot_b - 1) >> 5) - w_base;
              nzl &= (2u << (unsigned)(k_b - k_a)) - 1u;  // the words that hold slots of this segment (slot_b == slot_a -- a pass that begins at the segment's end -- makes this, like everything below, a value nobody reads)
              // word k_a may begin with slots of the segment before (already through ITS screen): they sit out the walk
              const bool shared_word = slot_b > slot_a && (slot_a & 31) != 0;
              unsigned sat_out = 0;
              if (shared_word) {
                const unsigned first_mask = 0xffffffffu >> (unsigned)(slot_a & 31);  // the slots from slot_a on
                const unsigned w = q[(unsigned)k_a * 64];
                sat_out = w & ~first_mask;
                q[(unsigned)k_a * 64] = w & first_mask;
              }
              // the lane's walk over its candidate bits: its word, the bits of it still to look at, where that word lives
              int k = k_a;
              unsigned cur = 0;
              unsigned* wp = q;
              const unsigned last_slot = (unsigned)(slot_b - 1);
              struct Pick { bool v; unsigned* w; int b; unsigned slot; };
              auto pick = [&]() {  // the next candidate of the lane (v = false: none; the slot then stays inside the segment)
                if (cur == 0 && nzl != 0) {
                  const int wb = 31 - __builtin_clz(nzl);
                  nzl &= ~(1u << wb);
                  k = k_b - wb;
                  wp = q + (unsigned)k * 64;
                  cur = *wp;
                }
                Pick c;
                c.v = cur != 0;
                c.b = 31 - __builtin_clz(cur | 1u);
                cur &= ~(1u << c.b);
                c.w = wp;
                const unsigned slot = ((unsigned)(w_base + k) << 5) + (unsigned)(31 - c.b);
                c.slot = slot < last_slot ? slot : last_slot;
                return c;
              };
              unsigned long long s2_t0 = 0;
              if (prof && lane == 0) s2_t0 = __builtin_readcyclecounter();
              if (slot_b > slot_a && xkind <= 12) {
                // ---- second form on 32-byte records {cx, cy, cz, K} | {cx, cz, K'} | {cx, cz, K', dcy}
                const ScreenSeg ss = screen2_seg(sray, SEG_REACH, SEG_TRAVEL, h_y, f);
                // (generic over where the records live: LDS -- KParams.xrec_lds_doubles -- or global memory)
                // ... and over the segment's kind (a compile-time constant inside the loop: with the kind tested per trip the loop
                // was a ladder of scalar branches around three out-of-line tests, and 20 % slower -- measured, round 5)
                auto stage_two = [&](auto xr, auto KINDc) {  // record of sorted slot s: xr + 4 s
                  constexpr int KIND = decltype(KINDc)::value;
                  struct Cand { bool v; unsigned* w; int b; double r0, r1, r2, r3; };  // the candidate's word and bit
                  constexpr bool kRecLds = std::is_same<decltype(xr), ldptr>::value;
                  // (LDS: the table's byte address as an opaque per-lane value, so that a record's four float64 are two reads off ONE
                  // address register + immediate offsets instead of two address computations)
                  unsigned lds_base = 0;
                  if constexpr (kRecLds) {
                    lds_base = (unsigned)(uintptr_t)xr;
                    asm volatile("" : "+v"(lds_base));
                  }
                  // The next candidate of the lane and its record: loads that stay in flight while the candidate before is tested.
                  // No branch around the loads -- a lane without a candidate reads some record of the segment -- so that the number
                  // of loads in flight is known at compile time (behind a branch the test would wait for ALL of them).
                  auto fetch = [&](Cand& c) {
                    const Pick pk = pick();
                    c.v = pk.v; c.w = pk.w; c.b = pk.b;
                    if constexpr (kRecLds) {
                      const ldptr r = (ldptr)(uintptr_t)(lds_base + pk.slot * 32u);
                      c.r0 = r[0]; c.r1 = r[1]; c.r2 = r[2]; c.r3 = r[3];
                    } else {
                      const auto r = xr + 4 * (long)pk.slot;
                      c.r0 = r[0]; c.r1 = r[1]; c.r2 = r[2]; c.r3 = r[3];
                    }
                  };
                  // (the arithmetic runs for every lane, candidate or not: under `if (c.v)` a trip in which no lane has one would
                  // jump over the wait for the record as well, and the compiler would then wait for everything before the next fetch)
                  auto test = [&](const Cand& c) {
                    const int word = KIND == 12   ? screen2_movy_y<true>(ss, c.r0, c.r1, c.r2, c.r3)
                                     : KIND == 11 ? screen2_static_y<true>(ss, c.r0, c.r1, c.r2)
                                                  : screen2_static<true>(ss, c.r0, c.r1, c.r2, c.r3);
                    if (c.v && word >= 0) atomicAnd(c.w, ~(1u << c.b));  // dropped (the lane's own LDS word: ds_and_b32)
                  };
                  Cand ca{false, q, 0, 0.0, 0.0, 0.0, 0.0}, cb{false, q, 0, 0.0, 0.0, 0.0, 0.0};
                  fetch(ca);
                  for (;;) {
                    if (ballot64(ca.v || nzl != 0) == 0) break;
                    fetch(cb);
                    test(ca);
                    if (ballot64(cb.v || nzl != 0) == 0) break;
                    fetch(ca);
                    test(cb);
                  }
                };
                auto run = [&](auto KINDc) {
                  if (xstaged) stage_two((ldptr)stage + ((long)x_first - 4 * (long)slot0), KINDc);
                  else stage_two((gdptr)(uintptr_t)p.xrec + ((long)x_first - 4 * (long)slot0), KINDc);
                };
                if (xkind == 12) run(std::integral_constant<int, 12>{});
                else if (xkind == 11) run(std::integral_constant<int, 11>{});
                else run(std::integral_constant<int, 10>{});
                plane_ran = true;
              } else if (slot_b > slot_a) {
                // ---- first form on 64-byte records {c0 xyz, r^2, dc xyz, 0} (xkind 13: any mover; 14: a mover along y whose
                // segment has no common height): what integrate_loop_f64_movers.inc runs wave-uniform, per lane here.  One candidate
                // at a time: seven float64 per record, two of them in flight would cost the kernel its register budget.
                double negmu, am;
                screen_margins(scr_s1 + SEG_REACH + SEG_TRAVEL * __builtin_fabs(f), scr_d1, a, negmu, am);
                const double neg_f = -f;
                auto stage_two = [&](auto xr) {  // record of sorted slot s: xr + 8 s
                  constexpr bool kRecLds = std::is_same<decltype(xr), ldptr>::value;
                  unsigned lds_base = 0;
                  if constexpr (kRecLds) {
                    lds_base = (unsigned)(uintptr_t)xr;
                    asm volatile("" : "+v"(lds_base));
                  }
                  for (;;) {
                    const Pick pk = pick();
                    if (ballot64(pk.v || nzl != 0) == 0) break;  // (a lane whose word came up empty -- its bits belong to a neighbour segment -- may still hold further words)
                    double r0, r1, r2, r3, r4, r5, r6;
                    if constexpr (kRecLds) {
                      const ldptr r = (ldptr)(uintptr_t)(lds_base + pk.slot * 64u);
                      r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3]; r4 = r[4]; r5 = r[5]; r6 = r[6];
                    } else {
                      const auto r = xr + 8 * (long)pk.slot;
                      r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3]; r4 = r[4]; r5 = r[5]; r6 = r[6];
                    }
                    const int word = screen_filter(fma_(neg_f, r4, ox - r0), fma_(neg_f, r5, oy - r1), fma_(neg_f, r6, oz - r2), dx, dy, dz, a, negmu, am, r3);
                    if (pk.v && word >= 0) atomicAnd(pk.w, ~(1u << pk.b));
                  }
                };
                if (xstaged) stage_two((ldptr)stage + ((long)x_first - 8 * (long)slot0));
                else stage_two((gdptr)(uintptr_t)p.xrec + ((long)x_first - 8 * (long)slot0));
                plane_ran = true;
              }
              if (prof && lane == 0) prof_lds[kSecStage2] += __builtin_readcyclecounter() - s2_t0;
              if (shared_word) q[(unsigned)k_a * 64] |= sat_out;
              if (partial) mw = q[(unsigned)w_count * 64] >> (unsigned)(8 * (4 - nb));
            }
            }  // kWords

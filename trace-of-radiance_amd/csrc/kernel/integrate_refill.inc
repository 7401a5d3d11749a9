// integrate_refill.inc -- section (A) of integrate_kernel's bounce iteration (textually included, tor_kernels.hip): lanes without a live path
// get the next work item -- a wave-uniform range pulled from the global counter (SEED_PIXEL: tiles in chain-length order;
// SEED_SAMPLE / probe: guided chunks) dealt out by ballot + prefix count -- and start its camera ray (render.nim:59-66).  The float64
// brute force with sample streams (kRes) starts its camera rays 64 at a time into a per-wave LDS reservoir instead and pops from it.
// SEEDING 4 (kList) walks a pixel list: the work index is list slot x spp + sample, and both seeding sites look the slot's pixel up.
// SEEDING 7 (kList on the pixel streams) walks it in tiles of 64 consecutive list slots (KParams.total_work = the list's length; the last
// tile may be partial): state is loaded and stored by the slot's PIXEL, and an entry outside the shard never becomes a work item.
// Reads / writes the lane state declared in integrate_kernel (active, have_item, o, d, time, rng, row, col, s, pix, acc, ...).
    // ================= (A) refill lanes that have no live path =========================
    // (the cooperative variants -- both exact accelerations, 168 registers and none to spare -- keep the integer division: the
    // float64 reciprocal form needs two more register pairs here and put a scratch STORE inside their bounce loop, 15 GB of HBM
    // writes per configs[2] frame at unchanged speed: profiles/r5_c3_accel3_summary.txt before the fix)
#define TOR_UDIV(n, d, inv) (coop_variant(F32, BLOCKS) ? (unsigned)(n) / (unsigned)(d) : udiv_by((n), (inv)))
    // ---- kRes variants (TOR_SEED_SAMPLE, float64 brute force): camera rays come from a per-wave RESERVOIR in LDS ----------------
    // A sample's stream depends on (pixel, sample) alone, so the wave can start samples ahead of need: when the reservoir runs
    // dry ALL 64 lanes fetch a sample each and run seed3, the two film coordinates (two float64 divisions), the lens rejection
    // loop and the time draw (render.nim:59-66, cameras.nim:47-57) -- every lane busy -- and park {generator state, lens offset,
    // film coordinates, time, pixel} in LDS; a lane whose path ended pops one entry (ten LDS reads) and finishes cameras.nim:49-55
    // from it.  Before, that code ran on every bounce iteration for the ~20 lanes of 64 that had just ended: 8.7 % of the frame
    // at 31 % lane occupancy (profiles/r5_section_probe_c2x50.txt).  Same operations in the same order per sample: same canvas.
    if constexpr (kRes) {
      const unsigned long long need_mask = ballot64(!active);
      if (need_mask != 0) {
        const unsigned want = (unsigned)__builtin_popcountll(need_mask);
        const unsigned prefix = lane_prefix(need_mask);
        // (the reservoir's state and the work range are the same in every lane, but they are updated inside this loop under
        // conditions the compiler cannot prove uniform: left alone it carried them in vector registers and compiled this section
        // as divergent control flow -- exec-mask juggling around every step, a lane-by-lane scan in front of the atomic.
        // readfirstlane at the section's entry keeps the section scalar.)
        auto rfl = [](unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
        unsigned rc = rfl(res_cnt), rh = rfl(res_head);
        // lanes first <= prefix < first + count take the entries rh + (prefix - first)
        auto pop = [&](unsigned first, unsigned count) {
          if (!active && prefix >= first && prefix < first + count) {
            const unsigned e = rh + (prefix - first);
            rng.s0 = res_rng[e]; rng.s1 = res_rng[64 + e]; rng.s2 = res_rng[128 + e]; rng.s3 = res_rng[192 + e];
            const double rdx = res_f[e], rdy = res_f[64 + e], fs = res_f[128 + e], ft = res_f[192 + e];
            time = res_f[256 + e];
            if constexpr (kList) {  // (the reservoir keeps the list slot; the pixel is looked up again here -- same LDS layout as SEEDING 1 / 3)
              const unsigned lp = (unsigned)p.pixel_list[res_pl0[0] + (unsigned)res_dp[e]];
              pix = lp < p.n_pixels ? (int)lp : -1;  // an entry outside the shard deposits nothing (tag -1: never flushed)
            } else {
              pix = (int)(res_pl0[0] + (unsigned)res_dp[e]);
            }
            const Camera cam = load_camera(p.cam_dev);
            const V3 offset = cam.u * rdx + cam.v * rdy;  // cameras.nim:49-55
            o = cam.origin + offset;
            d = cam.lower_left_corner + cam.horizontal * fs + cam.vertical * ft - cam.origin - offset;
            set_att(v3(1.0, 1.0, 1.0));  // render.nim:22
            depth = 0;
            active = true;
          }
        };
        const unsigned take1 = want < rc ? want : rc;
        if (take1 != 0) {
          pop(0u, take1);
          rh += take1;
          rc -= take1;
        }
        if (take1 < want) {
          // the reservoir is empty and lanes still wait: start the next (up to) 64 samples
          unsigned long long wn = bcast_first_u64(w_next), we = bcast_first_u64(w_end);
          unsigned cpl = rfl(cur_pl), cs = rfl(cur_s), nch = rfl(next_chunk);
          bool ex = rfl(exhausted ? 1u : 0u) != 0u;
          if (wn >= we && !ex) {
            // guided self-scheduling, the chunk shrinks with the work that is left (waves of one SIMD get very unequal service, so
            // anything parked in a slow wave becomes the tail of the frame); whole pixels per grab where the chunk allows it: a
            // pixel's samples then meet in ONE wave's LDS accumulator and reach HBM in one flush
            unsigned grab = nch;
            if (grab >= (unsigned)p.spp) grab = rfl(udiv_by(grab, p.inv_spp)) * (unsigned)p.spp;
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(p.work_counter, (unsigned long long)grab);
            base = bcast_first_u64(base);
            if (base >= p.total_work) {
              ex = true;
              if (prof && lane == 0) { prof_lds[kLogExhausted] = wall_clock64(); prof_lds[kLogItersAtExhaustion] = prof_lds[kStIters]; }
            } else {
              wn = base;
              we = (base + grab < p.total_work) ? base + grab : p.total_work;
              const unsigned long long pl0 = base / (unsigned)p.spp;  // one 64-bit division per chunk, wave-uniform
              cpl = (unsigned)pl0;
              cs = (unsigned)(base - pl0 * (unsigned)p.spp);
              const unsigned long long rest = p.total_work - we;
              unsigned long long g = rest / ((unsigned long long)p.n_waves * 32ull);
              g = (g > p.chunk) ? p.chunk : g;
              nch = (g < 64) ? 64u : (unsigned)g;
            }
          }
          if (wn < we) {
            const unsigned avail = (unsigned)(we - wn);
            const unsigned n = avail < 64u ? avail : 64u;
            const unsigned t = cs + (unsigned)lane;
            const unsigned dp = udiv_by(t, p.inv_spp);
            unsigned pl = cpl + dp;
            if constexpr (kList) {  // list slot -> pixel (lanes past the batch read nothing: their slot may lie past the list)
              const unsigned lp = (unsigned)lane < n ? (unsigned)p.pixel_list[pl] : 0u;
              pl = lp < p.n_pixels ? lp : 0u;
            }
            const unsigned gs = t - dp * (unsigned)p.spp;
            const unsigned lrow = udiv_by(pl, p.inv_ncols);
            const unsigned gcol = pl - lrow * (unsigned)p.ncols;
            // local row -> image row (tiles of row_tile rows dealt round-robin to the shards)
            const unsigned tile = udiv_by(lrow, p.inv_row_tile);
            const unsigned within = lrow - tile * (unsigned)p.row_tile;
            const unsigned grow = (tile * (unsigned)p.shard_count + (unsigned)p.shard_index) * (unsigned)p.row_tile + within;
            Rng g;
            seed3(g, (uint64_t)grow, (uint64_t)gcol, (uint64_t)((unsigned)p.first_sample + gs));  // (progressive passes: the frame's sample index)
            // render.nim:64-66
            const double fs = ((double)(int)gcol + uniform01(g)) / w_div;
            const double ft = ((double)(int)grow + uniform01(g)) / h_div;
            const Camera cam = load_camera(p.cam_dev);
            const V3 rd = random_in_unit_disk(g) * cam.lens_radius;  // cameras.nim:48
            const double tm = uniform_range(g, cam.shutter_open, cam.shutter_close);  // cameras.nim:56
            if ((unsigned)lane < n) {
              res_rng[lane] = g.s0; res_rng[64 + lane] = g.s1; res_rng[128 + lane] = g.s2; res_rng[192 + lane] = g.s3;
              res_f[lane] = rd.x; res_f[64 + lane] = rd.y; res_f[128 + lane] = fs; res_f[192 + lane] = ft; res_f[256 + lane] = tm;
              res_dp[lane] = (unsigned char)dp;
            }
            if (lane == 0) res_pl0[0] = cpl;
            wn += n;
            const unsigned t2 = cs + n;
            const unsigned dp2 = rfl(udiv_by(t2, p.inv_spp));
            cpl += dp2;
            cs = t2 - dp2 * (unsigned)p.spp;
            // ... and serve the lanes that were still waiting (a short batch -- the end of a range -- may leave some for the next iteration)
            const unsigned left = want - take1;
            const unsigned take2 = left < n ? left : n;
            rh = 0;
            rc = n;
            pop(take1, take2);
            rh = take2;
            rc = n - take2;
          }
          w_next = wn; w_end = we; cur_pl = cpl; cur_s = cs; next_chunk = nch; exhausted = ex;
        }
        res_cnt = rc;
        res_head = rh;
      }
    } else {
    bool need_fetch = !active && !have_item;
    unsigned long long need_mask = ballot64(need_fetch);
    if (need_mask != 0) {
      if (w_next >= w_end && !exhausted) {
        const int leader = (int)__builtin_ctzll(need_mask);
        // SEED_PIXEL: tiles of p.chunk consecutive pixels (neighbouring pixels in one wave keep the
        // rays coherent).  SEED_SAMPLE: guided self-scheduling, the chunk shrinks with the work
        // that is left (waves of one SIMD get very unequal service -- slot 0 runs ~20x faster than
        // slot 4 -- so anything parked in a slow wave becomes the tail of the frame).
        // (whole pixels per grab where the chunk allows it: a pixel's samples then meet in ONE wave's LDS accumulator
        // and reach HBM in one flush instead of one per wave that touched the pixel -- 5.7x less write traffic at
        // 1000 spp; the tail of the guided schedule shrinks below a pixel and splits it again, which is fine)
        unsigned grab = kPixel ? p.chunk : next_chunk;
        if (!kPixel && grab >= (unsigned)p.spp) grab = TOR_UDIV(grab, p.spp, p.inv_spp) * (unsigned)p.spp;
        unsigned long long base = 0;
        if (kPixel) {
          // tiles in chain-length-descending order (tile_order_kernel): the longest chains start first, everybody ends on the cheapest
          // tiles.  (Rounds 2-4 cut the order into two regions and kept the waves of slow hardware slots out of the first; with the
          // screened object loop a bounce costs a slot-2 wave far less than the 177 us that was built against, the cut cost the brute
          // force 4-7 % and was off by default since round 4 -- profiles/r4_pixel_brute_knobs.txt; removed in round 5.)
          if (lane == leader) base = atomicAdd(p.work_counter, (unsigned long long)kTilePixels);
          base = bcast_first_u64(__shfl(base, leader));
        } else {
          if (lane == leader) base = atomicAdd(p.work_counter, (unsigned long long)grab);
          base = bcast_first_u64(__shfl(base, leader));
        }
        if (base >= p.total_work) {
          exhausted = true;
          if (kMigrate && p.mig != nullptr && exhausted && lane == 0) atomicMin(p.mig + kMigTCounterDry, (unsigned long long)wall_clock64());
          if (prof && lane == 0 && exhausted) { prof_lds[kLogExhausted] = wall_clock64(); prof_lds[kLogItersAtExhaustion] = prof_lds[kStIters]; }
        } else {
          w_next = base;
          w_end = (base + grab < p.total_work) ? base + grab : p.total_work;
          if (kPixel) {
            // work index space = tiles of kTilePixels pixels, optionally in cost order (LPT): the
            // k-th fetch renders tile order[k]
            unsigned tile = (unsigned)(base / kTilePixels);
            if (p.order != nullptr) tile = p.order[tile];
            cur_pl = tile * kTilePixels;
            cur_s = 0;
            const unsigned left_px = ((kList ? (unsigned)p.total_work : p.n_pixels)) - cur_pl;  // (kList: list slots, not pixels)
            w_end = base + ((left_px < (unsigned)kTilePixels) ? left_px : (unsigned)kTilePixels);
          } else {  // one 64-bit division per chunk, wave-uniform
            unsigned long long pl0 = base / (unsigned)p.spp;
            cur_pl = (unsigned)pl0;
            cur_s = (unsigned)(base - pl0 * (unsigned)p.spp);
            const unsigned long long left = p.total_work - w_end;
            unsigned long long g = left / ((unsigned long long)p.n_waves * 32ull);
            g = (g > p.chunk) ? p.chunk : g;
            next_chunk = (g < 64) ? 64u : (unsigned)g;
          }
        }
      }
      if (w_next < w_end) {
        const unsigned prefix = lane_prefix(need_mask);
        const unsigned avail = (unsigned)(w_end - w_next);
        const unsigned want = (unsigned)__builtin_popcountll(need_mask);
        const unsigned take = (want < avail) ? want : avail;
        const bool got = need_fetch && prefix < take;
        if (got) {
          unsigned pl;
          if (kPixel) {
            pl = cur_pl + prefix;
            s = 0;
            if (kAccInLds) { pix_acc[0] = 0.0; pix_acc[64] = 0.0; pix_acc[128] = 0.0; }
            else acc = v3(0, 0, 0);
            if (kResMom) { pix_mom[0] = 0.0; pix_mom[64] = 0.0; pix_mom[128] = 0.0; }
          } else {  // sample and probe
            const unsigned t = cur_s + prefix;
            const unsigned dp = TOR_UDIV(t, p.spp, p.inv_spp);
            pl = cur_pl + dp;
            s = (int)(t - dp * (unsigned)p.spp);
          }
          bool off_shard = false;  // kList: a list entry outside the shard
          if constexpr (kList) {
            const unsigned lp = (unsigned)p.pixel_list[pl];
            off_shard = lp >= p.n_pixels;
            pl = off_shard ? 0u : lp;
          }
          // (round 5: the per-lane divisions by ncols, spp and row_tile are multiplications by their float64 reciprocals --
          // tor_device.hpp udiv_by, exact for every 32-bit dividend; a 32-bit division by a run-time divisor is ~22 vector
          // instructions and this section runs on nearly every bounce iteration)
          const unsigned lrow = TOR_UDIV(pl, p.ncols, p.inv_ncols);
          col = (int)(pl - lrow * (unsigned)p.ncols);
          // local row -> image row (tiles of row_tile rows dealt round-robin to the shards)
          const unsigned tile = TOR_UDIV(lrow, p.row_tile, p.inv_row_tile);
          const unsigned within = lrow - tile * (unsigned)p.row_tile;
          row = (int)((tile * (unsigned)p.shard_count + (unsigned)p.shard_index) * (unsigned)p.row_tile + within);
          pix = (int)pl;
          if constexpr (kList) {
            if (off_shard) pix = -1;  // deposits nothing (tag -1: never flushed)
          }
          // (kList on the pixel streams: an entry outside the shard is dropped here -- nothing read, nothing drawn, nothing written.  The
          // lane took the slot but holds no item: it stays idle through this bounce iteration and asks again at the next refill; the
          // sums it zeroed above and the row / column of pixel 0 it computed are never used, and pix = -1 is never read)
          have_item = !(kPixel && off_shard);
          if (kPixel && !off_shard) {
            if (kResume && p.first_sample > 0) {
              // a continued pixel: the state its stream had after first_sample samples and the raw sums so far, once per pixel and pass
              const unsigned long long* st = p.rstate + (size_t)pl * 4;
              rng.s0 = st[0]; rng.s1 = st[1]; rng.s2 = st[2]; rng.s3 = st[3];
              const double* so = p.out + (size_t)pl * 3;
              if (kAccInLds) { pix_acc[0] = so[0]; pix_acc[64] = so[1]; pix_acc[128] = so[2]; }
              else acc = v3(so[0], so[1], so[2]);
              if (kResMom) { const double* mo = p.mom + (size_t)pl * 3; pix_mom[0] = mo[0]; pix_mom[64] = mo[1]; pix_mom[128] = mo[2]; }
            } else {
              seed2(rng, (uint64_t)(int64_t)row, (uint64_t)(int64_t)col);  // render.nim:59-60
            }
            if (kPrio) pix_iters = 0;
          }
        }
        w_next += take;
        if (kPixel) {
          cur_pl += take;
        } else {
          const unsigned t = cur_s + take;
          const unsigned dp = TOR_UDIV(t, p.spp, p.inv_spp);
          cur_pl += dp;
          cur_s = t - dp * (unsigned)p.spp;
        }
      }
    }
    if (!active && have_item) {
      if (!kPixel) seed3(rng, (uint64_t)row, (uint64_t)col, (uint64_t)((unsigned)p.first_sample + (unsigned)s));  // (progressive passes: the frame's sample index)
      have_item = false;  // the pending sample is consumed by starting its path
      // render.nim:64-66
      const double u = ((double)col + uniform01(rng)) / w_div;
      const double v = ((double)row + uniform01(rng)) / h_div;
      const Camera cam = load_camera(p.cam_dev);
      const Ray r = camera_ray(cam, u, v, rng);
      o = r.origin;
      d = r.direction;
      time = r.time;
      set_att(v3(1.0, 1.0, 1.0));  // render.nim:22
      depth = 0;
      active = true;
    }
    }  // !kRes
#undef TOR_UDIV

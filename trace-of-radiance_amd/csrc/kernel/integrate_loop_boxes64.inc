// integrate_loop_boxes64.inc -- object loop of integrate_kernel, TOR_ACCEL_BLOCKS without the float32 filter: float64 slab test of the
// block boxes (kind 3) / super boxes (kind 4).
            // TOR_ACCEL_BLOCKS: the records are inflated axis-aligned boxes around spatial blocks of 8
            // objects (kind 3, entries flagged with bit 31) or around 8 such blocks (kind 4, bit 30).
            // Slab test; a set bit means 'this lane has to look inside'.  1/d may be +-inf (d = 0): (lo - o) * inf is +-inf, or
            // NaN when lo == o, and v_min/v_max_f64 drop a NaN operand -- the axis then imposes no
            // constraint, which is the conservative answer.
            const double ix = 1.0 / dx, iy = 1.0 / dy, iz = 1.0 / dz;
            cdptr rec = as_const(p.bnd) + 8 * (long)(seg_begin + i);
            for (; i < seg_count; i += kBlock) {
              unsigned m = kWords ? mw : 0u;
#pragma unroll
              for (int j = 0; j < kBlock; ++j) {
                const double tx0 = (rec[8 * j + 0] - ox) * ix, tx1 = (rec[8 * j + 3] - ox) * ix;
                const double ty0 = (rec[8 * j + 1] - oy) * iy, ty1 = (rec[8 * j + 4] - oy) * iy;
                const double tz0 = (rec[8 * j + 2] - oz) * iz, tz1 = (rec[8 * j + 5] - oz) * iz;
                const double t_in = __builtin_fmax(__builtin_fmax(__builtin_fmin(tx0, tx1), __builtin_fmin(ty0, ty1)),
                                                   __builtin_fmax(__builtin_fmin(tz0, tz1), 0.0));
                const double t_out = __builtin_fmin(__builtin_fmin(__builtin_fmax(tx0, tx1), __builtin_fmax(ty0, ty1)),
                                                    __builtin_fmax(tz0, tz1));
                m = (m << 1) | ((t_in <= t_out) ? 1u : 0u);
              }
              rec += 8 * kBlock;
              // a ray beyond the boxes' reach enters every box -- every REAL box: the padding entries of the super-box segment have
              // no block boxes or records behind them (as integrate_loop_boxes32.inc does for a `wild` ray)
              unsigned far = box_far;
              if (seg_kind == 4) {
                const int n_valid = p.n_super - i;  // bit (7 - j) <-> record i + j
                far &= (n_valid >= kBlock) ? 0xffu : ((n_valid <= 0) ? 0u : ((0xff00u >> n_valid) & 0xffu));
              }
              m |= far;
              q[qn * 64] = ((seg_kind == 3) ? 0x80000000u : 0x40000000u) | ((unsigned)(seg_block0 + i / kBlock) << 8) | m;
              qn += (m != 0) ? 1u : 0u;
              if (ballot64(qn >= (unsigned)kQCap) != 0) { full = true; i += kBlock; break; }
            }

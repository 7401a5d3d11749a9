// integrate_deposit.inc -- SEED_SAMPLE: finished samples are rounded to 2^-36 (exact float64 sums in any order) and deposited in the
// wave's LDS pixel cache; HBM sees one flush per pixel and wave (float64 atomics).  SEEDING 3 also deposits the second moments
// quantize36(q * q) of the same quantised values into a parallel cache (mom_lds) with the same slots, tags and flushes.
      // ---- deposit finished samples: exact (2^-36-quantised) float64 sums, any order ------
      // The wave keeps the pixels it is currently filling in a small LDS cache (pixels arrive
      // in increasing order, so a slot is evicted when the pixel is complete bar stragglers);
      // HBM only sees one flush per pixel and wave instead of one atomic per sample.
      unsigned long long ended_mask = ballot64(ended);
      const double qx = quantize36(radiance.x), qy = quantize36(radiance.y), qz = quantize36(radiance.z);
      while (ended_mask != 0) {
        const int src = (int)__builtin_ctzll(ended_mask);
        const int pp = __builtin_amdgcn_readlane(pix, src);
        const bool mine = ended && pix == pp;
        // (hashed: a wave's successive pixels are a multiple of the wave count apart -- 3072 on MI355X -- and would
        // all land in slot pp & 15, so every late sample of the previous pixel evicted the current one)
        const int slot = (pp ^ (pp >> 4) ^ (pp >> 9) ^ (pp >> 14)) & (kAccSlots - 1);
        const int tag = __builtin_amdgcn_readfirstlane(tag_lds[slot]);
        if (tag != pp) {
          if (lane < 3) {
            if (tag >= 0) unsafeAtomicAdd(p.out + (size_t)tag * 3 + lane, acc_lds[slot * 3 + lane]);
            acc_lds[slot * 3 + lane] = 0.0;
            if (kMom) {
              if (tag >= 0) unsafeAtomicAdd(p.mom + (size_t)tag * 3 + lane, mom_lds[slot * 3 + lane]);
              mom_lds[slot * 3 + lane] = 0.0;
            }
          }
          if (lane == 0) tag_lds[slot] = pp;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        }
        if (mine) {
          unsafeAtomicAdd(&acc_lds[slot * 3 + 0], qx);
          unsafeAtomicAdd(&acc_lds[slot * 3 + 1], qy);
          unsafeAtomicAdd(&acc_lds[slot * 3 + 2], qz);
          if (kMom) {  // q <= 1 (DESIGN 2): q * q <= 1, rounded to 2^-36 like q itself -- exact sums under the same bound
#if defined(TOR_ACCUM_MUTATE) && TOR_ACCUM_MUTATE == 1  // (mutation check of the oracle tests: the square of the unquantised radiance)
            unsafeAtomicAdd(&mom_lds[slot * 3 + 0], quantize36(radiance.x * radiance.x));
            unsafeAtomicAdd(&mom_lds[slot * 3 + 1], quantize36(radiance.y * radiance.y));
            unsafeAtomicAdd(&mom_lds[slot * 3 + 2], quantize36(radiance.z * radiance.z));
#else
            unsafeAtomicAdd(&mom_lds[slot * 3 + 0], quantize36(qx * qx));
            unsafeAtomicAdd(&mom_lds[slot * 3 + 1], quantize36(qy * qy));
            unsafeAtomicAdd(&mom_lds[slot * 3 + 2], quantize36(qz * qz));
#endif
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        ended_mask &= ~ballot64(mine);
      }

// tor_scene.hpp -- host-side flattening of the reference's AoS object list
// (hittables_lists.nim:15-46, HittableVariant hittables_variants.nim:50-57) into the device layouts
// described in tor_kernels.hpp, and the optional block-bounds acceleration layout.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/tor_render.h"

namespace tor {

// Brute-force layout of a subset of the objects (tor_kernels.hpp: stat / movy / mov / segs / cold).
struct HostLayout {
  std::vector<double> stat, mov, movy, segs, cold;
  // second form of the strict loop's FMA screen (tor_screen.hpp): per segment {xkind (0: none, 10 static, 11 static with a
  // common c0.y, 12 mover along y with a common c0.y), first float64 of its records in xrec, the common c0.y, 0...}; records
  // {cx, cy, cz, K} | {cx, cz, K', 0} | {cx, cz, K', dcy}: 4 float64 each, padded like the first form's
  std::vector<double> xsegs, xrec;
  // what the kernel reads of segs / xsegs, one 128-byte record per segment (16 float64 slots): int32 {xkind, kind, padded count |
  // padding << 24, first block, first hot record, first float64 in xrec, first float64 in xpl, the plane screen's gate (0 never, 1 always, 2 the wave votes; + 4: the reach pass runs in front of the whole words)}, then float64 {time0, time1 -
  // time0, reach, travel, common c0.y, largest radius^2, extent x, extent z} and the segment's first plane record (4 slots);
  // for xkinds 10 / 11 / 12 / 14 those 4 slots are {the first float32 record {cx', cz'}, Ox, Oz, {E, Cm} as float32 rounded up}
  std::vector<double> xhdr;
  // stage one in front of it (tor_screen.hpp: the plane screen, kinds 11 / 12 only): {cx, cz} per slot -- 16 bytes, the wave-uniform
  // loop reads nothing else -- at xpl[xsegs[3] + 2 * slot of the segment]; xsegs[4] = the largest radius^2 of the segment
  std::vector<double> xpl;
  // stage one in float32 (tor_screen.hpp plane_seg32, xkinds 10 / 11 / 12 / 14): {cx - Ox, cz - Oz} per slot at the SAME indices
  // as xpl (xkind 13's stretches unused), padding {kPlane32PadX, kPlane32PadZ}; per segment {Ox, Oz, E, Cm} in xpl32seg (0 for
  // segments without the float32 table).  The header (xhdr) of such a segment carries them in place of the float64 first record.
  std::vector<float> xpl32;
  std::vector<double> xpl32seg;
  // the reach pass in front of stage one's whole words (tor_screen.hpp reach_ray): kReachRecFloats floats per 32-slot WORD of the
  // sorted list, word w = slots [32 w, 32 w + 32) -- {xlo, xhi, zlo, zhi} float32 offsets from the segment's origin, {ylo, yhi}
  // float64 -- for the words wholly inside a segment of xkind 10 / 11 / 12 / 14; every other word (-inf, +inf): reached by everybody.
  // The segments of those xkinds that the reach pass runs on (tor_scene.cpp: enough objects, a thin height slab) are ordered by an
  // even split of their centres' ground positions, so that a word is a patch of ground.  xwb_all: the same table with every word (-inf, +inf) (TOR_PLANE=3: the reach pass runs and culls nothing)
  std::vector<float> xwb, xwb_all;
  std::vector<float> hot32;  // TOR_ACCEL_F32 segments (kinds 5/6/7): packed pair records, see tor_kernels.hpp
  int n_segs = 0;
  size_t n_sorted = 0;  // cold slots (padded)
  // coop_pixel_kernel walks the cold slots 64 at a time ("trips"); 4 float64 per trip {kind, time0, time1 - time0, 0}:
  // kind 0 = no slot of the trip moves, 1 = all move along y only and share (time0, time1), 2 = all move and share
  // (time0, time1), 3 = mixed (per-object handling)
  std::vector<double> coop_trips;
};

// TOR_ACCEL_F32: objects that qualify (tor_filter32.hpp: f32_eligible, and not farther than far_limit from
// the origin) are laid out for the float32 pre-filter, relative to `origin`; the others keep the float64 loop.
struct F32Options {
  double origin[3] = {0.0, 0.0, 0.0};
  double far_limit = 0.0;
};
// Origin = per-axis median of the (start) centres, far_limit = 8 x the median distance from it: robust
// against a few huge or far-away objects (the ground sphere of random_scene sits 1000 units below).
F32Options f32_options_for(const TorHittableVariant* objs, int64_t n);

// Builds the layout for objects `ids` (original indices, kept in this order inside each segment, except in the plane-screened
// segments that are ordered by ground position: see xwb).
// Returns false and sets err for unknown kinds.
bool build_layout(const TorHittableVariant* objs, const std::vector<int64_t>& ids, HostLayout& out, std::string& err,
                  const F32Options* f32 = nullptr);

// Acceleration layout (TOR_ACCEL_BLOCKS): large or irregular objects stay in an "always" brute-force
// layout; the rest are ordered by a top-down surface-area build (tor_scene.cpp build_accel) and cut into blocks of 8 consecutive objects.
// Per render call the blocks get conservative bounding spheres (they depend on the ray-time range).
struct HostAccel {
  bool available = false;
  HostLayout always;            // + one segment of kind 3 (the bounds) appended to always.segs
  std::vector<double> cold;     // always.cold followed by the spatial objects' cold records
  std::vector<double> hot;      // hot_stride float64 per spatial slot: {c0 xyz, r^2, dc xyz, time-group id or -1},
                                // or {c0 xyz, r^2} when none of the spatial objects moves
  int hot_stride = 8;
  std::vector<double> groups;   // {time0, time1 - time0} per time group of the spatial objects
  size_t spatial_base = 0;      // first cold slot of the spatial objects (multiple of 8)
  size_t n_blocks = 0;
  // Box fan-out (round 4 experiment, default 1 = off): a culling box of the wave-uniform loop covers `fanout` consecutive blocks
  // (16 / 32 objects for fanout 2 / 4).  Every lane tests every box (14 float32 instructions each), the pooled resolve filters only
  // the boxes a ray enters (8.5 instructions per object), so fewer, larger boxes looked cheaper on paper; measured, they are not
  // (tor_scene.cpp build_accel).  Blocks stay 8 objects (records, cold slots, masks); box b stands for blocks [b * fanout, (b + 1) * fanout).
  int fanout = 1;
  size_t n_boxes = 0;           // = ceil(n_blocks / fanout)
  bool two_level = false;       // the uniform loop tests boxes around 8 boxes; lanes descend to those
  struct Obj { double c0[3], dc[3], t0, dt, abs_r; bool moving, valid; };
  std::vector<Obj> spatial;     // n_blocks * 8 entries (padding: valid = false)
  // TOR_ACCEL_F32 block expansion: float32 pair records of the spatial slots (tor_filter32.hpp), 4 pairs per
  // block, hot32_stride floats per pair: 10 {cx cx' cy cy' cz cz' r2 r2' k k'} (no mover), 12 (+ dcy dcy':
  // movers along y only), 16 (+ dcx.. dcy.. dcz..).  Built when every spatial object qualifies for the
  // filter and the movers share one (time0, time1); otherwise the lanes expand the float64 records.
  bool sp32 = false;
  std::vector<float> hot32;
  int hot32_stride = 10;
  int hot32_block_stride = 40;  // floats from one block's records to the next (4 pairs + padding against LDS bank conflicts)
  double sp_t0 = 0.0, sp_dt = 1.0;      // the movers' time group
  float sp_mc0max = 0.0f, sp_dcmax = 0.0f;  // max |c0 - origin| and |dc| over the spatial objects (rounded up)
};

void build_accel(const TorHittableVariant* objs, int64_t n, HostAccel& out, const F32Options* f32 = nullptr);

// 8 float64 per block {lo xyz, hi xyz, 0, 0}: a conservative (inflated) axis-aligned box around the
// block's spheres over the ray-time range; padded to a multiple of 8 blocks with never-entered (NaN)
// boxes; then one slack record and the super boxes (one per 8 block boxes, again padded to 8).
// Returns false when the time range is not finite (caller falls back to brute force).
bool compute_block_bounds(const HostAccel& acc, double t_lo, double t_hi, std::vector<double>& bnd);
inline size_t accel_boxes_padded(const HostAccel& acc) { return (acc.n_boxes + 7) / 8 * 8; }  // records of the kind-3 segment

// Where the boxes of `bnd` (compute_block_bounds for acc) hold for the reference's rounding: a hit the reference accepts on a spatial
// object of radius r from an origin at distance |oc| lies at most 6 eps (|oc|^2 + r^2) / r outside the sphere, and every box is
// inflated by at least 1e-6.  With 16 eps (|oc|^2 + r_max^2) / r_min <= 1e-6 / 4, over 10x margin, the hit lies inside its box.
// |oc| <= |o - org| + half the diagonal of the boxes' union, so origins within sqrt(*reach2) of org qualify; *a_min keeps the test's
// products clear of the subnormal range (an underflowed product's error is absolute, not relative): a * r_min^2 >= 2^-1000.
// *reach2 = -1 and *a_min = +inf when no origin qualifies (no box, a radius of 0, radii too small for the margin).  A ray outside
// either bound must not be culled by the float64 boxes: the ray queries walk it (tor_query.hpp), the integrator's float64 block
// loop lets it enter every box (integrate_loop_boxes64.inc).
void block_reach(const HostAccel& acc, const std::vector<double>& bnd, double org[3], double* reach2, double* a_min);

// The same boxes for the float32 slab test (TOR_ACCEL_BLOCKS | TOR_ACCEL_F32): one record of 8 float32 per box,
// same record indices as `bnd`, {c.x, h.x, c.y, h.y, c.z, h.z, 0, 0} relative to `origin` -- centre and half-extent, the
// half-extent rounded up so that the float32 box contains the float64 one (NaN records stay NaN).  Returns max |coordinate| over the
// valid boxes, rounded up; *hmin_out = the smallest half-extent (tor_filter32.hpp: the ray-side inflation is relative to it).
float block_bounds_f32(const std::vector<double>& bnd, const double origin[3], std::vector<float>& bnd32, float* hmin_out);

}  // namespace tor

/*
 * tor_reach.h -- debug entries of the REACH PASS of libtor_mi355x.so, included by tor_render.h (which defines the types).
 *
 * The strict brute-force layout orders the objects of a plane-screened segment of xkind 10 / 11 / 12 / 14 by an even top-down split
 * of their ground positions, cut at the sorted list's word boundaries (TOR_REACH_ORDER=morton: by the Morton code, the order it
 * replaced), and keeps one box per 32-slot word of the sorted list; in front of stage one's whole words every ray
 * asks which of those words it can be near at all (csrc/tor_screen.hpp reach_ray / reach_miss).  A word nobody of the wave reaches
 * is not walked; a ray's bits in a walked word it does not reach are cleared.  What must hold: the segment's own second-stage
 * test drops every slot of a word the ray does not reach (tor_debug_screen2_scene's code is never 2 there).
 *
 * tor_debug_reach_scene: the reach pass over a whole scene on the HOST, from the layout and the table tor_scene_upload builds and
 * the functions the kernel runs.
 *   reach[ray * world.len + object]  1: the ray reaches the word of the object's slot, or that word carries no box (a word shared
 *                                    between segments, a word of the block phases, xkind 13, a segment with a non-finite input);
 *                                    0: the word carries a box and the ray does not reach it.
 *   word_out[object] (nullable)      the object's word of the sorted list (slot / 32) when that word carries a box, else -1.
 *   slot_out[object] (nullable)      the object's slot in the sorted list.
 *   boxes_out (nullable)             for the first max_words words of the sorted list, 6 float64 each: {xlo, xhi, zlo, zhi} of the
 *                                    word's record moved back by the segment's origin (absolute coordinates, rounded to nearest),
 *                                    {ylo, yhi}; a word without a box: -inf, +inf throughout; a boxed word of padding alone: the
 *                                    empty box +inf, -inf.  *n_words_out (nullable) = the words of the sorted list.
 *
 * tor_debug_last_reach: of the last strict brute-force launch on a context with statistics enabled (tor_context_set_stats),
 * out[0] = whole words stage one walked, out[1] = whole words it met (walked + skipped), summed over waves, segments and passes.
 * Counted by the kernel builds that carry the pass: a launch whose layout has no segment that asks for it (fewer than 8 boxed
 * words, or a height slab that is not thin against the ground box) reports 0, 0; TOR_PLANE=2 runs the pass on every segment.
 */
#ifndef TOR_REACH_H
#define TOR_REACH_H

#ifdef __cplusplus
extern "C" {
#endif

TOR_API int tor_debug_reach_scene(TorHittableList world, int64_t n_rays, const double* o, const double* d, const double* time,
                                  int8_t* reach, int32_t* word_out, int32_t* slot_out, double* boxes_out, int64_t max_words,
                                  int64_t* n_words_out);
TOR_API int tor_debug_last_reach(TorContext* ctx, uint64_t out[2]);

#ifdef __cplusplus
}
#endif

#endif /* TOR_REACH_H */

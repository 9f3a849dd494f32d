// analysis_launch.h -- the evidence build's hook in analysis.hip: the many-pair / one-query hdist with four contiguous words per lane
// for every pair (hdist_words_impl 0) instead of coalesced 256-word tiles.  Included once, by analysis.hip inside an anonymous
// namespace, under -DBITNUC_SWEEP_VARIANTS.
#pragma once

namespace evidence {
bool wants_hdist_words(const bitnuc_ctx *c) { return knobs(c).hdist_words_impl != 1; }
} // namespace evidence

// kernels_search.h — the choice of UClust::Search on the device (uclust.cpp:44-54), for many queries at once.
//
// The reference walks a query's word-count hits in order, aligns each (AlignPairFlat) and stops at the first whose EA reaches the threshold:
//     if (EA >= m_MinEA) { keep this path; break; }
// mpcgpu_search_pairs (mpcgpu_search.inc) has the EA of every candidate after the finishing kernel, before any dense posterior exists.
// search_pick_kernel makes the reference's choice from those floats: a wavefront per SLOT (a group's candidates inside the chunk at hand:
// pairs [first, first + count) of the chunk, in the order they are to be tried), lane t tests candidate base + t with the reference's own
// comparison (a NaN never qualifies), a ballot finds the lowest qualifying lane, and groups of more than 64 candidates go on in strides of
// 64 until one stride has a hit. A candidate whose list overflowed (flag bit 0: its EA is not valid, the host redoes the chunk) never
// qualifies. pick[s] = the pair of the chunk, acc[s] = its position among the slot's candidates, both MPC_PICK_NONE when none qualifies or
// the slot has count 0 (an empty group, or one that found its hit in an earlier chunk). The indirect kernels of kernels_aln.h read pick[].
#pragma once
#include "kernels_aln.h"

#define MPC_SEARCH_WAVES 4 // slots per workgroup

struct SearchPickParams {
	const u32 *first, *count; // per slot
	const float *ea;          // per pair of the chunk: what the finishing kernel wrote
	const u32 *flags;         // per pair: bit 0 = candidate overflow
	float min_ea;
	u32 nslots;
	u32 *pick, *acc;          // per slot, out
};

__global__ void __launch_bounds__(64 * MPC_SEARCH_WAVES) search_pick_kernel(SearchPickParams p)
{
	const u32 lane = threadIdx.x & 63u;
	const u32 s = blockIdx.x * MPC_SEARCH_WAVES + (threadIdx.x >> 6); // wave-uniform
	if (s >= p.nslots) return;
	const u32 first = p.first[s], count = p.count[s];
	u32 found = MPC_PICK_NONE;
	for (u32 base = 0; base < count; base += 64) {
		const u32 t = base + lane;
		bool ok = false;
		if (t < count) ok = !(p.flags[first + t] & 1u) && p.ea[first + t] >= p.min_ea; // uclust.cpp:47
		const u64 m = __ballot(ok);
		if (m) { found = base + (u32)__popcll((m - 1ull) & ~m); break; } // the lowest set lane
	}
	if (lane == 0) {
		p.pick[s] = found == MPC_PICK_NONE ? MPC_PICK_NONE : first + found;
		p.acc[s] = found;
	}
}

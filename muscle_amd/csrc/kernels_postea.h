// kernels_postea.h — finish one pair's posterior for its EA score alone (mpcgpu_ea_scores, mpcgpu_ea.inc).
//
// Replaces, per pair, what CalcEADistMx keeps of AlignPairFlat (eadistmx.cpp:54, alignpairflat.cpp:11-19): the expf half of CalcPostFlat
// (calcposteriorflat.cpp:16-22) over the candidate list the sweeps left, the score of CalcAlnFlat over the dense thresholded posterior
// (calcalnflat.cpp:6-46 — the same recurrence as CalcAlnScoreFlat, calcalnscoreflat.cpp:4-32) and EA = Score / min(LX, LY). The trace-back
// and the sparse matrix, which that caller throws away, are not computed: no packed record, no row or column counts, no transposed ranks.
//
// The code is post_rows_kernel's first half, the same function (mpc_post_rows_pair<.., FULL = false>, kernels_post.h): the same mpc_score_to_prob on the same
// operand with the same use_fma, the same threshold (the list holds the cells with Score >= MIN_SPARSE_SCORE), the same recurrence in the
// same order — the bits of mpcgpu_calc_posteriors + mpcgpu_get_ea. One 64-thread workgroup (one wavefront) per pair, a persistent grid.
//
// Output: ONE float per pair, ea[pid]. A list that overflowed its room (cand_cnt > capc) is reported in that float as MPC_EA_OVERFLOW, a
// negative value no EA takes (a score is a sum of probabilities along a path, >= 0): the host redoes the batch with a larger room.
// Working storage: the list itself (the score word of an entry becomes its probability, as in post_rows_kernel) and the row-sorted copy in
// LDS or, for a list of more than sort_cap entries, in the workgroup's slot of sort_scratch.
// Limit: the three per-position LDS arrays and the list must fit the CU's LDS, the test post_rows_kernel's host side makes
// (post_rows_fits: roughly LXmax + 2 * LYmax <= 36 000). The pairs beyond it have a workgroup-per-pair form, post_wide_ea_kernel
// (kernels_postwea.h): under MPCGPU_EA_WIDE=1 mpcgpu_ea_scores sends them there, without it the call refuses such a list by name.
#pragma once
#include "kernels_post.h"

#define MPC_EA_OVERFLOW (-1.0f)

struct PostEaParams {
	const u32 *pair_x, *pair_y; // per batch-local pair
	const u32 *seq_len;
	u64 *cand;          // as PostRowsParams::cand
	u32 capc;
	const u32 *cand_cnt;
	int use_fma;
	u32 lx_cap, ly_cap; // LDS array sizes (entries): rows+1, cols+1
	u32 sort_cap;       // LDS entries for the row-sorted list; larger lists use sort_scratch
	u32 batch;          // cells of one row handled per EA pass (64)
	u64 *sort_scratch;
	u64 sort_stride;
	float *ea;          // per batch-local pair: the only output
	u32 count;
	u32 long_min;       // as in PostParams
};

__global__ void __launch_bounds__(64) post_ea_kernel(PostEaParams p)
{
	MPC_DYN_SMEM(smem_raw);
	u32 *s_rend = (u32 *)smem_raw;              // the layout of post_rows_kernel
	u32 *s_cend = s_rend + p.lx_cap;
	float *s_pm = (float *)(s_cend + p.ly_cap);
	u64 *s_sorted = (u64 *)(smem_raw + ((((size_t)p.lx_cap + 2 * (size_t)p.ly_cap) * 4 + 7) & ~(size_t)7));
	const int t = threadIdx.x;

	for (u32 pid = blockIdx.x; pid < p.count; pid += gridDim.x) {
		const u32 LX = p.seq_len[p.pair_x[pid]], LY = p.seq_len[p.pair_y[pid]];
		const u32 c = p.cand_cnt[pid];
		if (c > p.capc) {
			if (t == 0) p.ea[pid] = MPC_EA_OVERFLOW;
			continue;
		}
		u64 *sorted = (c <= p.sort_cap) ? s_sorted : (p.sort_scratch + (u64)blockIdx.x * p.sort_stride);
		mpc_post_rows_pair<true, false>(t, LX, LY, mpc_key_shift(LX, p.long_min), p.cand + (u64)pid * p.capc, c, p.capc, sorted, nullptr, nullptr,
			p.ea + pid, nullptr, p.use_fma, p.batch, s_rend, s_cend, s_pm);
		__syncthreads(); // the next pair clears the arrays the lanes may still be reading
	}
}

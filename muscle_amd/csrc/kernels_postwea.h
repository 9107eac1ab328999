// kernels_postwea.h — post_wide_ea_kernel: post_ea_kernel's job (kernels_postea.h: probabilities and the EA score of a pair, one float
// out) with a whole WORKGROUP per pair, for the lists post_ea_kernel does not take (a sequence beyond ~12 100 positions: the three
// per-position arrays of the row-list code no longer fit a CU's LDS). mpcgpu_ea_scores sends the WIDE pairs of a list here
// (mpcgpu_ea.inc: MPCGPU_EA_WIDE, MPCGPU_EA_WIDE_MIN).
//
// The code is post_wide_kernel's first half (kernels_postw.h), statement by statement, on the same helpers (mpc_postw_sort,
// mpc_score_to_prob, mpc_wave_scan_max_nonneg) and in the same LDS layout (mpc_postw_smem): the same mpc_score_to_prob on the same
// operand with the same use_fma, the stable radix sort of (flat index << 32 | P bits) — key shift + bits(LX - 1) significant bits —
// the table of row starts in global scratch, the EA recurrence of calcalnscoreflat.cpp:4-32 with a lane owning consecutive columns
// and the prefix maximum crossing the workgroup. max is exact and the one add per stored cell is the reference's, so the float is,
// bit for bit, the EA of post_wide_kernel, of post_ea_kernel and of mpcgpu_calc_posteriors + mpcgpu_get_ea. What post_wide_kernel
// does beyond that is not done: no record (no row or column counts to clear), no FromPost rank, no column-major sort.
// It is written beside post_wide_kernel and not as a common function of both: that kernel's compiled code stays what it was.
//
// Output: ONE float per pair, ea[pid]; a list that overflowed its room (cand_cnt > capc) writes MPC_EA_OVERFLOW there, as
// post_ea_kernel does. The raw candidate list is only read.
#pragma once
#include "kernels_postw.h"
#include "kernels_postea.h"

struct PostWideEaParams { // PostWideParams without the record, nnz and flags
	const u32 *pair_x, *pair_y; // per batch-local pair
	const u32 *seq_len;
	const u64 *cand;
	u32 capc;
	const u32 *cand_cnt;
	int use_fma;
	u32 lds_cap;         // entries of each of the two LDS key buffers; longer lists ping-pong in key_scratch
	u32 srow_cap;        // floats of each of the two LDS DP rows; wider pairs use srow_scratch
	u64 *key_scratch;    // per workgroup: 2 * key_stride u64
	u64 key_stride;
	u32 *rs_scratch;     // per workgroup: rs_stride u32 (row starts, LXmax + 1)
	u64 rs_stride;
	float *srow_scratch; // per workgroup: srow_stride floats (2 * (LYmax + 1))
	u64 srow_stride;
	u64 *info;           // per workgroup: (candidates << 8 | radix passes) of its pair with the most candidates
	float *ea;           // per batch-local pair: the only output
	u32 count;
	u32 long_min;
};

__global__ void __launch_bounds__(MPC_POSTW_THREADS) post_wide_ea_kernel(PostWideEaParams p)
{
	MPC_DYN_SMEM(smem_raw);
	const u32 t = threadIdx.x, T = blockDim.x, lane = t & 63u, w = t >> 6, NW = T >> 6;
	PostwLds s; // the layout of post_wide_kernel
	s.off = (u32 *)smem_raw;
	s.wcnt = s.off + 256;
	s.wbase = s.wcnt + NW * 256u;
	u32 *s_rs = s.wbase + NW * 256u; // T + 1 row starts
	s.wv = s_rs + T + 1;             // 2 x MPC_POSTW_WAVES_MAX words
	float *s_row = (float *)(s.wv + 2 * MPC_POSTW_WAVES_MAX + 1);
	u64 *s_keys = (u64 *)(smem_raw + (((mpc_postw_fixed_words(T) + 2 * (size_t)p.srow_cap) * 4 + 7) & ~(size_t)7));
	u64 best = 0; // thread 0: (candidates << 8 | passes) of this workgroup's largest list

	for (u32 pid = blockIdx.x; pid < p.count; pid += gridDim.x) {
		const u32 LX = p.seq_len[p.pair_x[pid]], LY = p.seq_len[p.pair_y[pid]];
		const u32 kshift = mpc_key_shift(LX, p.long_min);
		const u32 c = p.cand_cnt[pid];
		if (c > p.capc) { // overflow: the host redoes the batch with a larger room
			if (t == 0) p.ea[pid] = MPC_EA_OVERFLOW;
			continue;
		}
		const bool in_lds = c <= p.lds_cap;
		u64 *A = in_lds ? s_keys : p.key_scratch + (u64)blockIdx.x * 2 * p.key_stride;
		u64 *B = in_lds ? s_keys + p.lds_cap : A + p.key_stride;
		float *S = (LY + 1 <= p.srow_cap) ? s_row : p.srow_scratch + (u64)blockIdx.x * p.srow_stride; // 2 * (LY + 1) floats
		u32 *rs = p.rs_scratch + (u64)blockIdx.x * p.rs_stride;
		const u64 *cand = p.cand + (u64)pid * p.capc;
		const u32 passes = (kshift + mpc_bits_of(LX - 1u) + 7u) / 8u;
		if (t == 0) { const u64 mine = ((u64)c << 8) | passes; best = mine > best ? mine : best; }

		// ---- probabilities (calcposteriorflat.cpp:16-22); key = (flat index << 32) | P bits
		for (u32 q = t; q < c; q += T) {
			const u64 v = cand[q];
			const float pr = mpc_score_to_prob(__uint_as_float((u32)v), p.use_fma);
			A[q] = (v & 0xffffffff00000000ull) | (u64)__float_as_uint(pr);
		}
		__syncthreads();
		const u64 *buf = mpc_postw_sort(A, B, c, passes, s); // row-major: rows ascending, columns ascending

		// ---- row starts: rs[i] = first sorted candidate of row i or of a later row, rs[LX] = c
		if (c == 0)
			for (u32 i = t; i <= LX; i += T) rs[i] = 0;
		for (u32 q = t; q < c; q += T) {
			const u32 r = (u32)(buf[q] >> 32) >> kshift;
			const u32 r0 = q ? ((u32)(buf[q - 1] >> 32) >> kshift) + 1u : 0u;
			for (u32 i = r0; i <= r; ++i) rs[i] = q;
			if (q == c - 1u)
				for (u32 i = r + 1u; i <= LX; ++i) rs[i] = c;
		}
		// ---- EA score (calcalnscoreflat.cpp:4-32): thread t owns DP columns [t*C, t*C + C). Two DP rows ping-pong
		// (Sp = S(i-1,.), Sn = S(i,.)) so the diagonal reads never race the writes.
		const u32 C = (LY + T) / T; // ceil((LY + 1) / T)
		float *Sp = S, *Sn = S + (LY + 1);
		for (u32 q = t; q <= LY; q += T)
			Sp[q] = 0.0f;
		__syncthreads();
		const u32 c0 = t * C;
		const u32 cmask = (1u << kshift) - 1u;
		float *s_wmax = (float *)s.wv;
		for (u32 i0 = 0; c && i0 < LX; i0 += T) {
			for (u32 k = t; k <= T && i0 + k <= LX; k += T) s_rs[k] = rs[i0 + k]; // T + 1 entries: thread 0 also reads the last
			__syncthreads();
			const u32 nl = LX - i0 < T ? LX - i0 : T;
			for (u32 rl = 0; rl < nl; ++rl) {
				const u32 b = s_rs[rl], e = s_rs[rl + 1u];
				if (e == b) continue; // a row without stored cells leaves S unchanged
				// first stored cell of this row whose DP column (col + 1) is at or right of my first column
				u32 lo = b, hi = e;
				while (lo < hi) {
					const u32 mid = (lo + hi) >> 1;
					if (((u32)(buf[mid] >> 32) & cmask) + 1u < c0) lo = mid + 1u; else hi = mid;
				}
				u32 kk = lo;
				u32 ncol = kk < e ? ((u32)(buf[kk] >> 32) & cmask) + 1u : 0xffffffffu;
				float run = 0.0f;
				for (u32 q = 0; q < C; ++q) {
					const u32 j = c0 + q;
					if (j > LY) break;
					float v = Sp[j]; // X = S(i-1, j)
					if (ncol == j) {
						const float bb = Sp[j - 1] + __uint_as_float((u32)buf[kk]); // B = S(i-1,j-1) + P
						v = fmaxf(v, bb);
						++kk;
						ncol = kk < e ? ((u32)(buf[kk] >> 32) & cmask) + 1u : 0xffffffffu;
					}
					run = (q == 0) ? v : fmaxf(run, v);
					Sn[j] = run; // prefix max inside my columns
				}
				// prefix maximum across the workgroup; threads without columns contribute 0 <= every S
				const float incl = mpc_wave_scan_max_nonneg(run);
				float excl = mpc_lane_up1(incl);
				if (lane == 0) excl = 0.0f;
				if (lane == 63u) s_wmax[w] = incl;
				__syncthreads();
				for (u32 ww = 0; ww < w; ++ww) excl = fmaxf(excl, s_wmax[ww]);
				for (u32 q = 0; q < C; ++q) {
					const u32 j = c0 + q;
					if (j > LY) break;
					Sn[j] = fmaxf(Sn[j], excl); // Y = S(i, j-1) folded in
				}
				__syncthreads();
				float *tmp = Sp; Sp = Sn; Sn = tmp;
			}
			__syncthreads(); // before the next chunk of row starts replaces this one
		}
		if (t == 0) {
			const float score = Sp[LY];
			const u32 mn = LX < LY ? LX : LY;
			p.ea[pid] = score / (float)mn; // calcposteriorflat.cpp:89 (uint -> float, IEEE divide)
		}
		__syncthreads(); // the next pair clears the DP row this one's score is read from
	}
	if (t == 0) p.info[blockIdx.x] = best;
}

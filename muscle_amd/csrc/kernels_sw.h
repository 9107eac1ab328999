// kernels_sw.h — sw_kernel: score-only affine-gap local alignment (Smith-Waterman) for lists of pairs, the numeric part of
// SWFast_SMx (sw.cpp:142-275) as CalcGuideTree_SW_BLOSUM62 uses it (swdistmx.cpp:87-127): per cell (i, j), in fp32,
//   M(i+1, j+1) = max(M(i, j), D(i, j), I(i, j), 0) + S(a_i, b_j)
//   D(i+1, j)   = max(M(i, j) + Open, D(i, j) + Ext)
//   I(i, j+1)   = max(M(i, j) + Open, I(i, j) + Ext)
// and the result is the largest M cell, or 0.0f when none is positive. No trace-back, no LA x LB matrix. Every cell is one fixed
// chain of single adds and maxima (the library is built with -ffp-contract=off, Ext is added once per step), so the value equals the
// reference's bit for bit whichever of several equal maxima wins. Borders: the reference holds -9e9f there and 0 in M(0, 0)
// (sw.cpp:166-182); here they are -infinity. Every border value enters a cell only through max(., 0) or, plus Open <= 0 / Ext <= 0,
// through D and I, which enter through max(., 0) again: a value <= 0 in their place changes no M cell (mpcgpu_sw_set_scores refuses
// Open > 0 and Ext > 0, as sw.cpp:151-152 asserts).
//
// Layout (the systolic sweep of kernels_fbc.h without its planes): a wavefront takes a work item = one row sequence X and a run of
// CONSECUTIVE column sequences of the letter buffer. Lane t owns H rows of X (rows rb * 64 * H + t * H + r; rb > 0 only in the LONG
// kernel, which walks a longer X in row blocks of 64 * H rows); at step s it stands on column s - t of the item's column axis. What
// moves from lane to lane by one DPP shift per step is the column's letter and the last row's M (a step later the diagonal of the next
// lane's first row) and D. The letter buffer holds every sequence followed by one separator letter, so the columns of a chain are one
// contiguous byte range: a lane that meets the separator has finished a pair — it hands its best cell to the pair's result (atomic
// maximum on the bits of a non-negative float: exact, order-free), clears its I row and starts the next pair with the next column.
// The fill and drain of the systolic schedule (T - 1 steps, T = lanes that own rows) is paid per chain, not per pair.
// The substitution table lives in LDS with three extra columns and two extra rows:
//   column / row alpha       the wildcard (every letter >= alpha): 0.0f against everything (blosumsmx.cpp:46-49)
//   column alpha + 1, + 2    the separator and the idle column (before the first and past the last column): -infinity, so a cell
//                            there is -infinity: M needs no reset, nothing of it can raise a best cell
//   row alpha + 1            the rows past the end of X: -infinity likewise
// The column letters reach lane 0 64 at a time: every lane loads one byte of the next 64 columns while the current 64 are swept
// (v_readlane per step). LONG: the last lane's M and D of every column go to a per-wave line in global memory, which lane 0 of the
// next row block reads back the same way; a column is read (step j) before it is rewritten (step j + 63), so one line serves.
#pragma once
#include "mpc_platform.h"

#define MPC_SW_HMAX 8                        // rows per lane; a row sequence longer than 64 * MPC_SW_HMAX rows takes the LONG kernel
#define MPC_SW_BLOCK_ROWS (64 * MPC_SW_HMAX) // rows of a row block of the LONG kernel
#define MPC_SW_ALPHA_MAX 32
#ifndef MPC_DEVICE_FENCE
#define MPC_DEVICE_FENCE() ((void)0) // the emulator: lanes meet at the wave rendezvous that follows
#endif

struct SwItem {
	u32 x;     // row sequence
	u32 col0;  // first column: byte offset into SwParams::let
	u32 ncols; // columns, the separator behind every column sequence included
	u32 out0;  // result of the item's first pair; the following pairs follow
};

struct SwParams {
	const u8 *let;      // letters of every sequence (0 .. alpha - 1, alpha = wildcard), each sequence followed by the separator alpha + 1
	const u32 *seq_off; // per sequence: offset into let
	const u32 *seq_len;
	const SwItem *items;
	u32 count;
	u32 *queue;
	const float *sub; // (alpha + 2) rows x (alpha + 3) columns, as described above
	u32 alpha;
	float open, ext;
	u32 *scores;    // bits of the results, zeroed by the host
	float *bnd;     // LONG: per wave of the grid 2 * bnd_stride floats (M line, D line)
	u64 bnd_stride; // >= columns of the longest item
};

template <int H, bool LONG>
__global__ void __launch_bounds__(256) sw_kernel(SwParams p)
{
	MPC_DYN_SMEM(smem_raw);
	float *s_sub = (float *)smem_raw;
	const int W = (int)p.alpha + 3;
	for (u32 q = threadIdx.x; q < (p.alpha + 2) * (u32)W; q += blockDim.x)
		s_sub[q] = p.sub[q];
	__syncthreads();

	const int t = threadIdx.x & 63;
	const float NINF = -__builtin_inff();
	const float open = p.open, ext = p.ext;
	const u32 SEP = p.alpha + 1, IDLE = p.alpha + 2, NOROW = (p.alpha + 1) * (u32)W;
	float *bM = nullptr, *bD = nullptr;
	if (LONG) {
		const u64 slot = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
		bM = p.bnd + slot * 2 * p.bnd_stride;
		bD = bM + p.bnd_stride;
	}

	for (;;) {
		const u32 qi = mpc_wave_first(atomicAdd(p.queue, t == 0 ? 1u : 0u));
		if (qi >= p.count)
			break;
		const u32 sx = p.items[qi].x, ncols = p.items[qi].ncols, out0 = p.items[qi].out0;
		const u8 *Y = p.let + p.items[qi].col0;
		const u32 LA = p.seq_len[sx];
		const u8 *X = p.let + p.seq_off[sx];
		const u32 nblocks = LONG ? (LA + MPC_SW_BLOCK_ROWS - 1) / MPC_SW_BLOCK_ROWS : 1u;
		for (u32 rb = 0; rb < nblocks; ++rb) {
			const u32 row0 = rb * (u32)(64 * H);
			const u32 rows = (LA - row0 < (u32)(64 * H)) ? LA - row0 : (u32)(64 * H);
			const u32 T = (rows + H - 1) / H;
			const bool more = LONG && rb + 1 < nblocks; // the block below reads this block's last row
			u32 arow[H];
			float cM[H], cI[H]; // own rows at the previous column
#pragma unroll
			for (int r = 0; r < H; ++r) {
				const u32 i = row0 + (u32)t * H + r;
				arow[r] = (i < LA) ? (u32)X[i] * (u32)W : NOROW;
				cM[r] = cI[r] = NINF;
			}
			float uM = NINF;   // M of the row above the lane's first, one column back: the diagonal of r = 0
			float dlast = NINF; // D below the lane's last row at its column: what the next lane takes
			u32 yprev = IDLE;
			float best = 0.0f;
			u32 k = 0; // pair of the item this lane is in
			const u32 nsteps = ncols + (more ? 63u : T - 1u);
			auto chunk = [&](u32 s0) -> u32 { const u32 c = s0 + (u32)t; return c < ncols ? (u32)Y[c] : IDLE; };
			auto line = [&](const float *b, u32 s0) -> float { const u32 c = s0 + (u32)t; return (LONG && rb > 0 && c < ncols) ? b[c] : NINF; };
			u32 ynext = chunk(0);
			float mnext = line(bM, 0), dnext = line(bD, 0);
			for (u32 s0 = 0; s0 < nsteps; s0 += 64) {
				const u32 ycur = ynext;
				const float mcur = mnext, dcur = dnext;
				ynext = chunk(s0 + 64);
				if (LONG) { mnext = line(bM, s0 + 64); dnext = line(bD, s0 + 64); }
				const u32 send = (nsteps - s0 < 64u) ? nsteps - s0 : 64u;
				for (u32 u = 0; u < send; ++u) {
					float nM = mpc_lane_up1(cM[H - 1]);
					float nD = mpc_lane_up1(dlast);
					u32 yc = (u32)mpc_lane_up1((int)yprev);
					const u32 y0 = mpc_read_lane(ycur, u);
					float m0 = NINF, d0 = NINF;
					if (LONG) { m0 = mpc_read_lane(mcur, u); d0 = mpc_read_lane(dcur, u); }
					if (t == 0) { yc = y0; nM = m0; nD = d0; }
					const float *scol = s_sub + yc;
					float diag = uM, d = nD;
#pragma unroll
					for (int r = 0; r < H; ++r) {
						const float S = scol[arow[r]];
						const float oM = cM[r], oI = cI[r];
						const float x = fmaxf(fmaxf(fmaxf(diag, d), oI), 0.0f) + S; // sw.cpp:198-216
						const float mo = diag + open;                               // sw.cpp:233, 248
						d = fmaxf(d + ext, mo);                                      // sw.cpp:234-239
						cI[r] = fmaxf(oI + ext, mo);                                 // sw.cpp:249-254
						cM[r] = x;
						best = fmaxf(best, x);                                       // sw.cpp:217-222
						diag = oM;
					}
					dlast = d;
					uM = nM;
					yprev = yc;
					if (more && t == 63) { // column s0 + u - 63 of the last row, for lane 0 of the block below
						const u32 c = s0 + u - 63u;
						if (s0 + u >= 63u && c < ncols) { bM[c] = cM[H - 1]; bD[c] = dlast; }
					}
					if (__ballot(yc >= SEP)) {
						if (yc >= SEP) {
#pragma unroll
							for (int r = 0; r < H; ++r) cI[r] = NINF;
							if (yc == SEP) {
								if (best > 0.0f) atomicMax(p.scores + out0 + k, __float_as_uint(best));
								++k;
								best = 0.0f;
							}
						}
					}
				}
			}
			if (more) MPC_DEVICE_FENCE(); // the lines this wave wrote are read back by other lanes of it
			MPC_WAVE_LDS_ORDER();
		}
	}
}

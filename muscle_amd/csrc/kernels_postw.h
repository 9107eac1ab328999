// kernels_postw.h — post_wide_kernel: post_kernel's job (kernels_post.h: probabilities, row-major order, EA score, FromPost, the
// column-major rank) with a whole WORKGROUP per pair, for the candidate lists post_rows_kernel does not take (sequences beyond
// ~12 000 positions: tens of millions of candidates for a 6 000 x 60 000 pair). Same inputs, same packed record byte for byte:
//   [rowcnt: LX] [colcnt: LY] [ent: 2*nnz = {P bits, col}] [row: nnz] [tperm: nnz]
// and nnz / ea / flags as post_kernel leaves them (overflow: flag 1, nnz 0, ea 0). The raw candidate list is only read.
//
// What replaces the two one-wave bitonic sorts and the sequential cursor:
//  * keys (flat index << 32 | P bits) in one of two buffers (LDS while the list fits lds_cap entries, else two global slots per
//    resident workgroup), sorted by the flat index with a STABLE LSD radix sort, 8 bits per pass over the index's significant bits
//    (key shift + bits(LX - 1): 2-4 passes). A pass: digit histogram in LDS, exclusive scan, then tile by tile (one key per thread)
//    the rank of a key among the keys of its digit: inside the wave from eight ballots, across the waves from a [wave][digit]
//    table that the first 256 threads scan. Keys are unique, so the sorted order — and everything derived from it — does not
//    depend on how the waves are scheduled.
//  * a table of LX + 1 row starts in global scratch (LX reaches 65 535), written at the row boundaries of the sorted list; the EA
//    loop stages it through LDS a workgroup's width at a time.
//  * the EA recurrence in post_kernel's formulation (calcalnscoreflat.cpp:4-32: T(j) = max(S(i-1,j), S(i-1,j-1) + P(i,j)), then a
//    prefix maximum over j) with T lanes: a lane owns ceil((LY+1)/T) consecutive columns, finds its first stored cell of the row by
//    binary search, and the prefix maximum crosses the workgroup as a wave scan plus one LDS word per wave. max is exact; the only
//    rounding is the one add per stored cell, as in the reference. Rows without cells are skipped.
//  * FromPost (mysparsemx.cpp:115-152): rank among the kept (P >= 0.01f) from a workgroup scan tile by tile.
//  * tperm: the kept entries are row-major, so a stable radix sort of (col << 32 | rank) by the COLUMN alone gives the
//    column-major order (rows stay ascending inside a column); no col * LX + row keys, no second full sort.
#pragma once
#include "kernels_post.h"

#ifdef MPC_EMU
#define MPC_POSTW_THREADS 128 // fewer fibers per workgroup; the kernel is written for any multiple of 64
#else
#define MPC_POSTW_THREADS 1024
#endif
#define MPC_POSTW_WAVES_MAX 16

struct PostWideParams {
	const u32 *pair_x, *pair_y; // per batch-local pair
	const u32 *seq_len;
	const u64 *cand; // read only: dense_post_raw_kernel reads the scores afterwards
	u32 capc;
	const u32 *cand_cnt;
	int use_fma;
	u32 lds_cap;        // entries of each of the two LDS key buffers; longer lists ping-pong in key_scratch
	u32 srow_cap;       // floats of each of the two LDS DP rows; wider pairs use srow_scratch
	u64 *key_scratch;   // per workgroup: 2 * key_stride u64
	u64 key_stride;
	u32 *rs_scratch;    // per workgroup: rs_stride u32 (row starts, LXmax + 1)
	u64 rs_stride;
	float *srow_scratch; // per workgroup: srow_stride floats (2 * (LYmax + 1))
	u64 srow_stride;
	u64 *info;          // per workgroup: (candidates << 8 | radix passes) of its pair with the most candidates
	u32 *res;
	u64 res_stride;
	u32 *nnz;
	float *ea;
	u32 *flags;
	u32 count;
	u32 long_min;
};

// LDS of post_wide_kernel for a workgroup of `threads`: digit offsets, [wave][digit] counts and bases, the staged row starts,
// two words per wave for the scans (double-buffered), the two DP rows, the two key buffers
__host__ __device__ __forceinline__ size_t mpc_postw_fixed_words(u32 threads) { return 256 + 2 * (size_t)(threads / 64) * 256 + (threads + 1) + 2 * MPC_POSTW_WAVES_MAX + 1; }
__host__ __device__ __forceinline__ size_t mpc_postw_smem(u32 threads, u32 lds_cap, u32 srow_cap)
{
	return (((mpc_postw_fixed_words(threads) + 2 * (size_t)srow_cap) * 4 + 7) & ~(size_t)7) + 16 * (size_t)lds_cap;
}

__device__ __forceinline__ u32 mpc_bits_of(u32 v) { u32 b = 0; while (v >> b) ++b; return b; } // bits to hold v (0 for 0)

struct PostwLds { u32 *off, *wcnt, *wbase, *wv; };

// Stable LSD radix sort of n u64 keys by their bits [32, 32 + 8 * passes), all threads of the workgroup. The keys start in `a`,
// `b` is the other buffer; returns the buffer that holds the sorted keys. Ends with a barrier.
__device__ __forceinline__ u64 *mpc_postw_sort(u64 *a, u64 *b, u32 n, u32 passes, const PostwLds &s)
{
	const u32 t = threadIdx.x, T = blockDim.x, lane = t & 63u, w = t >> 6, NW = T >> 6;
	for (u32 ps = 0; ps < passes; ++ps) {
		const u32 sh = 32u + 8u * ps;
		for (u32 d = t; d < 256u; d += T) s.off[d] = 0;
		for (u32 x = t; x < NW * 256u; x += T) s.wcnt[x] = 0;
		__syncthreads();
		for (u32 q = t; q < n; q += T)
			atomicAdd(&s.off[(u32)(a[q] >> sh) & 255u], 1u);
		__syncthreads();
		if (w == 0) { // exclusive scan of the 256 digit counts: four digits per lane of the first wave
			u32 v[4], sum = 0;
			for (u32 k = 0; k < 4; ++k) { v[k] = s.off[4 * lane + k]; sum += v[k]; }
			u32 incl = sum;
			for (int d = 1; d < 64; d <<= 1) {
				const u32 o = __shfl_up(incl, d);
				if ((int)lane >= d) incl += o;
			}
			u32 run = incl - sum;
			for (u32 k = 0; k < 4; ++k) { s.off[4 * lane + k] = run; run += v[k]; }
		}
		__syncthreads();
		for (u32 q0 = 0; q0 < n; q0 += T) {
			const u32 q = q0 + t;
			const bool have = q < n;
			const u64 key = have ? a[q] : 0ull;
			const u32 dg = (u32)(key >> sh) & 255u;
			// the lanes of this wave that hold a key of my digit
			u64 peers = __ballot(have);
			for (u32 bit = 0; bit < 8; ++bit) {
				const bool on = (dg >> bit) & 1u;
				const u64 m = __ballot(have && on);
				peers &= on ? m : ~m;
			}
			const u32 before = (u32)__popcll(peers & ((1ull << lane) - 1ull));
			if (have && before == 0) s.wcnt[w * 256u + dg] = (u32)__popcll(peers);
			__syncthreads();
			for (u32 d = t; d < 256u; d += T) { // where each wave's keys of digit d go; the counts are left zeroed for the next tile
				u32 run = s.off[d];
				for (u32 ww = 0; ww < NW; ++ww) {
					const u32 v = s.wcnt[ww * 256u + d];
					s.wbase[ww * 256u + d] = run;
					s.wcnt[ww * 256u + d] = 0;
					run += v;
				}
				s.off[d] = run;
			}
			__syncthreads();
			if (have) b[s.wbase[w * 256u + dg] + before] = key;
		}
		__syncthreads();
		u64 *tmp = a; a = b; b = tmp;
	}
	return a;
}

// exclusive prefix of v over the workgroup (thread order) and the total; `slot` alternates between consecutive calls so that
// one barrier per call is enough
__device__ __forceinline__ u32 mpc_postw_scan_add(u32 v, u32 *wv, u32 slot, u32 *total)
{
	const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6, NW = blockDim.x >> 6;
	u32 incl = v;
	for (int d = 1; d < 64; d <<= 1) {
		const u32 o = __shfl_up(incl, d);
		if ((int)lane >= d) incl += o;
	}
	u32 *ws = wv + slot * MPC_POSTW_WAVES_MAX;
	if (lane == 63u) ws[w] = incl;
	__syncthreads();
	u32 base = 0, tot = 0;
	for (u32 ww = 0; ww < NW; ++ww) { const u32 x = ws[ww]; base += ww < w ? x : 0u; tot += x; }
	*total = tot;
	return base + incl - v;
}

__global__ void __launch_bounds__(MPC_POSTW_THREADS) post_wide_kernel(PostWideParams p)
{
	MPC_DYN_SMEM(smem_raw);
	const u32 t = threadIdx.x, T = blockDim.x, lane = t & 63u, w = t >> 6, NW = T >> 6;
	PostwLds s;
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
		u32 *rec = p.res + (u64)pid * p.res_stride;
		const u32 c = p.cand_cnt[pid];
		if (c > p.capc) { // overflow: reported to the host, which retries with a larger capacity
			if (t == 0) { p.flags[pid] = 1u; p.nnz[pid] = 0; p.ea[pid] = 0.0f; }
			continue;
		}
		if (t == 0) p.flags[pid] = 0u;
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
		for (u32 q = t; q < LX + LY; q += T)
			rec[q] = 0;
		__syncthreads();
		u64 *buf = mpc_postw_sort(A, B, c, passes, s); // row-major: rows ascending, columns ascending
		u64 *oth = buf == A ? B : A;

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
		const float score = Sp[LY];
		const u32 mn = LX < LY ? LX : LY;
		const float ea = score / (float)mn; // calcposteriorflat.cpp:89 (uint -> float, IEEE divide)

		// ---- sparsify (mysparsemx.cpp:115-152): keep P >= 0.01f; rank = position among kept
		u32 mykept = 0;
		for (u32 q = t; q < c; q += T)
			mykept += (__uint_as_float((u32)buf[q]) >= MPC_MIN_SPARSE_PROB) ? 1u : 0u;
		u32 nnz = 0;
		(void)mpc_postw_scan_add(mykept, s.wv, 0, &nnz);
		u32 *rowcnt = rec, *colcnt = rec + LX;
		u32 *ent = rec + LX + LY;
		u32 *rowv = ent + 2 * (u64)nnz;
		u32 *tperm = rowv + nnz;
		u32 base = 0, slot = 1;
		for (u32 q0 = 0; q0 < c; q0 += T, slot ^= 1u) {
			const u32 q = q0 + t;
			const u64 key = q < c ? buf[q] : 0ull;
			const bool k = q < c && __uint_as_float((u32)key) >= MPC_MIN_SPARSE_PROB;
			u32 tot = 0;
			const u32 rank = base + mpc_postw_scan_add(k ? 1u : 0u, s.wv, slot, &tot);
			if (k) {
				const u32 idx = (u32)(key >> 32);
				const u32 row = idx >> kshift, col = idx & cmask;
				ent[2 * (u64)rank] = (u32)key;
				ent[2 * (u64)rank + 1] = col;
				rowv[rank] = row;
				atomicAdd(&rowcnt[row], 1u);
				atomicAdd(&colcnt[col], 1u);
				oth[rank] = ((u64)col << 32) | (u64)rank;
			}
			base += tot;
		}
		__syncthreads();
		// ---- column-major rank of every kept entry: the ranks, stably sorted by column
		const u64 *cm = mpc_postw_sort(oth, buf, nnz, (mpc_bits_of(LY - 1u) + 7u) / 8u, s);
		for (u32 q = t; q < nnz; q += T)
			tperm[(u32)cm[q]] = q;
		if (t == 0) { p.nnz[pid] = nnz; p.ea[pid] = ea; }
		__syncthreads();
	}
	if (t == 0) p.info[blockIdx.x] = best;
}

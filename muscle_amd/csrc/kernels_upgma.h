// kernels_upgma.h — UPGMA5 on the device: ScaleDistMx / FixEADistMx (upgma5.cpp:504-563), the initialisation of UPGMA5::Run
// (upgma5.cpp:131-159) and its join loop (upgma5.cpp:163-304), restated so that every float is the reference's bit for bit.
//
// The triangle. The reference keeps m_Dist under TriangleSubscript (upgma5.h:64-73: row i holds its partners j < i). Here the n (n - 1) / 2
// distances stay in the order they arrive in — InitPairs order (mpcflat.cpp:145-155), pair (i, j), i < j, at i (2n - i - 1) / 2 + j - i - 1,
// what mpcgpu_sw_scores and mpcgpu_ea_scores write — under 64-bit subscripts (mpc_tri). Which cell of memory holds a distance changes no
// value: every statement of the reference names a PAIR of rows, and the pair is what is looked up.
//
// What makes the reference O(n^2), and what has to be carried along to equal it: it keeps for every row its smallest distance and the partner
// that has it (m_MinDist, m_NearestNeighbor), finds the next join as the smallest m_MinDist, rewrites ONE row per join (the new node takes
// the row of its left child) and computes that row's new minimum — and never repairs the cached minimum of any OTHER row: m_MinDist[j] stays
// what it was although the distance it was taken from has been overwritten or its partner has died. Only the partner is redirected
// (m_NearestNeighbor[j] == Rmin becomes Lmin, upgma5.cpp:249-259). The join picked next is therefore not always the closest pair of the
// current matrix, and the tree is the tree of exactly this procedure. All scans are ascending with a strict '<' against FLT_MAX, so among
// equal values the lowest index wins, and a row without any distance below FLT_MAX keeps the neighbour UINT_MAX.
//
// Kernels:
//   upgma_sw_norm_kernel   Score / ((Li + Lj) / 2.0f) (swdistmx.cpp:75-76) over the raw scores of mpcgpu_sw_scores; many workgroups
//   upgma_minmax_kernel    per workgroup the smallest and the largest distance -> partial[2 b], partial[2 b + 1]
//   upgma_transform_kernel every workgroup folds the partials (no atomics, no second pass over the triangle), then rewrites its share:
//                          SCALE * (Max - d) / (Max - Min), SCALE * (d - Min) / (Max - Min), 1 - d, or d; then d < 0 -> 0 (upgma5.cpp:140-145)
//   upgma_init_kernel      a row per wavefront: its minimum and the lowest partner that has it
//   upgma_join_kernel      ONE persistent workgroup, all n - 1 joins. Per join: the argmin of m_MinDist over the live rows, the update of
//                          row Lmin with the linkage formula and the redirect, the new row's minimum, and lane 0's scalar writes. Three
//                          barriers per join, no other synchronisation: a single workgroup never waits for another one. LDS = true keeps
//                          m_MinDist, m_NearestNeighbor and m_NodeIndex in LDS (12 bytes per row), LDS = false in global memory.
// Minimum and maximum of ScaleDistMx: the reference folds with std::min / std::max from entry (0, 1) on. Floats that compare equal are the
// same float except +0 and -0; so that a parallel fold has one answer, -0 counts as the smaller and +0 as the larger of the two here. (The
// reference's answer for a matrix whose extreme is a zero of both signs depends on which it meets first.)
#pragma once
#include "mpc_platform.h"

#define MPC_UPGMA_NMAX 65536u // the reference's 32-bit uIndex1 * (uIndex1 - 1) wraps beyond (upgma5.h:68)
#ifdef MPC_EMU
#define MPC_UPGMA_THREADS 128 // fewer fibers per workgroup; the kernels are written for any multiple of 64
#else
#define MPC_UPGMA_THREADS 1024
#endif
#define MPC_UPGMA_LDS_ROWS_MAX 12288u // 12 bytes per row + the fold scratch within gfx950's 160 KB
#define MPC_UPGMA_SCRATCH_BYTES 256u  // two sets of 16 (value, index) slots for the folds of the join kernel
#define MPC_UPGMA_FLT_MAX __FLT_MAX__
#define MPC_UPGMA_NONE 0xffffffffu // UINT_MAX: no neighbour / a deleted row

enum { MPC_UPGMA_T_NONE = 0, MPC_UPGMA_T_SCALE_SIM = 1, MPC_UPGMA_T_SCALE_DIST = 2, MPC_UPGMA_T_EA = 3 };
enum { MPC_UPGMA_L_AVG = 0, MPC_UPGMA_L_MIN = 1, MPC_UPGMA_L_MAX = 2, MPC_UPGMA_L_BIASED = 3 };
// status word of a run: 0, or these in the top byte (both may be set: EA_RANGE is the refusal then) with the join index of NO_MIN below it
#define MPC_UPGMA_ST_NO_MIN 0x01000000u   // no live row has a minimum below FLT_MAX (the reference asserts, upgma5.cpp:197-199)
#define MPC_UPGMA_ST_EA_RANGE 0x02000000u // EA input outside 0 .. 1 (the reference dies, upgma5.cpp:512)

// subscript of the pair {a, b}, a != b, both < n
__device__ __forceinline__ u64 mpc_tri(u32 n, u32 a, u32 b)
{
	const u32 i = a < b ? a : b, j = a < b ? b : a;
	return (u64)i * (2ull * n - i - 1ull) / 2ull + (u64)(j - i - 1u);
}

// (v, i) := the smaller of (v, i) and (ov, oi): the lower value, of equal values the lower index — what an ascending scan with '<' keeps
__device__ __forceinline__ void mpc_argmin_take(float &v, u32 &i, float ov, u32 oi)
{
	if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// over the wave, the result in every lane
__device__ __forceinline__ void mpc_wave_argmin(float &v, u32 &i)
{
	for (unsigned d = 32; d >= 1; d >>= 1) {
		const float ov = __shfl_down(v, d);
		const u32 oi = __shfl_down(i, d);
		mpc_argmin_take(v, i, ov, oi);
	}
	v = mpc_read_lane(v, 0u);
	i = mpc_read_lane(i, 0u);
}
// over the workgroup (at most 16 waves... 64 would do), the result in every lane; sv / si: a slot per wave; one barrier. The caller must not
// reuse sv / si before another barrier has passed.
__device__ __forceinline__ void mpc_block_argmin(float &v, u32 &i, float *sv, u32 *si)
{
	mpc_wave_argmin(v, i);
	const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
	if (lane == 0) { sv[w] = v; si[w] = i; }
	__syncthreads();
	v = lane < nw ? sv[lane] : MPC_UPGMA_FLT_MAX;
	i = lane < nw ? si[lane] : MPC_UPGMA_NONE;
	mpc_wave_argmin(v, i);
}

__device__ __forceinline__ float mpc_min_z(float a, float b) { return (b < a || (b == a && (__float_as_uint(b) >> 31) != 0u)) ? b : a; }
__device__ __forceinline__ float mpc_max_z(float a, float b) { return (b > a || (b == a && (__float_as_uint(b) >> 31) == 0u)) ? b : a; }
// smallest and largest over the workgroup in every lane; s: two slots per wave; two barriers
__device__ __forceinline__ void mpc_block_minmax(float &lo, float &hi, float *s)
{
	for (unsigned d = 32; d >= 1; d >>= 1) {
		lo = mpc_min_z(lo, __shfl_down(lo, d));
		hi = mpc_max_z(hi, __shfl_down(hi, d));
	}
	const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
	if (lane == 0) { s[2 * w] = lo; s[2 * w + 1] = hi; }
	__syncthreads();
	lo = s[0];
	hi = s[1];
	for (u32 q = 1; q < nw; ++q) { lo = mpc_min_z(lo, s[2 * q]); hi = mpc_max_z(hi, s[2 * q + 1]); }
	__syncthreads();
}

// swdistmx.cpp:75-76: MeanLength = (Li + Lj) / 2.0f (the unsigned sum converted, the halving exact), NormScore = SWScore / MeanLength
__global__ void __launch_bounds__(256) upgma_sw_norm_kernel(float *tri, u32 n, const u32 *seq_len)
{
	for (u32 i = blockIdx.x; i + 1 < n; i += gridDim.x) {
		float *row = tri + mpc_tri(n, i, i + 1);
		const u32 Li = seq_len[i];
		for (u32 j = i + 1 + threadIdx.x; j < n; j += blockDim.x) {
			const float mean = (float)(Li + seq_len[j]) / 2.0f;
			row[j - i - 1] = row[j - i - 1] / mean;
		}
	}
}

// upgma5.cpp:524-535; m >= 1 distances, 2 * gridDim.x partials, dynamic LDS: 2 floats per wave
__global__ void __launch_bounds__(256) upgma_minmax_kernel(const float *tri, u64 m, float *partial)
{
	MPC_DYN_SMEM(smem_raw);
	float lo = tri[0], hi = tri[0];
	for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (u64)gridDim.x * blockDim.x) {
		const float d = tri[q];
		lo = mpc_min_z(lo, d);
		hi = mpc_max_z(hi, d);
	}
	mpc_block_minmax(lo, hi, (float *)smem_raw);
	if (threadIdx.x == 0) { partial[2 * blockIdx.x] = lo; partial[2 * blockIdx.x + 1] = hi; }
}

// upgma5.cpp:538-560 / 504-519, then the clamp of upgma5.cpp:140-145. stat[0], stat[1]: Min and Max of a scaling mode; status: see above
__global__ void __launch_bounds__(256) upgma_transform_kernel(float *tri, u64 m, int mode, const float *partial, u32 nparts, float *stat, u32 *status)
{
	MPC_DYN_SMEM(smem_raw);
	float Min = 0.0f, Max = 0.0f;
	if (mode == MPC_UPGMA_T_SCALE_SIM || mode == MPC_UPGMA_T_SCALE_DIST) {
		Min = partial[0];
		Max = partial[1];
		for (u32 q = threadIdx.x; q < nparts; q += blockDim.x) { Min = mpc_min_z(Min, partial[2 * q]); Max = mpc_max_z(Max, partial[2 * q + 1]); }
		mpc_block_minmax(Min, Max, (float *)smem_raw);
		if (blockIdx.x == 0 && threadIdx.x == 0) { stat[0] = Min; stat[1] = Max; }
	}
	const float SCALE = 10.0f;
	bool bad = false;
	for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < m; q += (u64)gridDim.x * blockDim.x) {
		float d = tri[q];
		if (mode == MPC_UPGMA_T_SCALE_SIM) d = SCALE * (Max - d) / (Max - Min);
		else if (mode == MPC_UPGMA_T_SCALE_DIST) d = SCALE * (d - Min) / (Max - Min);
		else if (mode == MPC_UPGMA_T_EA) { bad = bad || !(d >= 0.0f && d <= 1.0f); d = 1 - d; }
		if (d < 0) d = 0;
		tri[q] = d;
	}
	if (bad) atomicOr(status, MPC_UPGMA_ST_EA_RANGE);
}

// upgma5.cpp:111-118, 133-159: a row's partners in ascending order, '<' against FLT_MAX
__global__ void __launch_bounds__(256) upgma_init_kernel(const float *tri, u32 n, float *mn, u32 *nn, u32 *node)
{
	const u32 lane = threadIdx.x & 63u;
	const u32 nwv = gridDim.x * (blockDim.x >> 6);
	for (u32 r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < n; r += nwv) {
		float v = MPC_UPGMA_FLT_MAX;
		u32 bi = MPC_UPGMA_NONE;
		for (u32 j = lane; j < n; j += 64u) {
			if (j == r) continue;
			const float d = tri[mpc_tri(n, r, j)];
			if (d < v) { v = d; bi = j; }
		}
		mpc_wave_argmin(v, bi);
		if (lane == 0) { mn[r] = v; nn[r] = bi; node[r] = r; }
	}
}

struct UpgmaJoinParams {
	float *tri;
	u32 n;
	int linkage;
	float *mn; // m_MinDist, m_NearestNeighbor, m_NodeIndex as upgma_init_kernel left them (LDS = false: the working copy)
	u32 *nn;
	u32 *node;
	float *height; // n - 1
	u32 *left, *right;
	float *llen, *rlen;
	u32 *status;
};

__device__ __forceinline__ float mpc_upgma_link(int linkage, float dL, float dR)
{
	const float avg = (dL + dR) / 2;          // AVG, upgma5.cpp:10-13
	const float mi = dR < dL ? dR : dL;       // std::min(dL, dR)
	const float ma = dL < dR ? dR : dL;       // std::max(dL, dR)
	if (linkage == MPC_UPGMA_L_AVG) return avg;
	if (linkage == MPC_UPGMA_L_MIN) return mi;
	if (linkage == MPC_UPGMA_L_MAX) return ma;
	return 0.1f * avg + (1 - 0.1f) * mi;      // upgma5.cpp:242: two products and a sum, each rounded (-ffp-contract=off)
}

template <bool LDS>
__global__ void __launch_bounds__(MPC_UPGMA_THREADS) upgma_join_kernel(UpgmaJoinParams p)
{
	MPC_DYN_SMEM(smem_raw);
	const u32 n = p.n, T = blockDim.x, tid = threadIdx.x;
	float *svA = (float *)smem_raw;
	u32 *siA = (u32 *)smem_raw + 16;
	float *svB = (float *)smem_raw + 32;
	u32 *siB = (u32 *)smem_raw + 48;
	float *mn = LDS ? (float *)(smem_raw + MPC_UPGMA_SCRATCH_BYTES) : p.mn;
	u32 *nn = LDS ? (u32 *)(smem_raw + MPC_UPGMA_SCRATCH_BYTES) + n : p.nn;
	u32 *node = LDS ? (u32 *)(smem_raw + MPC_UPGMA_SCRATCH_BYTES) + 2 * (size_t)n : p.node;
	if (LDS) {
		for (u32 j = tid; j < n; j += T) { mn[j] = p.mn[j]; nn[j] = p.nn[j]; node[j] = p.node[j]; }
	}
	__syncthreads();
	const int linkage = p.linkage;
	for (u32 k = 0; k + 1 < n; ++k) {
		// upgma5.cpp:178-195
		float v = MPC_UPGMA_FLT_MAX;
		u32 L = MPC_UPGMA_NONE;
		for (u32 j = tid; j < n; j += T) {
			if (node[j] == MPC_UPGMA_NONE) continue;
			const float d = mn[j];
			if (d < v) { v = d; L = j; }
		}
		mpc_block_argmin(v, L, svA, siA);
		const u32 R = L < n ? nn[L] : MPC_UPGMA_NONE;
		if (L >= n || R >= n || R == L) { // the same in every lane
			// beside what the transform kernel left, not over it: of an EA matrix that is out of range AND leaves no minimum the
			// reference dies in FixEADistMx, and the host names that refusal first
			if (tid == 0) atomicOr(p.status, MPC_UPGMA_ST_NO_MIN | k);
			break;
		}
		// upgma5.cpp:212-271
		float nv = MPC_UPGMA_FLT_MAX;
		u32 ni = MPC_UPGMA_NONE;
		for (u32 j = tid; j < n; j += T) {
			if (j == L || j == R || node[j] == MPC_UPGMA_NONE) continue;
			const u64 vL = mpc_tri(n, L, j);
			const float nd = mpc_upgma_link(linkage, p.tri[vL], p.tri[mpc_tri(n, R, j)]);
			if (nn[j] == R) nn[j] = L; // upgma5.cpp:249-259
			p.tri[vL] = nd;
			if (nd < nv) { nv = nd; ni = j; }
		}
		mpc_block_argmin(nv, ni, svB, siB);
		// upgma5.cpp:276-298
		if (tid == 0) {
			const float h = p.tri[mpc_tri(n, L, R)] / 2;
			const u32 uL = node[L], uR = node[R];
			const float hL = uL < n ? 0 : p.height[uL - n];
			const float hR = uR < n ? 0 : p.height[uR - n];
			p.left[k] = uL;
			p.right[k] = uR;
			p.llen[k] = h - hL;
			p.rlen[k] = h - hR;
			p.height[k] = h;
			node[L] = n + k;
			nn[L] = ni;
			mn[L] = nv;
			node[R] = MPC_UPGMA_NONE;
		}
		__syncthreads();
	}
}

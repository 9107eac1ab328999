// kernels_fbcoop.h — the row-block forward/backward sweep of kernels_fb.h (fb_kernel<H, MEGA, LONG = true>) with the W wavefronts
// of a workgroup on ONE pair: CalcFwdFlat (fwdflat3.cpp:12-153), CalcBwdFlat (bwdflat3.cpp:10-184), CalcTotalProbFlat
// (totalprobflat.cpp:3-16) and the Score/threshold half of CalcPostFlat (calcposteriorflat.cpp:9-26), same cells, same expressions,
// same bits. What changes is who computes a row block and when.
//
// fb_kernel<.., LONG> walks the NB row blocks (64*H rows each) of a pair with one wave, block after block. The blocks are a pipeline,
// though: block b+1 reads row i0 of block b 64 columns at a time, and lane 63 of block b finishes column j at step j+63 — so block b+1
// may run its steps [64k, 64k+63] once block b has finished step 64k+126: a lag of two 64-step MACRO-STEPS. Here
//   - a workgroup takes one pair at a time from the launch's work queue;
//   - wave w of W owns blocks w, w+W, w+2W, ... of the forward sweep, and the same positions counted from the bottom in the backward sweep;
//   - all W waves run one common loop of macro-steps with one workgroup barrier per macro-step. A block takes M macro-steps
//     (forward: ceil((LY+64)/64), backward: ceil((LY+63)/64)), block b starts at macro-step
//         start(b) = max(start(b-1) + 2, start(b-W) + M) = (b / W) * max(M, 2W) + 2 * (b % W),
//     and the loop has start(NB-1) + M trips: a function of LX, LY, H and W alone, so every wave — one with fewer blocks or with none
//     included — meets the same number of barriers. No wave waits on a flag, and nothing is signalled outside the workgroup;
//   - every block boundary of the pair has its own line-buffer row (5 forward + 3 backward states x bnd_ld), since several are live at
//     once. A wave's stores to a boundary row are separated from the next block's loads by the workgroup-scope fence in front of the
//     barrier that ends the macro-step (the waves of a workgroup share the CU's L1);
//   - the forward M plane keeps one region per block, one slot per resident WORKGROUP;
//   - the wave that owns the last block forms the total and hands it to the others through LDS behind a barrier;
//   - the W waves append to the pair's one candidate list through a counter in LDS (one atomic per step that has candidates), so the
//     ORDER of the list differs from fb_kernel's; the finishing kernels take the candidates in any order (kernels_post.h). cand_cnt may
//     exceed capc as before (overflow, detected by the host).
#pragma once
#include "kernels_fb.h"

#define MPC_FB_COOP_LDS_BYTES 16 // dynamic LDS behind the emission tables: queue index, total, candidate counter (+ padding)

// Threads per workgroup the instantiation is compiled for. The VGPRs of H rows per lane decide how many waves a SIMD holds (4 SIMDs
// per CU), and the bound is what keeps the compiler inside that budget without spilling: 7 rows — 254 VGPRs under a bound of 512
// threads (2 waves per SIMD), with profiles 253 + spills there, so 256 threads; 4 rows — 168 VGPRs and six spilled under 768
// threads (3 per SIMD), none under 512; 1 row (tests) — 119 under 1024.
template <int H, bool MEGA> struct FbCoopBounds { static constexpr int threads = H >= 5 ? (MEGA ? 256 : 512) : H >= 2 ? 512 : 1024; };

template <int H, bool MEGA>
__global__ void __launch_bounds__((FbCoopBounds<H, MEGA>::threads)) fb_coop_kernel(FbParams p)
{
	MPC_DYN_SMEM(smem_raw);
	__shared__ MpcCoef s_coef[MPC_COEF_ENTRIES]; // as in fb_kernel: a compile-time LDS address
	float *s_match = (float *)smem_raw;                          // A*A (MEGA: the feature tables)
	float *s_ins = s_match + p.A * p.A;                          // A   (MEGA: unused)
	// per workgroup (dynamic LDS: one copy per workgroup on the emulator too): [0] queue index, [1] total, [2] candidates of the pair
	u32 *s_wg = (u32 *)(s_match + (MEGA ? p.mg_tab_floats : (u32)(p.A * p.A + p.A)));
	if (threadIdx.x < MPC_COEF_ENTRIES)
		mpc_coef_table_init(s_coef, (int)threadIdx.x);
	if (MEGA) {
		for (u32 q = threadIdx.x; q < p.mg_tab_floats; q += blockDim.x)
			s_match[q] = p.mg_tab[q];
	} else {
		for (int q = threadIdx.x; q < p.A * p.A; q += blockDim.x)
			s_match[q] = p.match[q];
		for (int q = threadIdx.x; q < p.A; q += blockDim.x)
			s_ins[q] = p.ins[q];
	}
	__syncthreads();

	const int t = threadIdx.x & 63;
	const int W = (int)(blockDim.x >> 6);
	const int w = (int)mpc_wave_first(threadIdx.x >> 6); // wave-uniform (SGPR): every branch on it is a scalar branch
	float *fm = p.fm_scratch + (u64)blockIdx.x * p.fm_stride;
	float *bnd = p.bnd + (u64)blockIdx.x * p.bnd_stride;
	const u32 ld = p.bnd_ld;
	const float LZ = MPC_LOG_ZERO;
	const float tSM = p.tSM, tSI = p.tSI, tSJ = p.tSJ, tMM = p.tMM, tMI = p.tMI, tMJ = p.tMJ;
	const float tII = p.tII, tIM = p.tIM, tJJ = p.tJJ, tJM = p.tJM;
	const int A = p.A;
	u32 mg_base[MPC_MEGA_FMAX], mg_alpha[MPC_MEGA_FMAX]; // wave-uniform (SGPRs)
#pragma unroll
	for (int f = 0; f < MPC_MEGA_FMAX; ++f) { mg_base[f] = MEGA ? p.mg_base[f] : 0u; mg_alpha[f] = MEGA ? p.mg_alpha[f] : 0u; }

	for (;;) {
		// Work queue, one grab per WORKGROUP: wave 0 takes the index as fb_kernel's waves do (kernels_fb.h on why it is not
		// `if (lane == 0) atomicAdd`) and leaves it in LDS. The barriers of the sweeps below (at least one each) separate the other
		// waves' read from wave 0's next write.
		if (w == 0) {
			const u32 grab = mpc_wave_first(atomicAdd(p.queue, t == 0 ? 1u : 0u));
			if (t == 0) { s_wg[0] = grab; s_wg[2] = 0u; }
		}
		__syncthreads();
		const u32 qi = mpc_wave_first(s_wg[0]);
		if (qi >= p.count)
			break;
		const u32 pid = p.order[qi];
		const u32 sx = p.pair_x[pid], sy = p.pair_y[pid];
		const int LX = (int)p.seq_len[sx], LY = (int)p.seq_len[sy];
		const u8 *X = p.seq_code + p.seq_off[sx];
		const u8 *Y = p.seq_code + p.seq_off[sy];
		constexpr int R = 64 * H;        // rows per block
		const int NB = (LX + R - 1) / R; // row blocks
		int T = 64;                      // lanes of the current block that own at least one row

		float cM[H], cIX[H], cJX[H], cIY[H], cJY[H]; // own rows at the previous column
		float insx[H];
		int mrow[H];
		u64 xl[MEGA ? H : 1];
		const u64 *PX = MEGA ? p.mg_prof + p.seq_off[sx] : nullptr, *PY = MEGA ? p.mg_prof + p.seq_off[sy] : nullptr;
		const float *IX = MEGA ? p.mg_ins + p.seq_off[sx] : nullptr, *IY = MEGA ? p.mg_ins + p.seq_off[sy] : nullptr;
		u32 ylo_prev = 0, yhi_prev = 0;
		float insy_prev = 0.0f;
#pragma unroll
		for (int r = 0; r < H; ++r) { // (a block sets them at its first macro-step)
			cM[r] = cIX[r] = cJX[r] = cIY[r] = cJY[r] = LZ;
			insx[r] = 0.0f; mrow[r] = 0; xl[MEGA ? r : 0] = 0ull;
		}

		// ------------------------------------------------------------------ forward
		{
		const int M = (LY + 64 + 63) >> 6, P = M > 2 * W ? M : 2 * W; // macro-steps of a block; between two blocks of a wave
		const int G = ((NB - 1) / W) * P + 2 * ((NB - 1) % W) + M;  // trips: the same for every wave
		int b = w, st = 2 * w;                                      // the wave's current block and its start macro-step
		int i0 = 0, nsteps = 0;
		float *fmb = fm;
		const float *bnd_in = bnd;
		float *bnd_out = bnd;
		float pfM = LZ, pfIX = LZ, pfJX = LZ, pfIY = LZ, pfJY = LZ; // 64 columns of row i0, one per lane
		float uM = LZ, uIX = LZ, uJX = LZ, uIY = LZ, uJY = LZ;      // row t*H at column j-1 (diagonal of r=0)
		float gIY = LZ, gJY = LZ;                                  // lane 0: row-0 chain (fwdflat3.cpp:81-93)
		int yprev = 0;
		for (int g = 0; g < G; ++g) {
			const int k = g - st; // macro-step of block b (k < M: the wave's next block starts P >= M later)
			if (b < NB && k >= 0) {
				if (k == 0) { // row block b: rows i0+1 .. i0+R
					i0 = b * R;
					T = ((LX - i0 < R ? LX - i0 : R) + H - 1) / H;
					nsteps = LY + T;
					fmb = fm + (u64)b * p.fm_block;
					bnd_in = bnd + (u64)(b > 0 ? b - 1 : 0) * 8 * ld; // row i0, written by block b-1
					bnd_out = bnd + (u64)b * 8 * ld;                   // row i0+R, for block b+1
					pfM = pfIX = pfJX = pfIY = pfJY = LZ;
#pragma unroll
					for (int r = 0; r < H; ++r) {
						const int i = i0 + t * H + r + 1;
						if (MEGA) {
							xl[MEGA ? r : 0] = (i <= LX) ? PX[i - 1] : 0ull;
							insx[r] = (i <= LX) ? IX[i - 1] : 0.0f; // fwdflat_mega.cpp:113
						} else {
							const int xc = (i <= LX) ? (int)X[i - 1] : 0;
							insx[r] = s_ins[xc];
							mrow[r] = xc * A;
						}
						cM[r] = cIX[r] = cJX[r] = cIY[r] = cJY[r] = LZ;
					}
					uM = uIX = uJX = uIY = uJY = LZ;
					gIY = gJY = LZ;
					yprev = 0;
					ylo_prev = 0; yhi_prev = 0; insy_prev = 0.0f;
				}
				const int s_end = (k + 1) * 64 < nsteps ? (k + 1) * 64 : nsteps;
				for (int s = k * 64; s < s_end; ++s) {
					const int j = s - t;
					// row t*H at column j comes from lane t-1's last row of the previous step
					float nM = mpc_lane_up1(cM[H - 1]);
					float nIX = mpc_lane_up1(cIX[H - 1]);
					float nJX = mpc_lane_up1(cJX[H - 1]);
					float nIY = mpc_lane_up1(cIY[H - 1]);
					float nJY = mpc_lane_up1(cJY[H - 1]);
					int yc = 0;
					u32 ylo = 0, yhi = 0;
					float insy;
					u32 yi[MEGA ? MPC_MEGA_FMAX : 1];
					if (MEGA) {
						ylo = (u32)mpc_lane_up1((int)ylo_prev);
						yhi = (u32)mpc_lane_up1((int)yhi_prev);
						insy = mpc_lane_up1(insy_prev);
						const bool incol = (s >= 1 && s <= LY);
						const u64 yload = incol ? PY[s - 1] : 0ull; // lane 0: column j = s
						const float iload = incol ? IY[s - 1] : 0.0f; // fwdflat_mega.cpp:120
						if (t == 0) { ylo = (u32)yload; yhi = (u32)(yload >> 32); insy = iload; }
#pragma unroll
						for (int f = 0; f < MPC_MEGA_FMAX; ++f)
							yi[f] = mg_base[f] + (((f < 4 ? ylo : yhi) >> (8 * (f & 3))) & 0xffu);
					} else {
						yc = mpc_lane_up1(yprev);
						const int yload = (s >= 1 && s <= LY) ? (int)Y[s - 1] : 0; // lane 0: letter of column j = s
						if (t == 0)
							yc = yload;
						insy = s_ins[yc];
					}
					if (b > 0) {
						// row i0, the last row of the block above, comes back from the line buffer: these 64 columns were finished
						// by step 64k+126 of block b-1, two macro-steps (and two barriers) ago
						if ((s & 63) == 0) {
							const int jj = s + t;
							const bool in = jj <= LY;
							pfM = in ? bnd_in[0 * ld + jj] : LZ; pfIX = in ? bnd_in[1 * ld + jj] : LZ; pfJX = in ? bnd_in[2 * ld + jj] : LZ;
							pfIY = in ? bnd_in[3 * ld + jj] : LZ; pfJY = in ? bnd_in[4 * ld + jj] : LZ;
						}
						const float bM = mpc_read_lane(pfM, s & 63), bIX = mpc_read_lane(pfIX, s & 63), bJX = mpc_read_lane(pfJX, s & 63);
						const float bIY = mpc_read_lane(pfIY, s & 63), bJY = mpc_read_lane(pfJY, s & 63);
						if (t == 0) { nM = bM; nIX = bIX; nJX = bJX; nIY = bIY; nJY = bJY; }
					} else
					if (t == 0) {
						// row 0 (fwdflat3.cpp:35-39, :44-45, :57-65, :81-93)
						nM = LZ; nIX = LZ; nJX = LZ;
						if (j <= 0) { nIY = LZ; nJY = LZ; }
						else if (j == 1) { nIY = tSI + insy; nJY = tSJ + insy; }
						else { nIY = gIY + tII + insy; nJY = gJY + tJJ + insy; }
						gIY = nIY; gJY = nJY;
					}
					float dM = uM, dIX = uIX, dJX = uJX, dIY = uIY, dJY = uJY; // (i-1, j-1)
					float upM = nM, upIX = nIX, upJX = nJX;                     // (i-1, j)
					float *fmrow = fmb + ((u64)s * H) * 64 + t;
#pragma unroll
					for (int r = 0; r < H; ++r) {
						const float oM = cM[r], oIX = cIX[r], oJX = cJX[r], oIY = cIY[r], oJY = cJY[r]; // (i, j-1)
						const float m = MEGA ? mpc_mega_match(s_match, mg_alpha, xl[MEGA ? r : 0], yi) // fwdflat_mega.cpp:121
						                     : s_match[mrow[r] + yc];
						// fwdflat3.cpp:116-145 (kernels_fb.h on the borders: the same expressions over LOG_ZERO neighbours)
						float vM = mpc_la5t(dM + tMM, dIX + tIM, dJX + tJM, dIY + tIM, dJY + tJM, s_coef) + m;
						float vIX = mpc_la2t(upIX + tII, upM + tMI, s_coef) + insx[r];
						float vJX = mpc_la2t(upJX + tJJ, upM + tMJ, s_coef) + insx[r];
						float vIY = mpc_la2t(oIY + tII, oM + tMI, s_coef) + insy;
						float vJY = mpc_la2t(oJY + tJJ, oM + tMJ, s_coef) + insy;
						if (r == 0) {
							const bool row1 = (t == 0) && (b == 0);
							if (row1 && j == 0) { vIX = tSI + insx[0]; vJX = tSJ + insx[0]; } // fwdflat3.cpp:42-43
							if (row1 && j == 1) vM = tSM + m;                                 // fwdflat3.cpp:111-112
						}
						cM[r] = vM; cIX[r] = vIX; cJX[r] = vJX; cIY[r] = vIY; cJY[r] = vJY;
						fmrow[r * 64] = vM;
						dM = oM; dIX = oIX; dJX = oJX; dIY = oIY; dJY = oJY;
						upM = vM; upIX = vIX; upJX = vJX;
					}
					uM = nM; uIX = nIX; uJX = nJX; uIY = nIY; uJY = nJY;
					yprev = yc;
					ylo_prev = ylo; yhi_prev = yhi; insy_prev = insy;
					if (b + 1 < NB && t == 63 && j >= 0 && j <= LY) { // row i0+R for the next block (column j = s-63)
						bnd_out[0 * ld + j] = cM[H - 1]; bnd_out[1 * ld + j] = cIX[H - 1]; bnd_out[2 * ld + j] = cJX[H - 1];
						bnd_out[3 * ld + j] = cIY[H - 1]; bnd_out[4 * ld + j] = cJY[H - 1];
					}
				}
				if (k == M - 1) { // the block is done
					if (b == NB - 1) {
						// F(LX,LY,*) sits in lane T-1, row (LX-1)%H, after its last step (column LY).
						float eM = LZ, eIX = LZ, eJX = LZ, eIY = LZ, eJY = LZ;
						const int rl = (LX - 1) % H;
#pragma unroll
						for (int r = 0; r < H; ++r)
							if (r == rl) { eM = cM[r]; eIX = cIX[r]; eJX = cJX[r]; eIY = cIY[r]; eJY = cJY[r]; }
						eM = __shfl(eM, T - 1); eIX = __shfl(eIX, T - 1); eJX = __shfl(eJX, T - 1);
						eIY = __shfl(eIY, T - 1); eJY = __shfl(eJY, T - 1);
						// totalprobflat.cpp:3-16 with B(LX,LY,*) = start scores (bwdflat3.cpp:53-61); state order
						// M, IX, IY, JX, JY (pairhmm.h:11-19), left fold from LOG_ZERO.
						float tot = LZ;
						tot = mpc_la2t(tot, eM + tSM, s_coef);
						tot = mpc_la2t(tot, eIX + tSI, s_coef);
						tot = mpc_la2t(tot, eIY + tSI, s_coef);
						tot = mpc_la2t(tot, eJX + tSJ, s_coef);
						tot = mpc_la2t(tot, eJY + tSJ, s_coef);
						if (t == 0) {
							p.total[pid] = tot;
							s_wg[1] = __float_as_uint(tot); // for the other waves, behind this macro-step's barrier (the last one)
						}
					}
					b += W; st += P;
				}
			}
			MPC_WAVE_FENCE(); // this macro-step's boundary-row (and forward-plane) stores, before the barrier that publishes them
			__syncthreads();
		}
		}
		const float total = __uint_as_float(mpc_wave_first(s_wg[1]));

		// ------------------------------------------------------------------ backward + posterior
		// Row i uses the emissions of x_{i+1}=X[i] and y_{j+1}=Y[j] (bwdflat3.cpp:46,64). Blocks bottom-up: position bb = NB-1-b.
		u64 *cand = p.cand + (u64)pid * p.capc;
		{
		const int M = (LY + 63 + 63) >> 6, P = M > 2 * W ? M : 2 * W;
		const int G = ((NB - 1) / W) * P + 2 * ((NB - 1) % W) + M;
		int bb = w, st = 2 * w;
		int b = 0, i0 = 0, bsteps = 0;
		const float *fmb = fm;
		const float *bnd_in = bnd;
		float *bnd_out = bnd;
		float pfM = LZ, pfIX = LZ, pfJX = LZ; // 64 columns of the row below the block, one per lane
		float gM = LZ;                        // row (t+1)*H+1 at column j+1: diagonal of r=H-1
		int ynext_prev = 0;
		for (int g = 0; g < G; ++g) {
			const int k = g - st;
			if (bb < NB && k >= 0) {
				if (k == 0) {
					b = NB - 1 - bb;
					i0 = b * R;
					T = ((LX - i0 < R ? LX - i0 : R) + H - 1) / H;
					bsteps = LY + T - 1;
					fmb = fm + (u64)b * p.fm_block;
					bnd_in = bnd + ((u64)b * 8 + 5) * ld;                   // row i0+R+1 (M, IX, JX), written by block b+1
					bnd_out = bnd + ((u64)(b > 0 ? b - 1 : 0) * 8 + 5) * ld; // row i0+1, for block b-1
					pfM = pfIX = pfJX = LZ;
#pragma unroll
					for (int r = 0; r < H; ++r) {
						const int i = i0 + t * H + r + 1;
						if (MEGA) {
							xl[MEGA ? r : 0] = (i < LX) ? PX[i] : 0ull;
							insx[r] = (i < LX) ? IX[i] : 0.0f; // bwdflat_mega.cpp:55
						} else {
							const int xc = (i < LX) ? (int)X[i] : 0;
							insx[r] = s_ins[xc];
							mrow[r] = xc * A;
						}
						cM[r] = cIX[r] = cJX[r] = cIY[r] = cJY[r] = LZ; // virtual column LY+1
					}
					gM = LZ;
					ynext_prev = 0;
					ylo_prev = 0; yhi_prev = 0; insy_prev = 0.0f;
				}
				const int s_end = (k + 1) * 64 < bsteps ? (k + 1) * 64 : bsteps;
				for (int s = k * 64; s < s_end; ++s) {
					const int j = LY - s + (T - 1 - t);
					// row (t+1)*H+1 at column j: lane t+1's first row from the previous step
					float nM = mpc_lane_down1(cM[0]);
					float nIX = mpc_lane_down1(cIX[0]);
					float nJX = mpc_lane_down1(cJX[0]);
					if (bb > 0) {
						// the first row of the block below comes back from the line buffer (lane 63 is at column LY - s): lane 0 of that
						// block wrote column j at its step LY+T'-1-j, these 64 columns by step 64k+126 at the latest
						if ((s & 63) == 0) {
							const int jj = LY - s - t;
							const bool in = jj >= 1;
							pfM = in ? bnd_in[0 * ld + jj] : LZ; pfIX = in ? bnd_in[1 * ld + jj] : LZ; pfJX = in ? bnd_in[2 * ld + jj] : LZ;
						}
						const float bM = mpc_read_lane(pfM, s & 63), bIX = mpc_read_lane(pfIX, s & 63), bJX = mpc_read_lane(pfJX, s & 63);
						if (t == 63) { nM = bM; nIX = bIX; nJX = bJX; }
					} else
					if (t == 63) { nM = LZ; nIX = LZ; nJX = LZ; } // nothing below the wave: virtual row
					const int jl = LY - s; // column of the leading lane T-1
					int yc = 0;
					u32 ylo = 0, yhi = 0;
					float insy;
					u32 yi[MEGA ? MPC_MEGA_FMAX : 1];
					if (MEGA) {
						ylo = (u32)mpc_lane_down1((int)ylo_prev);
						yhi = (u32)mpc_lane_down1((int)yhi_prev);
						insy = mpc_lane_down1(insy_prev);
						const bool incol = (jl >= 0 && jl < LY);
						const u64 yload = incol ? PY[jl] : 0ull;      // y_{j+1} of the leading lane's column
						const float iload = incol ? IY[jl] : 0.0f;    // bwdflat_mega.cpp:78
						if (t >= T - 1) { ylo = (u32)yload; yhi = (u32)(yload >> 32); insy = iload; }
#pragma unroll
						for (int f = 0; f < MPC_MEGA_FMAX; ++f)
							yi[f] = mg_base[f] + (((f < 4 ? ylo : yhi) >> (8 * (f & 3))) & 0xffu);
					} else {
						yc = mpc_lane_down1(ynext_prev);
						const int yload = (jl >= 0 && jl < LY) ? (int)Y[jl] : 0;
						if (t >= T - 1)
							yc = yload; // leading lane (and idle lanes beyond it)
						insy = s_ins[yc];
					}
					const int sf = j + t; // forward step that stored column j of this lane (uniform: LY-s+T-1)
					const float *fmrow = fmb + ((u64)(sf < 0 ? 0 : sf) * H) * 64 + t;
					float dgM = gM;                           // M(i+1, j+1)
					float dnIX = nIX, dnJX = nJX;             // (i+1, j)
					bool anyhit = false;
					float sc[H];
#pragma unroll
					for (int r = H - 1; r >= 0; --r) {
						const int i = i0 + t * H + r + 1;
						const float oM = cM[r], oIY = cIY[r], oJY = cJY[r]; // (i, j+1)
						// bwdflat3.cpp:75-79
						const float xM = dgM + (MEGA ? mpc_mega_match(s_match, mg_alpha, xl[MEGA ? r : 0], yi) // bwdflat_mega.cpp:79-80
						                             : s_match[mrow[r] + yc]);
						const float xIX = dnIX + insx[r];
						const float xJX = dnJX + insx[r];
						const float xIY = oIY + insy;
						const float xJY = oJY + insy;
						// bwdflat3.cpp:81-118 (interior; :132-176 fall out of the same expressions over LOG_ZERO virtual neighbours)
						float vM = mpc_la5t(tMM + xM, tMI + xIX, tMJ + xJX, tMI + xIY, tMJ + xJY, s_coef);
						float vIX = mpc_la2t(tII + xIX, tIM + xM, s_coef);
						float vJX = mpc_la2t(tJJ + xJX, tJM + xM, s_coef);
						float vIY = mpc_la2t(tII + xIY, tIM + xM, s_coef);
						float vJY = mpc_la2t(tJJ + xJY, tJM + xM, s_coef);
						if (i == LX && j == LY) { // bwdflat3.cpp:53-61
							vM = tSM; vIX = tSI; vIY = tSI; vJX = tSJ; vJY = tSJ;
						}
						// calcposteriorflat.cpp:14: Score = F_M + B_M - Total
						const float f = fmrow[r * 64];
						const float score = (f + vM) - total;
						sc[r] = score;
						anyhit = anyhit || ((i <= LX) && (j >= 1) && (j <= LY) && score >= p.thr);
						dgM = oM; // becomes M(i, j+1) = diagonal of row i-1
						cM[r] = vM; cIX[r] = vIX; cJX[r] = vJX; cIY[r] = vIY; cJY[r] = vJY;
						dnIX = vIX; dnJX = vJX;
					}
					gM = nM;
					ynext_prev = yc;
					ylo_prev = ylo; yhi_prev = yhi; insy_prev = insy;
					if (b > 0 && t == 0 && j >= 1 && j <= LY) { // row i0+1 for the block above
						bnd_out[0 * ld + j] = cM[0]; bnd_out[1 * ld + j] = cIX[0]; bnd_out[2 * ld + j] = cJX[0];
					}
					if (__ballot(anyhit)) {
						// the step's candidates: counted over its H rows, ONE add on the pair's counter in LDS, then written row by row
						u64 bal[H];
						u32 nhit = 0;
#pragma unroll
						for (int r = 0; r < H; ++r) {
							const int i = i0 + t * H + r + 1;
							const bool hit = (i <= LX) && (j >= 1) && (j <= LY) && (sc[r] >= p.thr);
							bal[r] = __ballot(hit);
							nhit += (u32)__popcll(bal[r]);
						}
						u32 pos0 = mpc_wave_first(atomicAdd(&s_wg[2], t == 0 ? nhit : 0u));
#pragma unroll
						for (int r = 0; r < H; ++r) {
							const int i = i0 + t * H + r + 1;
							const bool hit = (bal[r] >> t) & 1ull;
							const u32 pos = pos0 + (u32)__popcll(bal[r] & ((1ull << t) - 1ull));
							if (hit && pos < p.capc) {
								const u32 idx = ((u32)(i - 1) << MPC_KEY_ROW_SHIFT_LONG) | (u32)(j - 1);
								cand[pos] = ((u64)idx << 32) | (u64)__float_as_uint(sc[r]);
							}
							pos0 += (u32)__popcll(bal[r]);
						}
					}
				}
				if (k == M - 1) { bb += W; st += P; }
			}
			MPC_WAVE_FENCE();
			__syncthreads();
		}
		}
		if (w == 0 && t == 0)
			p.cand_cnt[pid] = s_wg[2]; // every wave's adds lie before the sweep's last barrier
		// (wave 0 resets the counter and the queue index at the top; the other waves read neither before the barrier there)
	}
}

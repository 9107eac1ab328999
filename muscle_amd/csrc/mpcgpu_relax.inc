// mpcgpu_relax.inc — host side of the consistency relax (part of mpcgpu.cpp's translation unit): LDS geometries, the band tile cutter
// and the launches of relax_var_kernel / relax_band_kernel (kernels_relaxv.h, kernels_relaxb.h). Reference: MPCFlat::ConsIter,
// consflat.cpp:5-23; ConsPair, conspairflat.cpp:10-110.
// ---- variable-size records + relax_var_kernel (kernels_relaxv.h) -------------------------------------------------------
// Two geometries. The primary one: two 1024-thread workgroups per CU (8 waves per SIMD, 64 VGPRs), 80 KB of LDS each (one
// workgroup's staging overlaps the other's merges), 13 cells per lane. With 14 the compiler keeps five row-offset registers in
// spill slots and reloads them inside the walk (each reload waits for vmcnt(0)); 13 has none, and although 2 600 more 4x4 tiles
// then split into 4x2 the two iterations at 1000 x L~400 take 1171 ms against 1195 (12: 1282, most tiles split) — profiles/r05g.
// The fallback, for the pairs whose records or cells do not fit that: one 1024-thread workgroup per CU with the CU's 160 KB and
// 16 cells per lane (second launch). Either has ONE staging buffer after the pair table. (Measured and removed: two 512- or
// 768-thread workgroups per CU, one 1024-thread workgroup with two staging buffers — docs/HISTORY.md, profiles/r02e, r03b, r04a.)
u32 var_max_slots(bool fallback) { return fallback ? 16u : 13u; }
// bytes of the staging buffer. MPCGPU_RELAX_LDS_KB: tests shrink the budget to reach tile splitting with short sequences (_1024: the fallback alone)
u32 var_buf_bytes(bool fallback)
{
	const u64 lds_cap = (u64)(fallback ? env_int("MPCGPU_RELAX_LDS_KB_1024", env_int("MPCGPU_RELAX_LDS_KB", 160)) : env_int("MPCGPU_RELAX_LDS_KB", 80)) * 1024;
	return (u32)((lds_cap - MPC_RV_TAB_BYTES) & ~15ull);
}

// the instantiation a launch runs: its address (attributes, occupancy), launched when `go`
template <int SL, int WGS, int DG = 0> const void *relax_var_go(bool go, const RelaxVarParams &rp, u32 grid, size_t smem, hipStream_t st)
{
	if (go) MPC_LAUNCH((relax_var_kernel<1024, SL, WGS, DG>), grid, 1024, smem, st, rp);
	return (const void *)relax_var_kernel<1024, SL, WGS, DG>;
}

// launches relax_var_kernel of the primary geometry or the fallback over a tile list; `report`: the launch names the kernel in
// relax_info (and may be a measurement kernel)
static int relax_var_launch(mpcgpu_ctx *c, const StoreParams &sp, u64 k0, u64 k1, bool fallback, const DevBuf &d_tiles, u32 ntiles, bool report)
{
	const u32 buf_bytes = var_buf_bytes(fallback);
	const size_t smem = MPC_RV_TAB_BYTES + (size_t)buf_bytes;
	RelaxVarParams rp;
	rp.s = sp; rp.tiles = d_tiles.as<u32>(); rp.ntiles = ntiles;
	rp.k0 = k0; rp.k1 = k1;
	rp.tile_next = c->d_tile_next.as<u32>() + (fallback ? 8 : 0);
	// MPCGPU_RELAX_DIAG=1|2|3 (staging only / merges only / merges + barriers): measurement kernels whose results are WRONG by design;
	// they exist only in a library built with -DMPC_RELAX_DIAG_BUILD (make diag), which also says so on stderr at every launch
	int diag = report ? env_int("MPCGPU_RELAX_DIAG", 0) : 0;
#ifndef MPC_RELAX_DIAG_BUILD
	if (diag) return fail(c, "MPCGPU_RELAX_DIAG needs a library built with -DMPC_RELAX_DIAG_BUILD (measurement kernels: wrong results by design)");
#else
	if (diag) { fprintf(stderr, "[mpcgpu] WARNING: MPCGPU_RELAX_DIAG=%d: measurement kernel, the relax results are WRONG by design\n", diag); c->relax_fallback = true; }
#endif
	if (fallback) diag = 0; // (the measurement kernels are of the primary geometry)
	u32 grid = 1;
	auto go = [&](bool launch) -> const void * {
		if (fallback) return relax_var_go<16, 1>(launch, rp, grid, smem, c->stream);
#ifdef MPC_RELAX_DIAG_BUILD
		if (diag == 1) return relax_var_go<13, 2, 1>(launch, rp, grid, smem, c->stream);
		if (diag == 2) return relax_var_go<13, 2, 2>(launch, rp, grid, smem, c->stream);
		if (diag) return relax_var_go<13, 2, 3>(launch, rp, grid, smem, c->stream);
#endif
		return relax_var_go<13, 2>(launch, rp, grid, smem, c->stream);
	};
	const void *fn = go(false);
	HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
	if (report) {
		char kn[128];
		snprintf(kn, sizeof(kn), "relax_var_kernel<1024, %u, %d, %d, MpcRvBlocksAsm>", var_max_slots(fallback), fallback ? 1 : 2, diag);
		c->relax_kernel_name = kn;
	}
	int occ = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 1024, smem) != hipSuccess || occ < 1) occ = 1;
	grid = std::max(std::min<u32>(rp.ntiles, (u32)c->prop.multiProcessorCount * (u32)occ), 1u);
	if (trace_on()) {
		fprintf(stderr, "[mpcgpu] relax var: tiles=%u %s buf=%u B lds=%zu B occ=%d grid=%u max_nnz=%u\n", rp.ntiles, fallback ? "fallback" : "primary", buf_bytes, smem, occ, grid, c->max_nnz);
		fflush(stderr);
	}
	TimedSpan ts;
	if (span_begin(c, 3, &ts)) return 1;
	go(true);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts)) return 1;
	return 0;
}

// ---- band tiles + relax_band_kernel (kernels_relaxb.h) ---------------------------------------------------------------------
#ifdef MPC_RELAX_DIAG_BUILD
#define MPC_RB_DIAG_CASES(TH, SL) \
	if (diag == 1) { fn = (const void *)relax_band_kernel<TH, SL, 2, 1>; if (go) MPC_LAUNCH((relax_band_kernel<TH, SL, 2, 1>), grid, TH, smem, c->stream, rp); } \
	else if (diag == 2) { fn = (const void *)relax_band_kernel<TH, SL, 2, 2>; if (go) MPC_LAUNCH((relax_band_kernel<TH, SL, 2, 2>), grid, TH, smem, c->stream, rp); } \
	else if (diag == 3) { fn = (const void *)relax_band_kernel<TH, SL, 2, 3>; if (go) MPC_LAUNCH((relax_band_kernel<TH, SL, 2, 3>), grid, TH, smem, c->stream, rp); } \
	else if (diag == 4) { fn = (const void *)relax_band_kernel<TH, SL, 2, 4>; if (go) MPC_LAUNCH((relax_band_kernel<TH, SL, 2, 4>), grid, TH, smem, c->stream, rp); } \
	else
#else
#define MPC_RB_DIAG_CASES(TH, SL)
#endif
constexpr u32 kBandSlotsWin = 15; // cells per lane of the direct-index merge (its two-word descriptor sets became one word each: registers for two more cells)
constexpr u32 kBandThreads = 1024, kBandSlots = 13; // two 1024-thread workgroups per CU (8 waves per SIMD, 64 VGPRs), 13 cells per lane (14: spill reloads inside the walk, and every reload waits for vmcnt(0) - the prefetch)

// 0 = launched (or nothing to do), 1 = error, 2 = not for band tiles (the caller runs relax_var)
int relax_band(mpcgpu_ctx *c, const StoreParams &sp, u64 k0, u64 k1)
{
	const u32 n = c->n, nb1 = c->band_nb1;
	// geometry: two 1024-thread workgroups per CU, 80 KB of LDS each (kBandThreads). (Measured and removed: four 512-thread workgroups
	// per CU with 40 KB each, whose barriers hold 8 waves instead of 16: 9.6 of 13 cells per lane at 1000 x L~400, and 2472 against
	// 1545 ms per two iterations on rdrp-500 — profiles/r06g, r10a)
	// (measured and removed again, profiles/r10a_rdrp_geometry_sweep.log: ONE 1024-thread workgroup per CU with the CU's 160 KB and 26 cells per
	// lane — 8x4 bands, 10.7 cells per lane, every step prefetched, 6.6 B per cell-step instead of 11.7 — is 18 % SLOWER on real data
	// (rdrp-500: 1818 against 1545 ms per two iterations): the walk's merges are chains of dependent LDS reads and want 8 waves per SIMD)
	const u32 lds_bytes = (u32)std::max(env_int("MPCGPU_RELAX_LDS_KB", 80), 3) * 1024u;
	const u32 cap = (lds_bytes - MPC_RB_TAB_BYTES) & ~15u, cap_blocks = cap / 16;
	const u32 cus = (u32)c->prop.multiProcessorCount;
	// the direct-index merge (window records for the Y operand) where the store has them; the measurement kernels exist for the
	// block walk only
	const bool use_win = c->win_ok && !env_int("MPCGPU_RELAX_DIAG", 0);
	const u32 kernel_slots = use_win ? kBandSlotsWin : kBandSlots;
	const u32 max_slots = (u32)std::min<int>(std::max(env_int("MPCGPU_RELAX_SLOTS", (int)kernel_slots), 1), (int)kernel_slots);
	if (c->btiles_k0 != k0 || c->btiles_k1 != k1) {
		c->btiles_k0 = c->btiles_k1 = ~0ull;
		const auto t_cut0 = std::chrono::steady_clock::now();
		auto lap_ms = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_cut0).count(); };
		RbTileTabs tb;
		tb.cell_off = c->d_cell_off.as<u32>(); tb.yr = c->d_yr.as<u32>(); tb.ovf_sum = c->d_ovf_sum.as<u32>(); tb.ovf_maxc = c->d_ovf_maxc.as<u32>();
		tb.nb1 = nb1; tb.threads = kBandThreads; tb.k0 = k0; tb.k1 = k1;
		tb.win = use_win ? 1u : 0u;
		tb.ysum = use_win ? c->d_wsum.as<u32>() : tb.ovf_sum; tb.ymaxc = use_win ? c->d_wmaxc.as<u32>() : tb.ovf_maxc;
		// tile words of a list of tiles whose words 0..5 are set: Y ranges, first-piece blocks, slots; out: slots, mean blocks, bound, cells
		auto eval_tiles = [&](std::vector<u32> &words, std::vector<u32> &out) -> int {
			const u32 nt = (u32)(words.size() / MPC_RB_TILE_WORDS);
			out.assign((size_t)nt * 4, 0u);
			if (!nt) return 0;
			if (upload(c, c->d_btiles, words)) return 1;
			HIPCHK(c, c->d_bt_out.ensure((size_t)nt * 16));
			MPC_LAUNCH(band_eval_kernel, std::min<u32>(nt, cus * 32), 64, 0, c->stream, sp, tb, c->d_btiles.as<u32>(), nt, c->d_bt_out.as<u32>());
			HIPCHK(c, hipGetLastError());
			HIPCHK(c, hipMemcpyAsync(words.data(), c->d_btiles.p, words.size() * 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(c, hipMemcpyAsync(out.data(), c->d_bt_out.p, out.size() * 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(c, hipStreamSynchronize(c->stream));
			return 0;
		};
		auto pair_index = [&](u32 X, u32 Y) -> u64 { return (u64)X * n - ((u64)X * (X + 1)) / 2 + (Y - X - 1); }; // InitPairs order (mpcflat.cpp:145-155), X < Y
		// does the block of sequences [x0, x0+cx) x [y0, y0+cy) hold a pair whose position may lie in [k0, k1)? (a conservative test: the
		// kernels check every pair's own position)
		auto block_in_range = [&](u32 x0, u32 cx, u32 y0, u32 cy) -> bool {
			if (c->order_rects.empty()) {
				// InitPairs order: pair indices grow with X first — the block's pairs lie between its first row's first and its last row's last pair
				const u32 xl = std::min(x0 + cx - 1, y0 + cy - 2);
				return !(pair_index(x0, std::max(y0, x0 + 1)) >= k1 || pair_index(xl, y0 + cy - 1) < k0);
			}
			for (size_t r = 0; r < c->order_rects.size() / 4; ++r) { // block order: the rectangles whose positions meet [k0, k1) and whose sequences meet the block's
				const u32 *q = &c->order_rects[4 * r];
				const u64 cnt = q[2] >= q[1] ? (u64)(q[1] - q[0]) * (q[3] - q[2]) : (u64)(q[1] - q[0]) * (q[1] - q[0] - 1) / 2;
				if (c->order_base[r] >= k1 || c->order_base[r] + cnt <= k0) continue;
				if (x0 < q[1] && x0 + cx > q[0] && y0 < q[3] && y0 + cy > q[2]) return true;
			}
			return false;
		};
		u64 last_cut_candidates = 0; // super-tiles with cells in the last cut
		// super-tiles of nx x ny sequences cut into row bands of <= max_slots cells per lane and <= target blocks per step (mean)
		// stride > 1: every stride-th super-tile only — a SAMPLE of the cut, for pricing a shape (the search below)
		auto cut = [&](u32 nx, u32 ny, u32 target, std::vector<u32> &words, std::vector<u32> &out, u32 stride = 1) -> int {
			std::vector<u32> cand;
			const u32 nbx = (n + nx - 1) / nx, nby = (n + ny - 1) / ny;
			u64 seen = 0;
			for (u32 xb = 0; xb < nbx; ++xb)
				for (u32 yb = 0; yb < nby; ++yb) {
					const u32 x0 = xb * nx, cx = std::min(nx, n - x0), y0 = yb * ny, cy = std::min(ny, n - y0);
					if (y0 + cy <= x0 + 1) continue; // no pair X < Y in this block
					// a rank of a sharded run relaxes [k0, k1) only: blocks whose pairs all lie outside that range are not candidates
					if (!block_in_range(x0, cx, y0, cy)) continue;
					if (seen++ % stride) continue;
					cand.insert(cand.end(), {x0, cx, y0, cy});
				}
			const u32 nc = (u32)(cand.size() / 4);
			words.clear();
			if (!nc) { out.clear(); return 0; }
			// The cut's small inputs and outputs (candidates in, bands per candidate out, list bases in) live in ONE page-locked record that
			// the kernels read and write in place: three transfers and a wait fewer per cut. (The FIRST wait of a cut ends 16 - 27 ms late in
			// some processes, every or every other step, whatever is queued first — copy or kernel, polled or blocking wait; not under
			// rocprofv3, not with torch initialised before the context: profiles/r10k_rank_time.log. Not understood, not fixed by this.)
			HIPCHK(c, c->h_bt.ensure(cand.size() * 4 + (size_t)nc * 8));
			u32 *cnt = c->h_bt.as<u32>(), *base = cnt + nc, *hcand = base + nc; // [cnt nc][base nc][cand 4 nc]
			memcpy(hcand, cand.data(), cand.size() * 4);
			const u32 grid = std::min<u32>(nc, cus * 32);
			MPC_LAUNCH(band_cut_kernel, grid, 64, (size_t)(nb1 + 1) * 8, c->stream, sp, tb, (const u32 *)hcand, nc, max_slots, target, 0, cnt,
				(const u32 *)nullptr, (u32 *)nullptr);
			HIPCHK(c, hipGetLastError());
			HIPCHK(c, hipStreamSynchronize(c->stream));
			u64 tot = 0;
			last_cut_candidates = 0;
			for (u32 q = 0; q < nc; ++q) { base[q] = (u32)tot; tot += cnt[q]; last_cut_candidates += cnt[q] ? 1 : 0; }
			if (tot > 0x7fffffffull / MPC_RB_TILE_WORDS) return fail(c, "mpcgpu_cons_iter: too many band tiles");
			words.assign((size_t)tot * MPC_RB_TILE_WORDS, 0u);
			if (!tot) { out.clear(); return 0; }

			HIPCHK(c, c->d_btiles.ensure(words.size() * 4));
			MPC_LAUNCH(band_cut_kernel, grid, 64, (size_t)(nb1 + 1) * 8, c->stream, sp, tb, (const u32 *)hcand, nc, max_slots, target, 1, (u32 *)nullptr,
				(const u32 *)base, c->d_btiles.as<u32>());
			HIPCHK(c, hipGetLastError());
			HIPCHK(c, hipMemcpyAsync(words.data(), c->d_btiles.p, words.size() * 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(c, hipStreamSynchronize(c->stream)); // (the tile words are read back before eval_tiles below reuses them)
			return eval_tiles(words, out);
		};
	struct Score { double fill, bytes_per_cell, in_target; u64 tiles; };
		auto score = [&](const std::vector<u32> &out, u32 target) {
			Score sc = {0, 0, 0, out.size() / 4};
			u64 cells = 0, est = 0, ok = 0;
			for (size_t t = 0; t + 3 < out.size(); t += 4) { cells += out[t + 3]; est += out[t + 1]; ok += out[t + 1] <= target ? 1 : 0; }
			if (sc.tiles) { sc.fill = (double)cells / ((double)sc.tiles * max_slots * kBandThreads); sc.in_target = (double)ok / (double)sc.tiles; }
			sc.bytes_per_cell = cells ? 16.0 * (double)est / (double)cells : 0.0;
			return sc;
		};
		// Shape of the super-tiles and the target the bands are cut to. MPCGPU_RELAX_SHAPE=nx,ny[,kb]: forced.
		// Narrow rows (1000 x L~400: 2 cells per row, y ranges that follow the diagonal): 8x8 super-tiles whose steps leave room for
		// the next step beside the current one fill the register slots — taken at once. Otherwise (real data: 7 cells per row, the
		// cells of 50 rows spread over 200 rows of the partner, and steps that vary by a factor of 1.6 around their mean) every
		// shape of the menu is cut in both modes and priced: a tile-step costs a fixed part (staging block, barrier; plus the exposed
		// transfer when the next step cannot be prefetched) and a part per cell slot. Shapes with more X than Y sequences are on the
		// menu because the X pieces are the band's rows only, the Y pieces the whole range those rows' cells reach.
		static const u32 menu[10][2] = {{8, 8}, {8, 4}, {8, 2}, {8, 1}, {4, 4}, {4, 2}, {4, 1}, {2, 2}, {2, 1}, {1, 1}};
		std::vector<u32> &words = c->v_words, &out = c->v_out; // (kept: see mpcgpu_ctx)
		words.clear(); out.clear();
		u32 use_nx = 0, use_ny = 0, use_target = 0;
		const u32 margin = std::min<u32>(cap_blocks / 16, 64); // blocks: steps vary around the mean
		const u32 half = cap_blocks / 2 > margin ? cap_blocks / 2 - margin : cap_blocks / 2, full = cap_blocks > 2 * margin ? cap_blocks - 2 * margin : cap_blocks;
		if (const char *sh = getenv("MPCGPU_RELAX_SHAPE")) {
			unsigned a = 0, b = 0, kb = 0;
			const int got = sscanf(sh, "%u,%u,%u", &a, &b, &kb);
			if (got >= 2 && a >= 1 && a <= MPC_RB_MAXN && b >= 1 && b <= MPC_RB_MAXN) {
				use_nx = a; use_ny = b; use_target = got == 3 && kb ? std::min<u32>(kb * 64, cap_blocks) : half;
				if (cut(use_nx, use_ny, use_target, words, out)) return 1;
			}
		}
		if (!use_nx && n <= 64) {
			// few sequences (the shrubs of -super7, the clusters of -super5): the 8 x 8 super-tiles with ALL their rows as one band
			// each, evaluated in one pass; taken when every one of them fits the cell slots and leaves room for the next step
			std::vector<u32> &w2 = c->v_w2, &o2 = c->v_o2; // (kept: see mpcgpu_ctx)
			w2.clear(); o2.clear();
			for (u32 x0 = 0; x0 < n; x0 += 8)
				for (u32 y0 = x0; y0 < n; y0 += 8) {
					u32 nw[MPC_RB_TILE_WORDS] = {x0, std::min(8u, n - x0), y0, std::min(8u, n - y0), 0u, (nb1 - 1) * (u32)MPC_RB_HB};
					if (y0 + nw[3] > x0 + 1) w2.insert(w2.end(), nw, nw + MPC_RB_TILE_WORDS);
				}
			if (eval_tiles(w2, o2)) return 1;
			bool ok = !w2.empty();
			for (size_t t = 0; t + 3 < o2.size(); t += 4) ok = ok && o2[t] <= max_slots && o2[t + 1] <= half;
			if (ok) { words.swap(w2); out.swap(o2); use_nx = 8; use_ny = 8; use_target = half; }
		}
		if (!use_nx) {
			if (cut(8, 8, half, words, out)) return 1;
			const Score sc = score(out, half);
			if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles 8x8, two steps resident: %llu tiles, fill %.2f, %.2f B/cell-step, %.0f %% within target\n",
				(unsigned long long)sc.tiles, sc.fill, sc.bytes_per_cell, 100 * sc.in_target);
			if (!sc.tiles) { c->h_btiles.clear(); c->btiles_k0 = k0; c->btiles_k1 = k1; return 0; } // no cell in [k0,k1)
			if (sc.fill >= 0.70 && sc.in_target >= 0.90) { use_nx = 8; use_ny = 8; use_target = half; }
			// few cells (the shrubs of -super7: 32 sequences): nothing was cut — one band per super-tile — so no other shape or target
			// gives fewer tile-steps, and the search below (20 more cuts) is skipped
			else if (sc.in_target >= 1.0 && sc.tiles == last_cut_candidates) { use_nx = 8; use_ny = 8; use_target = half; }
		}
		if (!use_nx) {
			// worst step / mean step of this data set: the exact worst steps of a sample of 4x2 tiles cut to the whole area (95th percentile)
			double r95 = 1.0;
			{
				if (cut(4, 2, full, words, out, (u64)((n + 7) / 8) * ((n + 7) / 8) / 2 >= 4096 ? 8u : 1u)) return 1; // (a sample of a sample where there are thousands of super-tiles)
				const u32 nt = (u32)(words.size() / MPC_RB_TILE_WORDS);
				std::vector<u32> sample;
				const u32 stride = std::max(nt / 4096u, 1u);
				for (u32 t = 0; t < nt; t += stride) if (out[4 * t + 3]) sample.push_back(t);
				if (!sample.empty()) {
					if (upload(c, c->d_btiles, words) || upload(c, c->d_bt_list, sample)) return 1;
					HIPCHK(c, c->d_bt_count.ensure(sample.size() * 4));
					MPC_LAUNCH(band_fit_kernel, std::min<u32>(((u32)sample.size() + 3u) / 4u, cus * 8), 256, 0, c->stream, sp, c->d_ovf_off.as<u32>(), nb1,
						c->d_btiles.as<u32>(), c->d_bt_list.as<u32>(), (u32)sample.size(), c->d_bt_count.as<u32>(), tb.win);
					HIPCHK(c, hipGetLastError());
					std::vector<u32> worst(sample.size());
					HIPCHK(c, hipMemcpyAsync(worst.data(), c->d_bt_count.p, sample.size() * 4, hipMemcpyDeviceToHost, c->stream));
					HIPCHK(c, hipStreamSynchronize(c->stream));
					std::vector<double> ratio;
					for (size_t q = 0; q < sample.size(); ++q) if (out[4 * sample[q] + 1]) ratio.push_back((double)worst[q] / (double)out[4 * sample[q] + 1]);
					if (!ratio.empty()) { std::sort(ratio.begin(), ratio.end()); r95 = std::max(ratio[std::min(ratio.size() - 1, (size_t)(0.95 * (double)ratio.size()))], 1.0); }
				}
			}
			const u32 single = std::max(std::min((u32)((double)cap_blocks / r95 * 0.98), full), 1u); // mean step such that the worst one still fits
			// cost of a tile-step in units of one cell slot of this data (a slot's merges grow with the rows' entries)
			// cost of a tile-step in units of one cell slot of this data (a slot's merges grow with the rows' entries)
			// (Round 6, measured and not kept — profiles/r14a_cut_priced.log, r14b: pricing the BANDS the same way inside band_cut_kernel,
			// i.e. closing a band at the prefix with the lowest (fixed + slots of its busiest wave) per cell instead of the longest that
			// fits, brings the busiest wave from 3.55 to 3.23 slots at 2.9 instead of 3.0 cells per lane on rdrp-1000 4x2 tiles — and
			// the relax from 12 052 to 12 120 ms per two iterations; left to choose the shape as well it takes 2x2 tiles: 12 276 ms. The
			// slots a wave waits at the barrier for are not lost: the CU's other workgroup issues in them.)
			u64 rows = 0;
			for (u32 i = 0; i + 1 < n; ++i) rows += (u64)c->len[i] * (n - 1 - i);
			const double per_row = rows ? (double)c->total_entries / (double)rows : 2.0;
			const double slot_us = 0.3 + 0.2 * per_row, fixed = 1.0 / slot_us, exposed = 1.5 / slot_us;
			if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles: %.1f cells per row; worst step / mean step = %.3f (95th percentile): one step resident = %u blocks mean\n", per_row, r95, single);
			double best = 0;
			bool have = false;
			std::vector<u32> &w2 = c->v_w2, &o2 = c->v_o2; // (kept: see mpcgpu_ctx)
			w2.clear(); o2.clear();
			// Round 6: the twenty cuts of the search are PRICED on every 8th super-tile when there are thousands of them (the cost is a
			// sum over tiles: an eighth of them, evenly spread, ranks the shapes the same), and only the winner is cut in full — on the
			// first 1000 rdrp records the search was 0.47 s of a 13.4 s step (44 launches of band_cut_kernel = 0.17 s, the rest host work
			// on 450 000 tiles x 21 cuts): profiles/r13a_kernel_stats_rdrp1000.csv
			const u32 price_stride = (u64)((n + 7) / 8) * ((n + 7) / 8) / 2 >= 4096 ? 8u : 1u;
			for (u32 mode = 0; mode < 2; ++mode)
				for (u32 m = 0; m < 10; ++m) {
					const u32 target = mode == 0 ? half : single;
					if (cut(menu[m][0], menu[m][1], target, w2, o2, price_stride)) return 1;
					u64 slots = 0, over = 0;
					const u64 nt = o2.size() / 4;
					for (size_t t = 0; t + 3 < o2.size(); t += 4) { slots += std::min(o2[t], max_slots); over += o2[t + 1] > target ? 1 : 0; }
					if (!nt) continue;
					// tiles over the target (single index bands that do not fit) will be split by sequences: charged double
					const double cost = ((double)nt + (double)over) * (fixed + (mode ? exposed : 0.0)) + (double)slots;
					if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles %ux%u, %s: %llu tiles (%llu over the target), %.1f cells per lane, cost %.3g\n",
						menu[m][0], menu[m][1], mode ? "one step resident" : "two steps resident", (unsigned long long)nt, (unsigned long long)over,
						(double)slots / (double)nt, cost);
					if (!have || cost < best) { have = true; best = cost; words.swap(w2); out.swap(o2); use_nx = menu[m][0]; use_ny = menu[m][1]; use_target = target; }
				}
			if (!have) { c->h_btiles.clear(); c->btiles_k0 = k0; c->btiles_k1 = k1; return 0; }
			if (price_stride > 1 && cut(use_nx, use_ny, use_target, words, out)) return 1; // the winner, in full
		}
		// every tile must fit: cells per lane, 16-bit first-piece offsets, and its WORST step in the staging area (upper bound
		// first; the exact maximum over Z only where the bound does not settle it). What does not fit is halved: band, then Y, then X.
		std::vector<u32> &okw = c->v_okw;
		okw.clear();
		u64 nsplit = 0;
		if (!words.empty() && upload(c, c->d_btiles, words)) return 1; // (the device copy is that of the last shape tried)
		for (int round = 0; round < 24 && !words.empty(); ++round) {
			const u32 nt = (u32)(words.size() / MPC_RB_TILE_WORDS);
			std::vector<u32> need, exact;
			for (u32 t = 0; t < nt; ++t)
				if (out[4 * t] <= max_slots && words[(size_t)t * MPC_RB_TILE_WORDS + 6] <= MPC_RB_MAXFIRST && out[4 * t + 2] > cap_blocks) need.push_back(t);
			if (!need.empty()) {
				if (trace_on()) {
					u64 bsum = 0, esum = 0;
					for (u32 t : need) { bsum += out[4 * t + 2]; esum += out[4 * t + 1]; }
					fprintf(stderr, "[mpcgpu] band tiles: %zu of %u tiles need the exact worst step (mean bound %.0f blocks, mean step %.0f, area %u)\n",
						need.size(), nt, (double)bsum / need.size(), (double)esum / need.size(), cap_blocks);
				}
				if (upload(c, c->d_bt_list, need)) return 1;
				HIPCHK(c, c->d_bt_count.ensure(need.size() * 4));
				MPC_LAUNCH(band_fit_kernel, std::min<u32>(((u32)need.size() + 3u) / 4u, cus * 8), 256, 0, c->stream, sp, c->d_ovf_off.as<u32>(), nb1,
					c->d_btiles.as<u32>(), c->d_bt_list.as<u32>(), (u32)need.size(), c->d_bt_count.as<u32>(), tb.win);
				HIPCHK(c, hipGetLastError());
				exact.resize(need.size());
				HIPCHK(c, hipMemcpyAsync(exact.data(), c->d_bt_count.p, need.size() * 4, hipMemcpyDeviceToHost, c->stream));
				HIPCHK(c, hipStreamSynchronize(c->stream));
				for (size_t q = 0; q < need.size(); ++q) out[4 * need[q] + 2] = exact[q]; // the bound becomes the exact worst step
			}
			std::vector<u32> next;
			for (u32 t = 0; t < nt; ++t) {
				const u32 *w = &words[(size_t)t * MPC_RB_TILE_WORDS];
				if (out[4 * t + 3] == 0) continue; // no cell
				if (out[4 * t] <= max_slots && w[6] <= MPC_RB_MAXFIRST && out[4 * t + 2] <= cap_blocks) { okw.insert(okw.end(), w, w + MPC_RB_TILE_WORDS); continue; }
				++nsplit;
				auto push = [&](u32 x0, u32 nx, u32 y0, u32 ny, u32 r0, u32 r1) {
					u32 nw[MPC_RB_TILE_WORDS] = {x0, nx, y0, ny, r0, r1};
					next.insert(next.end(), nw, nw + MPC_RB_TILE_WORDS);
				};
				const u32 x0 = w[0], nx = w[1], y0 = w[2], ny = w[3], r0 = w[4], r1 = w[5];
				const u32 hb = (r1 - r0) / MPC_RB_HB;
				if (hb > 1) { const u32 mid = r0 + (hb / 2) * MPC_RB_HB; push(x0, nx, y0, ny, r0, mid); push(x0, nx, y0, ny, mid, r1); }
				else if (ny > 1) { push(x0, nx, y0, ny / 2, r0, r1); push(x0, nx, y0 + ny / 2, ny - ny / 2, r0, r1); }
				else if (nx > 1) { push(x0, nx / 2, y0, ny, r0, r1); push(x0 + nx / 2, nx - nx / 2, y0, ny, r0, r1); }
				else {
					if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles: rows [%u,%u) of pair (%u,%u) do not fit (slots %u, first %u, worst step %u blocks of %u)\n",
						r0, r1, x0, y0, out[4 * t], w[6], out[4 * t + 2], cap_blocks);
					return 2;
				}
			}
			words.swap(next);
			if (eval_tiles(words, out)) return 1;
		}
		if (!words.empty()) return 2;
		u64 ntail_split = 0;
		{
			// The tail of the launch: the kernel deals the list to the 8 XCDs in contiguous chunks (a counter each), and a chunk's
			// LAST tiles — one per resident workgroup of the XCD — are the ones that finish alone. They are cut in two by rows (any
			// part of a tile is a valid tile): half the tail, which is one tile of ~62 per workgroup on one GPU and one of ~8 on a rank
			// of eight (profiles/r12c: 109.4 -> 107.1 ms per rank of 8, 792.2 -> 791.0 ms on one GPU).
			const u32 W = MPC_RB_TILE_WORDS;
			const size_t nt = okw.size() / W;
			const u32 per_xcd = std::max(cus * 2u / 8u, 1u); // resident workgroups of an XCD (two per CU)
			if (nt >= (size_t)per_xcd * 8u * 3u) {
				const size_t chunk = (nt + 7) / 8;
				std::vector<u32> split;
				split.reserve(okw.size() + (size_t)per_xcd * 8u * W);
				for (size_t c0 = 0; c0 < nt; c0 += chunk) {
					const size_t c1 = std::min(c0 + chunk, nt), body = c1 - c0 > per_xcd ? c1 - per_xcd : c0;
					split.insert(split.end(), okw.begin() + c0 * W, okw.begin() + body * W);
					for (size_t t = body; t < c1; ++t) {
						const u32 *w = &okw[t * W];
						const u32 hb = (w[5] - w[4] + MPC_RB_HB - 1) / MPC_RB_HB;
						if (hb < 2) { split.insert(split.end(), w, w + W); continue; }
						const u32 mid = w[4] + (hb / 2) * MPC_RB_HB;
						u32 a[MPC_RB_TILE_WORDS] = {w[0], w[1], w[2], w[3], w[4], mid}, b[MPC_RB_TILE_WORDS] = {w[0], w[1], w[2], w[3], mid, w[5]};
						split.insert(split.end(), a, a + W);
						split.insert(split.end(), b, b + W);
						++ntail_split;
					}
				}
				okw.swap(split);
			}
		}
		{
			u64 cells = 0, est = 0;
			std::vector<u32> &o2 = c->v_o2, &w2 = c->v_w2; // (kept: see mpcgpu_ctx)
			w2 = okw;
			if (eval_tiles(w2, o2)) return 1; // (fills words 6.. of the halves; also leaves the final list's statistics for the description)
			if (ntail_split) { // halves without a cell go; the others are tiles like any other
				okw.clear();
				for (size_t t = 0; t < w2.size() / MPC_RB_TILE_WORDS; ++t)
					if (o2[4 * t + 3]) okw.insert(okw.end(), w2.begin() + t * MPC_RB_TILE_WORDS, w2.begin() + (t + 1) * MPC_RB_TILE_WORDS);
			}
			u64 slots = 0;
			for (size_t t = 0; t + 3 < o2.size(); t += 4) { cells += o2[t + 3]; est += o2[t + 1]; slots += o2[t + 3] ? o2[t] : 0u; }
			const size_t nt = okw.size() / MPC_RB_TILE_WORDS;
			char b[384];
			snprintf(b, sizeof(b), "%zu band tiles of <= %ux%u pairs (%llu split), target %u B per step of %u B staging (%s), mean step %.0f B, %.1f of %u cells per lane (%.2f slots on the busiest wave), %.2f B per cell-step",
				nt, use_nx, use_ny, (unsigned long long)nsplit, use_target * 16, cap, use_target <= cap_blocks / 2 ? "two steps resident" : "one step resident",
				nt ? 16.0 * (double)est / (double)nt : 0.0, nt ? (double)cells / ((double)nt * kBandThreads) : 0.0, max_slots, nt ? (double)slots / (double)nt : 0.0, cells ? 16.0 * (double)est / (double)cells : 0.0);
			c->tiles_desc = b;
		}
		c->h_btiles.swap(okw);
		if (trace_on() && (trace_level() & 2))
			for (size_t t = 0; t < c->h_btiles.size() / MPC_RB_TILE_WORDS && t < 64; ++t) {
				const u32 *w = &c->h_btiles[t * MPC_RB_TILE_WORDS];
				fprintf(stderr, "[mpcgpu] tile %zu: X %u+%u Y %u+%u rows [%u,%u) first %u slots %u; Y rows", t, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7] & 0xffu);
				for (u32 j = 0; j < w[3]; ++j) fprintf(stderr, " [%u,%u)", w[8 + j] & 0xffffu, w[8 + j] >> 16);
				fprintf(stderr, "\n");
			}
		if (upload(c, c->d_btiles, c->h_btiles)) return 1;
		HIPCHK(c, hipStreamSynchronize(c->stream));
		if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles: cut, checked and uploaded in %.2f ms\n", lap_ms());
		c->btiles_k0 = k0; c->btiles_k1 = k1;
	}
	const u32 ntiles = (u32)(c->h_btiles.size() / MPC_RB_TILE_WORDS);
	if (!ntiles) return 0;
	HIPCHK(c, c->d_tile_next.ensure(160 * 4));
	HIPCHK(c, hipMemsetAsync(c->d_tile_next.p, 0, 160 * 4, c->stream));
	RelaxBandParams rp;
	rp.s = sp; rp.ovf_off = c->d_ovf_off.as<u32>(); rp.nb1 = nb1; rp.cell_off = c->d_cell_off.as<u32>();
	rp.tiles = c->d_btiles.as<u32>(); rp.ntiles = ntiles; rp.k0 = k0; rp.k1 = k1; rp.cap_bytes = cap;
	rp.tile_next = c->d_tile_next.as<u32>();
	{ // cell order inside an X group (kernels_relaxb.h): blocks of G rows, a block's cells pair after pair. MPCGPU_RELAX_ORDER = G, or "pairs"
		// (no blocks: the layout until round 4's last profile). 1000 x 400, relax per step: pairs 880 ms, G = 1: 929, 2: 920, 4: 885,
		// 8: 849, 16: 851, 32: 886 (profiles/r09b_order_sweep.log). The two-list walk on wide rows (rdrp, <= 4x2 pairs, 3 cells per lane) gains nothing from
		// blocks: 12 577 ms against 12 280 pair after pair (profiles/r09c) — its default stays "pairs".
		const char *order_env = getenv("MPCGPU_RELAX_ORDER");
		const u32 order_default = use_win ? 8u : 0u;
		rp.by_rows = !order_env ? order_default : !strcmp(order_env, "pairs") ? 0u : (u32)atoi(order_env) > 0 ? (u32)atoi(order_env) : order_default;
	}
	const size_t smem = MPC_RB_TAB_BYTES + (size_t)cap;
	const int diag = env_int("MPCGPU_RELAX_DIAG", 0); // measurement only (results wrong): needs a library built with -DMPC_RELAX_DIAG_BUILD
#ifndef MPC_RELAX_DIAG_BUILD
	if (diag) return fail(c, "MPCGPU_RELAX_DIAG needs a library built with -DMPC_RELAX_DIAG_BUILD (measurement kernels: wrong results by design)");
#else
	if (diag) { fprintf(stderr, "[mpcgpu] WARNING: MPCGPU_RELAX_DIAG=%d: measurement kernel, the relax results are WRONG by design\n", diag); c->relax_fallback = true; }
#endif
	const char *merge_env = getenv("MPCGPU_RELAX_MERGE"); // "cxx": the compiler's code for the merge instead of the hand-scheduled one (A/B)
	const bool merge_cxx = merge_env && !strcmp(merge_env, "cxx");
	u32 grid = 1;
	const void *fn = nullptr;
	for (int go = 0; go < 2; ++go) { // pass 0: which instantiation (attributes, occupancy); pass 1: launch
		TimedSpan ts;
		if (go && span_begin(c, 3, &ts)) return 1;
		if (use_win) { // window records for the Y operand: the direct-index merge
			if (merge_cxx) { fn = (const void *)relax_band_kernel<kBandThreads, kBandSlotsWin, 2, 0, MpcRbWinCxx>; if (go) MPC_LAUNCH((relax_band_kernel<kBandThreads, kBandSlotsWin, 2, 0, MpcRbWinCxx>), grid, kBandThreads, smem, c->stream, rp); }
			else { fn = (const void *)relax_band_kernel<kBandThreads, kBandSlotsWin, 2, 0, MpcRbWinAsm>; if (go) MPC_LAUNCH((relax_band_kernel<kBandThreads, kBandSlotsWin, 2, 0, MpcRbWinAsm>), grid, kBandThreads, smem, c->stream, rp); }
		}
		else
		MPC_RB_DIAG_CASES(kBandThreads, kBandSlots)
		if (merge_cxx) { fn = (const void *)relax_band_kernel<kBandThreads, kBandSlots, 2, 0, MpcRbBlocksCxx>; if (go) MPC_LAUNCH((relax_band_kernel<kBandThreads, kBandSlots, 2, 0, MpcRbBlocksCxx>), grid, kBandThreads, smem, c->stream, rp); }
		else { fn = (const void *)relax_band_kernel<kBandThreads, kBandSlots, 2>; if (go) MPC_LAUNCH((relax_band_kernel<kBandThreads, kBandSlots, 2>), grid, kBandThreads, smem, c->stream, rp); }
		if (!go) {
			// (the two runtime queries cost a good fraction of a millisecond: once per context, kernel and LDS size — a -super7 run
			// relaxes 400 small stores on every worker context)
			int occ = 0;
			if (c->band_fn == fn && c->band_smem == smem) occ = c->band_occ;
			else {
				HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
				if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, (int)kBandThreads, smem) != hipSuccess || occ < 1) occ = 1;
				c->band_fn = fn; c->band_smem = smem; c->band_occ = occ;
			}
			grid = std::max(std::min<u32>(ntiles, cus * (u32)occ), 1u);
			char kn[128];
			snprintf(kn, sizeof(kn), "relax_band_kernel<%u, %u, 2, %d, %s>", kBandThreads, kernel_slots, diag,
				use_win ? (merge_cxx ? "MpcRbWinCxx" : "MpcRbWinAsm") : merge_cxx && !diag ? "MpcRbBlocksCxx" : "MpcRbBlocksAsm");
			c->relax_kernel_name = kn;
			if (trace_on()) { fprintf(stderr, "[mpcgpu] relax band: %s; lds=%zu B occ=%d grid=%u\n", c->tiles_desc.c_str(), smem, occ, grid); fflush(stderr); }
		} else {
			HIPCHK(c, hipGetLastError());
			if (span_end(c, &ts)) return 1;
		}
	}
#ifdef MPC_RELAX_DIAG_BUILD
	if (trace_on()) {
		u32 cnt[160];
		HIPCHK(c, hipMemcpyAsync(cnt, c->d_tile_next.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		fprintf(stderr, "[mpcgpu] relax band (measurement build): %u steps prefetched beside the current one, %u staged after the merges\n", cnt[9], cnt[8]);
		if (diag == 4) {
			const unsigned long long *t = (const unsigned long long *)(cnt + 16);
			fprintf(stderr, "[mpcgpu] relax band timers per wave number (share of the walk: barrier / staging block / DMA wait):");
			for (int w = 0; w < 16; ++w)
				fprintf(stderr, " %d: %.1f/%.1f/%.1f", w, 100.0 * t[4 * w + 1] / std::max<double>(t[4 * w], 1), 100.0 * t[4 * w + 2] / std::max<double>(t[4 * w], 1), 100.0 * t[4 * w + 3] / std::max<double>(t[4 * w], 1));
			fprintf(stderr, "\n");
		}
	}
#endif
	return 0;
}

int relax_var(mpcgpu_ctx *c, const StoreParams &sp, u64 k0, u64 k1)
{
	const u32 n = c->n;
	auto pidx = [&](u32 i, u32 j) { return pair_pos(c, i, j); };
	// Tiles of the primary geometry or the fallback out of a list of candidate tiles: a tile is kept when its cells fit the register slots and its
	// records of one step, packed back to back, fit one staging buffer at EVERY step (the worst step of every tile is measured on
	// the device); others are split (Y first, then X) and measured again. Single pairs that still do not fit go to `leftover`
	// (when given: the fallback takes them) or fail the call.
	auto build_tiles = [&](bool fallback, std::vector<u32> cand, std::vector<u32> &ok, std::vector<u32> *leftover) -> int {
		const u32 threads = 1024;
		const u32 buf_bytes = var_buf_bytes(fallback);
		const u32 max_slots = (u32)std::min<int>(std::max(env_int("MPCGPU_RELAX_SLOTS", (int)var_max_slots(fallback)), 1), (int)var_max_slots(fallback));
		// slots a tile needs: the cells of its pairs in [k0,k1), every pair rounded up to whole waves, in chunks of `threads`
		auto tile_slots = [&](u32 x0, u32 nx, u32 y0, u32 ny) {
			u64 cells = 0;
			for (u32 X = x0; X < x0 + nx; ++X)
				for (u32 Y = std::max(y0, X + 1); Y < y0 + ny; ++Y) {
					const u64 k = pidx(X, Y);
					if (k >= k0 && k < k1) cells += ((u64)c->all_nnz[k] + 63) & ~63ull;
				}
			return (u32)((cells + threads - 1) / threads);
		};
		std::vector<u32> tiles;
		bool too_big = false;
		std::function<void(u32, u32, u32, u32)> emit = [&](u32 x0, u32 nx, u32 y0, u32 ny) {
			const u32 slots = tile_slots(x0, nx, y0, ny);
			if (slots == 0) return;
			if (slots <= max_slots) { tiles.insert(tiles.end(), {x0, nx, y0, ny}); return; }
			if (ny > 1) { emit(x0, nx, y0, ny / 2); emit(x0, nx, y0 + ny / 2, ny - ny / 2); }
			else if (nx > 1) { emit(x0, nx / 2, y0, ny); emit(x0 + nx / 2, nx - nx / 2, y0, ny); }
			else if (leftover) leftover->insert(leftover->end(), {x0, nx, y0, ny});
			else too_big = true;
		};
		for (size_t t = 0; t + 3 < cand.size(); t += 4) emit(cand[t], cand[t + 1], cand[t + 2], cand[t + 3]);
		if (too_big) return fail(c, "mpcgpu_cons_iter: a pair has more than %u stored cells (tile slot budget)", max_slots * threads);
		const u32 budget_blocks = buf_bytes / 16;
		for (int round = 0; round < 8 && !tiles.empty(); ++round) {
			const u32 nt = (u32)(tiles.size() / 4);
			if (upload(c, c->d_tiles, tiles)) return 1;
			HIPCHK(c, c->d_tilefit.ensure((size_t)nt * 4));
			MPC_LAUNCH(var_tile_fit_kernel, std::min<u32>(nt, (u32)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp, c->d_tiles.as<u32>(), nt,
				c->d_tilefit.as<u32>());
			HIPCHK(c, hipGetLastError());
			std::vector<u32> fit(nt);
			HIPCHK(c, hipMemcpyAsync(fit.data(), c->d_tilefit.p, (size_t)nt * 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(c, hipStreamSynchronize(c->stream));
			std::vector<u32> next;
			u32 nsplit = 0;
			for (u32 t = 0; t < nt; ++t) {
				const u32 x0 = tiles[4 * t], nx = tiles[4 * t + 1], y0 = tiles[4 * t + 2], ny = tiles[4 * t + 3];
				if (fit[t] <= budget_blocks) { ok.insert(ok.end(), {x0, nx, y0, ny}); continue; }
				++nsplit;
				auto push = [&](u32 a, u32 b, u32 cc, u32 d) { if (tile_slots(a, b, cc, d)) next.insert(next.end(), {a, b, cc, d}); };
				if (ny > 1) { push(x0, nx, y0, ny / 2); push(x0, nx, y0 + ny / 2, ny - ny / 2); }
				else if (nx > 1) { push(x0, nx / 2, y0, ny); push(x0 + nx / 2, nx - nx / 2, y0, ny); }
				else if (leftover) leftover->insert(leftover->end(), {x0, nx, y0, ny});
				else return fail(c, "mpcgpu_cons_iter: the two records of pair (%u,%u) need %u bytes of LDS at some step, one staging buffer holds %u",
					x0, y0, fit[t] * 16, buf_bytes);
			}
			if (trace_on() && nsplit) { fprintf(stderr, "[mpcgpu] relax var: %u of %u tiles over the LDS budget (%u B), split\n", nsplit, nt, buf_bytes); fflush(stderr); }
			tiles.swap(next);
		}
		if (!tiles.empty()) return fail(c, "mpcgpu_cons_iter: tile splitting did not converge");
		return 0;
	};
	auto describe = [](const std::vector<u32> &ok) {
		u32 hist[5][5] = {{0}};
		for (size_t t = 0; t + 3 < ok.size(); t += 4) hist[std::min(ok[t + 1], 4u)][std::min(ok[t + 3], 4u)]++;
		char b[256];
		int o = snprintf(b, sizeof(b), "%zu tiles:", ok.size() / 4);
		for (u32 a = 4; a >= 1; --a)
			for (u32 bb = 4; bb >= 1; --bb)
				if (hist[a][bb] && o < (int)sizeof(b) - 24) o += snprintf(b + o, sizeof(b) - o, " %ux%u x %u", a, bb, hist[a][bb]);
		return std::string(b);
	};
	if (c->tiles_k0 != k0 || c->tiles_k1 != k1 || c->tiles_bx != 4 || c->tiles_by != 4) {
		c->tiles_k0 = c->tiles_k1 = ~0ull;
		// X blocks of 4, Y blocks of 4, walked in 8x8 super-tiles (the workgroups of an XCD read the same sequences' records)
		std::vector<u32> cand;
		const u32 nbx = (n + 3) / 4, nby = (n + 3) / 4;
		for (u32 sx = 0; sx < nbx; sx += 8)
			for (u32 sy = 0; sy < nby; sy += 8)
				for (u32 xb = sx; xb < std::min(sx + 8, nbx); ++xb)
					for (u32 yb = sy; yb < std::min(sy + 8, nby); ++yb) {
						const u32 x0 = xb * 4, nx = std::min(4u, n - x0), y0 = yb * 4, ny = std::min(4u, n - y0);
						if (y0 + ny <= x0 + 1) continue; // no pair X < Y in this block
						cand.insert(cand.end(), {x0, nx, y0, ny});
					}
		std::vector<u32> ok, ok2, left;
		if (build_tiles(false, cand, ok, c->var_mixed ? &left : nullptr)) return 1;
		if (!left.empty() && build_tiles(true, left, ok2, nullptr)) return 1;
		c->tiles_desc = describe(ok);
		if (!ok2.empty()) c->tiles_desc += "; + 1 x 1024-thread workgroup per CU, 1 staging buffer of 160 KB for " + describe(ok2);
		c->h_tiles.swap(ok);
		c->h_tiles2.swap(ok2);
		if (upload(c, c->d_tiles, c->h_tiles)) return 1;
		if (!c->h_tiles2.empty() && upload(c, c->d_tiles2, c->h_tiles2)) return 1;
		HIPCHK(c, hipStreamSynchronize(c->stream)); // the source of the async copy lives in the context; drained before any rebuild
		c->tiles_k0 = k0; c->tiles_k1 = k1; c->tiles_bx = 4; c->tiles_by = 4;
	}
	if (c->h_tiles.empty() && c->h_tiles2.empty()) return 0;
	HIPCHK(c, c->d_tile_next.ensure(16 * 4));
	HIPCHK(c, hipMemsetAsync(c->d_tile_next.p, 0, 16 * 4, c->stream));
	if (!c->h_tiles.empty() && relax_var_launch(c, sp, k0, k1, false, c->d_tiles, (u32)(c->h_tiles.size() / 4), true)) return 1;
	if (!c->h_tiles2.empty() && relax_var_launch(c, sp, k0, k1, true, c->d_tiles2, (u32)(c->h_tiles2.size() / 4), c->h_tiles.empty())) return 1;
	return 0;
}


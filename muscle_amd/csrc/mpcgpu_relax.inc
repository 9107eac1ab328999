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

// MPCGPU_RELAX_SLOTS: the cells per lane the tiles of either kernel are cut to, 1 .. the kernel's own
static u32 relax_slots(u32 kernel_slots) { return (u32)std::min<int>(std::max(env_int("MPCGPU_RELAX_SLOTS", (int)kernel_slots), 1), (int)kernel_slots); }
// MPCGPU_RELAX_DIAG=1|2|3 (staging only / merges only / merges + barriers; band kernel: also 4, per-wave phase timers): measurement kernels whose
// results are WRONG by design; they exist only in a library built with -DMPC_RELAX_DIAG_BUILD (make diag), which also says so on stderr at every launch
static int relax_diag_env() { return env_int("MPCGPU_RELAX_DIAG", 0); }
// the measurement mode of a launch: an error in the product library, a warning and is_fallback in the measurement build
static int relax_diag_mode(mpcgpu_ctx *c, int *diag)
{
	*diag = relax_diag_env();
#ifndef MPC_RELAX_DIAG_BUILD
	if (*diag) return fail(c, "MPCGPU_RELAX_DIAG needs a library built with -DMPC_RELAX_DIAG_BUILD (measurement kernels: wrong results by design)");
#else
	if (*diag) { fprintf(stderr, "[mpcgpu] WARNING: MPCGPU_RELAX_DIAG=%d: measurement kernel, the relax results are WRONG by design\n", *diag); c->relax_fallback = true; }
#endif
	return 0;
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
	int diag = 0;
	if (report && relax_diag_mode(c, &diag)) return 1;
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
constexpr u32 kBandSlotsWin = 15; // cells per lane of the direct-index merge (its two-word descriptor sets became one word each: registers for two more cells)
constexpr u32 kBandThreads = 1024, kBandSlots = 13; // two 1024-thread workgroups per CU (8 waves per SIMD, 64 VGPRs), 13 cells per lane (14: spill reloads inside the walk, and every reload waits for vmcnt(0) - the prefetch)

// geometry and knobs of the band relax, for the cutter and the launch alike
struct BandGeom {
	u32 cap, cap_blocks;    // staging area after the tables: bytes, 16-byte blocks
	u32 margin, half, full; // blocks: what steps vary around their mean by; the targets "two steps resident" and "one step, the whole area"
	bool use_win;           // the direct-index merge (window records for the Y operand)
	u32 kernel_slots, max_slots, cus; // cells per lane of the kernel / the tiles are cut to (MPCGPU_RELAX_SLOTS); CUs
};
static BandGeom band_geom(const mpcgpu_ctx *c)
{
	BandGeom g;
	// geometry: two 1024-thread workgroups per CU, 80 KB of LDS each (kBandThreads). (Measured and removed: four 512-thread workgroups
	// per CU with 40 KB each, whose barriers hold 8 waves instead of 16: 9.6 of 13 cells per lane at 1000 x L~400, and 2472 against
	// 1545 ms per two iterations on rdrp-500 — profiles/r06g, r10a)
	// (measured and removed again, profiles/r10a_rdrp_geometry_sweep.log: ONE 1024-thread workgroup per CU with the CU's 160 KB and 26 cells per
	// lane — 8x4 bands, 10.7 cells per lane, every step prefetched, 6.6 B per cell-step instead of 11.7 — is 18 % SLOWER on real data
	// (rdrp-500: 1818 against 1545 ms per two iterations): the walk's merges are chains of dependent LDS reads and want 8 waves per SIMD)
	const u32 lds_bytes = (u32)std::max(env_int("MPCGPU_RELAX_LDS_KB", 80), 3) * 1024u;
	g.cap = (lds_bytes - MPC_RB_TAB_BYTES) & ~15u; g.cap_blocks = g.cap / 16;
	g.cus = (u32)c->prop.multiProcessorCount;
	// the direct-index merge (window records for the Y operand) where the store has them; the measurement kernels exist for the
	// block walk only
	g.use_win = c->win_ok && !relax_diag_env();
	g.kernel_slots = g.use_win ? kBandSlotsWin : kBandSlots;
	g.max_slots = relax_slots(g.kernel_slots);
	g.margin = std::min<u32>(g.cap_blocks / 16, 64); // blocks: steps vary around the mean
	g.half = g.cap_blocks / 2 > g.margin ? g.cap_blocks / 2 - g.margin : g.cap_blocks / 2;
	g.full = g.cap_blocks > 2 * g.margin ? g.cap_blocks - 2 * g.margin : g.cap_blocks;
	return g;
}

// ---- the tile cutter: what its steps share (the store, the band tables, the geometry, the pair range)
struct BandCut { mpcgpu_ctx *c; const StoreParams &sp; RbTileTabs tb; const BandGeom &g; u64 k0, k1; };
struct BandShape { u32 nx = 0, ny = 0, target = 0; }; // super-tiles of nx x ny sequences, bands cut to `target` blocks per step (mean); nx == 0: none

// tile words of a list of tiles whose words 0..5 are set: Y ranges, first-piece blocks, slots; out: slots, mean blocks, bound, cells
static int eval_tiles(const BandCut &bc, std::vector<u32> &words, std::vector<u32> &out)
{
	mpcgpu_ctx *c = bc.c;
	const u32 nt = (u32)(words.size() / MPC_RB_TILE_WORDS);
	out.assign((size_t)nt * 4, 0u);
	if (!nt) return 0;
	if (upload(c, c->d_btiles, words)) return 1;
	HIPCHK(c, c->d_bt_out.ensure((size_t)nt * 16));
	MPC_LAUNCH(band_eval_kernel, std::min<u32>(nt, bc.g.cus * 32), 64, 0, c->stream, bc.sp, bc.tb, c->d_btiles.as<u32>(), nt, c->d_bt_out.as<u32>());
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(words.data(), c->d_btiles.p, words.size() * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(out.data(), c->d_bt_out.p, out.size() * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}
static u64 init_pair_index(u32 n, u32 X, u32 Y) { return (u64)X * n - ((u64)X * (X + 1)) / 2 + (Y - X - 1); } // InitPairs order (mpcflat.cpp:145-155), X < Y
// does the block of sequences [x0, x0+cx) x [y0, y0+cy) hold a pair whose position may lie in [k0, k1)? (a conservative test: the
// kernels check every pair's own position)
static bool block_in_range(const BandCut &bc, u32 x0, u32 cx, u32 y0, u32 cy)
{
	const mpcgpu_ctx *c = bc.c;
	const u64 k0 = bc.k0, k1 = bc.k1;
	if (c->order_rects.empty()) {
		// InitPairs order: pair indices grow with X first — the block's pairs lie between its first row's first and its last row's last pair
		const u32 xl = std::min(x0 + cx - 1, y0 + cy - 2);
		return !(init_pair_index(c->n, x0, std::max(y0, x0 + 1)) >= k1 || init_pair_index(c->n, xl, y0 + cy - 1) < k0);
	}
	for (size_t r = 0; r < c->order_rects.size() / 4; ++r) { // block order: the rectangles whose positions meet [k0, k1) and whose sequences meet the block's
		const u32 *q = &c->order_rects[4 * r];
		const u64 cnt = q[2] >= q[1] ? (u64)(q[1] - q[0]) * (q[3] - q[2]) : (u64)(q[1] - q[0]) * (q[1] - q[0] - 1) / 2;
		if (c->order_base[r] >= k1 || c->order_base[r] + cnt <= k0) continue;
		if (x0 < q[1] && x0 + cx > q[0] && y0 < q[3] && y0 + cy > q[2]) return true;
	}
	return false;
}
// super-tiles of nx x ny sequences cut into row bands of <= max_slots cells per lane and <= target blocks per step (mean)
// stride > 1: every stride-th super-tile only — a SAMPLE of the cut, for pricing a shape (the search below)
// with_cells: receives the number of super-tiles of this cut that hold a cell
static int cut(const BandCut &bc, u32 nx, u32 ny, u32 target, std::vector<u32> &words, std::vector<u32> &out, u32 stride = 1, u64 *with_cells = nullptr)
{
	mpcgpu_ctx *c = bc.c;
	const u32 n = c->n, nb1 = bc.tb.nb1, max_slots = bc.g.max_slots;
	std::vector<u32> cand;
	const u32 nbx = (n + nx - 1) / nx, nby = (n + ny - 1) / ny;
	u64 seen = 0;
	for (u32 xb = 0; xb < nbx; ++xb)
		for (u32 yb = 0; yb < nby; ++yb) {
			const u32 x0 = xb * nx, cx = std::min(nx, n - x0), y0 = yb * ny, cy = std::min(ny, n - y0);
			if (y0 + cy <= x0 + 1) continue; // no pair X < Y in this block
			// a rank of a sharded run relaxes [k0, k1) only: blocks whose pairs all lie outside that range are not candidates
			if (!block_in_range(bc, x0, cx, y0, cy)) continue;
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
	const u32 grid = std::min<u32>(nc, bc.g.cus * 32);
	MPC_LAUNCH(band_cut_kernel, grid, 64, (size_t)(nb1 + 1) * 8, c->stream, bc.sp, bc.tb, (const u32 *)hcand, nc, max_slots, target, 0, cnt,
		(const u32 *)nullptr, (u32 *)nullptr);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipStreamSynchronize(c->stream));
	u64 tot = 0, nonempty = 0;
	for (u32 q = 0; q < nc; ++q) { base[q] = (u32)tot; tot += cnt[q]; nonempty += cnt[q] ? 1 : 0; }
	if (with_cells) *with_cells = nonempty;
	if (tot > 0x7fffffffull / MPC_RB_TILE_WORDS) return fail(c, "mpcgpu_cons_iter: too many band tiles");
	words.assign((size_t)tot * MPC_RB_TILE_WORDS, 0u);
	if (!tot) { out.clear(); return 0; }
	HIPCHK(c, c->d_btiles.ensure(words.size() * 4));
	MPC_LAUNCH(band_cut_kernel, grid, 64, (size_t)(nb1 + 1) * 8, c->stream, bc.sp, bc.tb, (const u32 *)hcand, nc, max_slots, target, 1, (u32 *)nullptr,
		(const u32 *)base, c->d_btiles.as<u32>());
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(words.data(), c->d_btiles.p, words.size() * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream)); // (the tile words are read back before eval_tiles below reuses them)
	return eval_tiles(bc, words, out);
}
// the exact worst step (blocks, the maximum over Z) of the listed tiles of the device's tile words: for the sample that prices
// "one step resident" (sample_r95) and for the tiles whose upper bound does not settle the fit (fit_or_split)
static int fit_worst_steps(const BandCut &bc, const std::vector<u32> &list, std::vector<u32> &worst)
{
	mpcgpu_ctx *c = bc.c;
	if (upload(c, c->d_bt_list, list)) return 1;
	HIPCHK(c, c->d_bt_count.ensure(list.size() * 4));
	MPC_LAUNCH(band_fit_kernel, std::min<u32>(((u32)list.size() + 3u) / 4u, bc.g.cus * 8), 256, 0, c->stream, bc.sp, c->d_ovf_off.as<u32>(), bc.tb.nb1,
		c->d_btiles.as<u32>(), c->d_bt_list.as<u32>(), (u32)list.size(), c->d_bt_count.as<u32>(), bc.tb.win);
	HIPCHK(c, hipGetLastError());
	worst.resize(list.size());
	HIPCHK(c, hipMemcpyAsync(worst.data(), c->d_bt_count.p, list.size() * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

// Shape of the super-tiles and the target the bands are cut to. MPCGPU_RELAX_SHAPE=nx,ny[,kb]: forced.
// Narrow rows (1000 x L~400: 2 cells per row, y ranges that follow the diagonal): 8x8 super-tiles whose steps leave room for
// the next step beside the current one fill the register slots — taken at once. Otherwise (real data: 7 cells per row, the
// cells of 50 rows spread over 200 rows of the partner, and steps that vary by a factor of 1.6 around their mean) every
// shape of the menu is cut in both modes and priced: a tile-step costs a fixed part (staging block, barrier; plus the exposed
// transfer when the next step cannot be prefetched) and a part per cell slot. Shapes with more X than Y sequences are on the
// menu because the X pieces are the band's rows only, the Y pieces the whole range those rows' cells reach.
// s.nx == 0 afterwards: no cell in [k0,k1)
static int choose_shape(const BandCut &bc, BandShape &s, std::vector<u32> &words, std::vector<u32> &out)
{
	mpcgpu_ctx *c = bc.c;
	const BandGeom &g = bc.g;
	const u32 n = c->n, nb1 = bc.tb.nb1, half = g.half, full = g.full, max_slots = g.max_slots;
	static const u32 menu[10][2] = {{8, 8}, {8, 4}, {8, 2}, {8, 1}, {4, 4}, {4, 2}, {4, 1}, {2, 2}, {2, 1}, {1, 1}};
	std::vector<u32> &w2 = c->v_w2, &o2 = c->v_o2; // (kept: see mpcgpu_ctx)
	if (const char *sh = getenv("MPCGPU_RELAX_SHAPE")) { // route 1: forced
		unsigned a = 0, b = 0, kb = 0;
		const int got = sscanf(sh, "%u,%u,%u", &a, &b, &kb);
		if (got >= 2 && a >= 1 && a <= MPC_RB_MAXN && b >= 1 && b <= MPC_RB_MAXN) {
			s = {a, b, got == 3 && kb ? std::min<u32>(kb * 64, g.cap_blocks) : half};
			if (cut(bc, s.nx, s.ny, s.target, words, out)) return 1;
		}
		if (trace_on()) {
			if (s.nx) fprintf(stderr, "[mpcgpu] band tiles forced: %ux%u, target %u blocks\n", s.nx, s.ny, s.target);
			else fprintf(stderr, "[mpcgpu] band tiles: MPCGPU_RELAX_SHAPE=%s is not a shape, searching\n", sh);
		}
	}
	if (!s.nx && n <= 64) { // route 2
		// few sequences (the shrubs of -super7, the clusters of -super5): the 8 x 8 super-tiles with ALL their rows as one band
		// each, evaluated in one pass; taken when every one of them fits the cell slots and leaves room for the next step
		w2.clear(); o2.clear();
		for (u32 x0 = 0; x0 < n; x0 += 8)
			for (u32 y0 = x0; y0 < n; y0 += 8) {
				u32 nw[MPC_RB_TILE_WORDS] = {x0, std::min(8u, n - x0), y0, std::min(8u, n - y0), 0u, (nb1 - 1) * (u32)MPC_RB_HB};
				if (y0 + nw[3] > x0 + 1) w2.insert(w2.end(), nw, nw + MPC_RB_TILE_WORDS);
			}
		if (eval_tiles(bc, w2, o2)) return 1;
		bool ok = !w2.empty();
		for (size_t t = 0; t + 3 < o2.size(); t += 4) ok = ok && o2[t] <= max_slots && o2[t + 1] <= half;
		if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles, %u sequences, one band per 8x8 super-tile: %zu tiles, %s\n", n, o2.size() / 4,
			ok ? "taken" : "refused (a super-tile over the slots or the target)");
		if (ok) { words.swap(w2); out.swap(o2); s = {8, 8, half}; }
	}
	if (!s.nx) { // route 3: 8x8 with two steps resident, taken at once where it fills the register slots
		u64 with_cells = 0, cells = 0, est = 0, ok = 0;
		if (cut(bc, 8, 8, half, words, out, 1, &with_cells)) return 1;
		const u64 tiles = out.size() / 4;
		for (size_t t = 0; t + 3 < out.size(); t += 4) { cells += out[t + 3]; est += out[t + 1]; ok += out[t + 1] <= half ? 1 : 0; }
		const double fill = tiles ? (double)cells / ((double)tiles * max_slots * kBandThreads) : 0.0, in_target = tiles ? (double)ok / (double)tiles : 0.0;
		if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles 8x8, two steps resident: %llu tiles, fill %.2f, %.2f B/cell-step, %.0f %% within target\n",
			(unsigned long long)tiles, fill, cells ? 16.0 * (double)est / (double)cells : 0.0, 100 * in_target);
		if (!tiles) return 0;
		const char *why = "not taken, searching"; // (trace only)
		if (fill >= 0.70 && in_target >= 0.90) { s = {8, 8, half}; why = "taken, the slots are filled"; }
		// few cells (the shrubs of -super7: 32 sequences): nothing was cut — one band per super-tile — so no other shape or target
		// gives fewer tile-steps, and the search below (20 more cuts) is skipped
		else if (in_target >= 1.0 && tiles == with_cells) { s = {8, 8, half}; why = "taken, nothing was cut"; }
		if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles 8x8, two steps resident: %s\n", why);
	}
	if (s.nx) return 0;
	// route 4: the priced search
	// Round 6: the twenty cuts of the search are PRICED on every 8th super-tile when there are thousands of them (the cost is a
	// sum over tiles: an eighth of them, evenly spread, ranks the shapes the same), and only the winner is cut in full — on the
	// first 1000 rdrp records the search was 0.47 s of a 13.4 s step (44 launches of band_cut_kernel = 0.17 s, the rest host work
	// on 450 000 tiles x 21 cuts): profiles/r13a_kernel_stats_rdrp1000.csv
	const u32 price_stride = (u64)((n + 7) / 8) * ((n + 7) / 8) / 2 >= 4096 ? 8u : 1u;
	// worst step / mean step of this data set: the exact worst steps of a sample of 4x2 tiles cut to the whole area (95th percentile)
	double r95 = 1.0;
	{
		if (cut(bc, 4, 2, full, words, out, price_stride)) return 1; // (a sample of a sample where there are thousands of super-tiles)
		const u32 nt = (u32)(words.size() / MPC_RB_TILE_WORDS);
		std::vector<u32> sample;
		const u32 stride = std::max(nt / 4096u, 1u);
		for (u32 t = 0; t < nt; t += stride) if (out[4 * t + 3]) sample.push_back(t);
		if (!sample.empty()) {
			std::vector<u32> worst;
			if (upload(c, c->d_btiles, words) || fit_worst_steps(bc, sample, worst)) return 1;
			std::vector<double> ratio;
			for (size_t q = 0; q < sample.size(); ++q) if (out[4 * sample[q] + 1]) ratio.push_back((double)worst[q] / (double)out[4 * sample[q] + 1]);
			if (!ratio.empty()) { std::sort(ratio.begin(), ratio.end()); r95 = std::max(ratio[std::min(ratio.size() - 1, (size_t)(0.95 * (double)ratio.size()))], 1.0); }
		}
	}
	const u32 single = std::max(std::min((u32)((double)g.cap_blocks / r95 * 0.98), full), 1u); // mean step such that the worst one still fits
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
	w2.clear(); o2.clear();
	for (u32 mode = 0; mode < 2; ++mode)
		for (u32 m = 0; m < 10; ++m) {
			const u32 target = mode == 0 ? half : single;
			if (cut(bc, menu[m][0], menu[m][1], target, w2, o2, price_stride)) return 1;
			u64 slots = 0, over = 0;
			const u64 nt = o2.size() / 4;
			for (size_t t = 0; t + 3 < o2.size(); t += 4) { slots += std::min(o2[t], max_slots); over += o2[t + 1] > target ? 1 : 0; }
			if (!nt) continue;
			// tiles over the target (single index bands that do not fit) will be split by sequences: charged double
			const double cost = ((double)nt + (double)over) * (fixed + (mode ? exposed : 0.0)) + (double)slots;
			if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles %ux%u, %s: %llu tiles (%llu over the target), %.1f cells per lane, cost %.3g\n",
				menu[m][0], menu[m][1], mode ? "one step resident" : "two steps resident", (unsigned long long)nt, (unsigned long long)over,
				(double)slots / (double)nt, cost);
			if (!have || cost < best) { have = true; best = cost; words.swap(w2); out.swap(o2); s = {menu[m][0], menu[m][1], target}; }
		}
	if (have && price_stride > 1 && cut(bc, s.nx, s.ny, s.target, words, out)) return 1; // the winner, in full
	return 0;
}

// halves a tile {x0, nx, y0, ny, r0, r1} into a and b: by row bands first where asked (band tiles), then by Y, then by X sequences; false: a single
// pair (and band) is left
static bool halve_tile(const u32 *w, bool rows_first, u32 *a, u32 *b)
{
	for (u32 i = 0; i < 6; ++i) a[i] = b[i] = w[i];
	const u32 hb = rows_first ? (w[5] - w[4]) / MPC_RB_HB : 0u;
	if (hb > 1) a[5] = b[4] = w[4] + (hb / 2) * MPC_RB_HB;
	else if (w[3] > 1) { a[3] = w[3] / 2; b[2] = w[2] + w[3] / 2; b[3] = w[3] - w[3] / 2; }
	else if (w[1] > 1) { a[1] = w[1] / 2; b[0] = w[0] + w[1] / 2; b[1] = w[1] - w[1] / 2; }
	else return false;
	return true;
}
// every tile must fit: cells per lane, 16-bit first-piece offsets, and its WORST step in the staging area (upper bound
// first; the exact maximum over Z only where the bound does not settle it). What does not fit is halved: band, then Y, then X.
// The tiles that fit go to okw. 2: rows of a single pair do not fit
static int fit_or_split(const BandCut &bc, std::vector<u32> &words, std::vector<u32> &out, std::vector<u32> &okw, u64 *nsplit)
{
	mpcgpu_ctx *c = bc.c;
	const u32 max_slots = bc.g.max_slots, cap_blocks = bc.g.cap_blocks;
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
			if (fit_worst_steps(bc, need, exact)) return 1;
			for (size_t q = 0; q < need.size(); ++q) out[4 * need[q] + 2] = exact[q]; // the bound becomes the exact worst step
		}
		std::vector<u32> next;
		u64 by_band = 0, by_y = 0, by_x = 0, over_first = 0; // (trace only)
		for (u32 t = 0; t < nt; ++t) {
			const u32 *w = &words[(size_t)t * MPC_RB_TILE_WORDS];
			if (out[4 * t + 3] == 0) continue; // no cell
			if (out[4 * t] <= max_slots && w[6] <= MPC_RB_MAXFIRST && out[4 * t + 2] <= cap_blocks) { okw.insert(okw.end(), w, w + MPC_RB_TILE_WORDS); continue; }
			++*nsplit;
			u32 a[MPC_RB_TILE_WORDS] = {0}, b[MPC_RB_TILE_WORDS] = {0};
			if (!halve_tile(w, true, a, b)) {
				if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles: rows [%u,%u) of pair (%u,%u) do not fit (slots %u, first %u, worst step %u blocks of %u)\n",
					w[4], w[5], w[0], w[2], out[4 * t], w[6], out[4 * t + 2], cap_blocks);
				return 2;
			}
			next.insert(next.end(), a, a + MPC_RB_TILE_WORDS);
			next.insert(next.end(), b, b + MPC_RB_TILE_WORDS);
			if (a[5] != w[5]) ++by_band; else if (a[3] != w[3]) ++by_y; else ++by_x;
			if (out[4 * t] <= max_slots && w[6] > MPC_RB_MAXFIRST) ++over_first;
		}
		if (trace_on() && by_band + by_y + by_x)
			fprintf(stderr, "[mpcgpu] band tiles: round %d halves %llu tiles by band, %llu by Y, %llu by X (%llu of them over the first-piece limit of %u blocks alone)\n",
				round, (unsigned long long)by_band, (unsigned long long)by_y, (unsigned long long)by_x, (unsigned long long)over_first, (unsigned)MPC_RB_MAXFIRST);
		words.swap(next);
		if (eval_tiles(bc, words, out)) return 1;
	}
	return words.empty() ? 0 : 2;
}
// The tail of the launch: the kernel deals the list to the 8 XCDs in contiguous chunks (a counter each), and a chunk's
// LAST tiles — one per resident workgroup of the XCD — are the ones that finish alone. They are cut in two by rows (any
// part of a tile is a valid tile): half the tail, which is one tile of ~62 per workgroup on one GPU and one of ~8 on a rank
// of eight (profiles/r12c: 109.4 -> 107.1 ms per rank of 8, 792.2 -> 791.0 ms on one GPU).
// Returns the tiles cut in two.
static u64 split_tail(u32 cus, std::vector<u32> &okw)
{
	u64 ntail_split = 0;
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
	return ntail_split;
}
// the tile list in words (relax_info); o2: the statistics of the final list as eval_tiles left them
static std::string describe_band_tiles(const BandGeom &g, const BandShape &s, u64 nsplit, size_t nt, const std::vector<u32> &o2)
{
	u64 cells = 0, est = 0, slots = 0;
	for (size_t t = 0; t + 3 < o2.size(); t += 4) { cells += o2[t + 3]; est += o2[t + 1]; slots += o2[t + 3] ? o2[t] : 0u; }
	char b[384];
	snprintf(b, sizeof(b), "%zu band tiles of <= %ux%u pairs (%llu split), target %u B per step of %u B staging (%s), mean step %.0f B, %.1f of %u cells per lane (%.2f slots on the busiest wave), %.2f B per cell-step",
		nt, s.nx, s.ny, (unsigned long long)nsplit, s.target * 16, g.cap, s.target <= g.cap_blocks / 2 ? "two steps resident" : "one step resident",
		nt ? 16.0 * (double)est / (double)nt : 0.0, nt ? (double)cells / ((double)nt * kBandThreads) : 0.0, g.max_slots, nt ? (double)slots / (double)nt : 0.0, cells ? 16.0 * (double)est / (double)cells : 0.0);
	return b;
}
// MPCGPU_TRACE & 2: the first 64 tiles
static void trace_band_tiles(const std::vector<u32> &tiles)
{
	for (size_t t = 0; t < tiles.size() / MPC_RB_TILE_WORDS && t < 64; ++t) {
		const u32 *w = &tiles[t * MPC_RB_TILE_WORDS];
		fprintf(stderr, "[mpcgpu] tile %zu: X %u+%u Y %u+%u rows [%u,%u) first %u slots %u; Y rows", t, w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7] & 0xffu);
		for (u32 j = 0; j < w[3]; ++j) fprintf(stderr, " [%u,%u)", w[8 + j] & 0xffffu, w[8 + j] >> 16);
		fprintf(stderr, "\n");
	}
}

// cuts, checks and uploads the band tiles of [k0,k1) and caches them (the sparsity pattern is frozen). 0 = done (possibly no tile),
// 1 = error, 2 = rows of a single pair do not fit
static int cut_band_tiles(mpcgpu_ctx *c, const StoreParams &sp, const BandGeom &g, u64 k0, u64 k1)
{
	c->btiles_k0 = c->btiles_k1 = ~0ull;
	const auto t_cut0 = std::chrono::steady_clock::now();
	BandCut bc = {c, sp, {}, g, k0, k1};
	RbTileTabs &tb = bc.tb;
	const bool use_win = g.use_win;
	tb.cell_off = c->d_cell_off.as<u32>(); tb.yr = c->d_yr.as<u32>(); tb.ovf_sum = c->d_ovf_sum.as<u32>(); tb.ovf_maxc = c->d_ovf_maxc.as<u32>();
	tb.nb1 = c->band_nb1; tb.threads = kBandThreads; tb.k0 = k0; tb.k1 = k1;
	tb.win = use_win ? 1u : 0u;
	tb.ysum = use_win ? c->d_wsum.as<u32>() : tb.ovf_sum; tb.ymaxc = use_win ? c->d_wmaxc.as<u32>() : tb.ovf_maxc;
	std::vector<u32> &words = c->v_words, &out = c->v_out, &okw = c->v_okw; // (kept: see mpcgpu_ctx)
	words.clear(); out.clear();
	BandShape s;
	if (choose_shape(bc, s, words, out)) return 1;
	if (!s.nx) { c->h_btiles.clear(); c->btiles_k0 = k0; c->btiles_k1 = k1; return 0; } // no cell in [k0,k1)
	okw.clear();
	u64 nsplit = 0;
	if (const int r = fit_or_split(bc, words, out, okw, &nsplit)) return r;
	const u64 ntail_split = split_tail(g.cus, okw);
	std::vector<u32> &o2 = c->v_o2, &w2 = c->v_w2; // (kept: see mpcgpu_ctx)
	w2 = okw;
	if (eval_tiles(bc, w2, o2)) return 1; // (fills words 6.. of the halves; also leaves the final list's statistics for the description)
	if (ntail_split) { // halves without a cell go; the others are tiles like any other
		okw.clear();
		for (size_t t = 0; t < w2.size() / MPC_RB_TILE_WORDS; ++t)
			if (o2[4 * t + 3]) okw.insert(okw.end(), w2.begin() + t * MPC_RB_TILE_WORDS, w2.begin() + (t + 1) * MPC_RB_TILE_WORDS);
		if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles: tail of %zu tiles on %u CUs: %llu cut in two by rows, %zu halves without a cell dropped\n",
			w2.size() / MPC_RB_TILE_WORDS - (size_t)ntail_split, g.cus, (unsigned long long)ntail_split, (w2.size() - okw.size()) / MPC_RB_TILE_WORDS);
	}
	c->tiles_desc = describe_band_tiles(g, s, nsplit, okw.size() / MPC_RB_TILE_WORDS, o2);
	c->h_btiles.swap(okw);
	if (trace_on() && (trace_level() & 2)) trace_band_tiles(c->h_btiles);
	if (upload(c, c->d_btiles, c->h_btiles)) return 1;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (trace_on()) fprintf(stderr, "[mpcgpu] band tiles: cut, checked and uploaded in %.2f ms\n",
		std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_cut0).count());
	c->btiles_k0 = k0; c->btiles_k1 = k1;
	return 0;
}

// ---- the band launch. The instantiation a launch runs: its address (attributes, occupancy), launched when `go`
template <int SL, int DG, class Merge> const void *relax_band_go(bool go, const RelaxBandParams &rp, u32 grid, size_t smem, hipStream_t st)
{
	if (go) MPC_LAUNCH((relax_band_kernel<kBandThreads, SL, 2, DG, Merge>), grid, kBandThreads, smem, st, rp);
	return (const void *)relax_band_kernel<kBandThreads, SL, 2, DG, Merge>;
}
// window records for the Y operand: the direct-index merge; else the block walk, which alone has measurement kernels (diag 1..4, with the
// hand-scheduled merge). merge_cxx: the compiler's code for the merge instead of the hand-scheduled one (A/B)
// seg: the store lies in segments (StoreParams::pad_zbase) — the same four merges with the per-step base address in the staging; a
// store of one segment never comes here, so what it launches is what it always launched
// long_form: the records' long form (kernels_store.h) — its own merge, in either staging; no window records, no measurement kernels
static const void *relax_band_select(bool go, bool use_win, bool merge_cxx, int diag, bool seg, bool long_form, const RelaxBandParams &rp, u32 grid, size_t smem, hipStream_t st)
{
	if (long_form) {
		if (seg) return relax_band_go<kBandSlots, 0, MpcRbSegmented<MpcRbLongCxx> >(go, rp, grid, smem, st);
		return relax_band_go<kBandSlots, 0, MpcRbLongCxx>(go, rp, grid, smem, st);
	}
	if (seg) {
		if (use_win && merge_cxx) return relax_band_go<kBandSlotsWin, 0, MpcRbSegmented<MpcRbWinCxx> >(go, rp, grid, smem, st);
		if (use_win) return relax_band_go<kBandSlotsWin, 0, MpcRbSegmented<MpcRbWinAsm> >(go, rp, grid, smem, st);
		if (merge_cxx) return relax_band_go<kBandSlots, 0, MpcRbSegmented<MpcRbBlocksCxx> >(go, rp, grid, smem, st);
		return relax_band_go<kBandSlots, 0, MpcRbSegmented<MpcRbBlocksAsm> >(go, rp, grid, smem, st);
	}
	if (use_win && merge_cxx) return relax_band_go<kBandSlotsWin, 0, MpcRbWinCxx>(go, rp, grid, smem, st);
	if (use_win) return relax_band_go<kBandSlotsWin, 0, MpcRbWinAsm>(go, rp, grid, smem, st);
#ifdef MPC_RELAX_DIAG_BUILD
	if (diag == 1) return relax_band_go<kBandSlots, 1, MpcRbBlocksAsm>(go, rp, grid, smem, st);
	if (diag == 2) return relax_band_go<kBandSlots, 2, MpcRbBlocksAsm>(go, rp, grid, smem, st);
	if (diag == 3) return relax_band_go<kBandSlots, 3, MpcRbBlocksAsm>(go, rp, grid, smem, st);
	if (diag == 4) return relax_band_go<kBandSlots, 4, MpcRbBlocksAsm>(go, rp, grid, smem, st);
#endif
	if (merge_cxx) return relax_band_go<kBandSlots, 0, MpcRbBlocksCxx>(go, rp, grid, smem, st);
	return relax_band_go<kBandSlots, 0, MpcRbBlocksAsm>(go, rp, grid, smem, st);
}
// cell order inside an X group (kernels_relaxb.h): blocks of G rows, a block's cells pair after pair. MPCGPU_RELAX_ORDER = G, or "pairs"
// (no blocks: the layout until round 4's last profile). 1000 x 400, relax per step: pairs 880 ms, G = 1: 929, 2: 920, 4: 885,
// 8: 849, 16: 851, 32: 886 (profiles/r09b_order_sweep.log). The two-list walk on wide rows (rdrp, <= 4x2 pairs, 3 cells per lane) gains nothing from
// blocks: 12 577 ms against 12 280 pair after pair (profiles/r09c) — its default stays "pairs".
static u32 band_cell_order(bool use_win)
{
	const char *order_env = getenv("MPCGPU_RELAX_ORDER");
	const u32 order_default = use_win ? 8u : 0u;
	return !order_env ? order_default : !strcmp(order_env, "pairs") ? 0u : (u32)atoi(order_env) > 0 ? (u32)atoi(order_env) : order_default;
}

// 0 = launched (or nothing to do), 1 = error, 2 = not for band tiles (the caller runs relax_var)
int relax_band(mpcgpu_ctx *c, const StoreParams &sp, u64 k0, u64 k1)
{
	const BandGeom g = band_geom(c);
	if (c->btiles_k0 != k0 || c->btiles_k1 != k1)
		if (const int r = cut_band_tiles(c, sp, g, k0, k1)) return r;
	const u32 ntiles = (u32)(c->h_btiles.size() / MPC_RB_TILE_WORDS);
	if (!ntiles) return 0;
	HIPCHK(c, c->d_tile_next.ensure(160 * 4));
	HIPCHK(c, hipMemsetAsync(c->d_tile_next.p, 0, 160 * 4, c->stream));
	RelaxBandParams rp;
	rp.s = sp; rp.ovf_off = c->d_ovf_off.as<u32>(); rp.nb1 = c->band_nb1; rp.cell_off = c->d_cell_off.as<u32>();
	rp.tiles = c->d_btiles.as<u32>(); rp.ntiles = ntiles; rp.k0 = k0; rp.k1 = k1; rp.cap_bytes = g.cap;
	rp.tile_next = c->d_tile_next.as<u32>();
	rp.by_rows = band_cell_order(g.use_win);
	const size_t smem = MPC_RB_TAB_BYTES + (size_t)g.cap;
	int diag = 0;
	if (relax_diag_mode(c, &diag)) return 1;
	const bool seg = sp.pad_zbase != nullptr || sp.win_zbase != nullptr;
	if (seg && diag) return fail(c, "MPCGPU_RELAX_DIAG: the measurement kernels do not read a record store in segments");
	const bool long_form = c->pad_long;
	if (long_form && diag) return fail(c, "MPCGPU_RELAX_DIAG: the measurement kernels do not read a record store in the long form");
	const char *merge_env = getenv("MPCGPU_RELAX_MERGE"); // "cxx": the compiler's code for the merge instead of the hand-scheduled one (A/B)
	const bool merge_cxx = merge_env && !strcmp(merge_env, "cxx");
	const void *fn = relax_band_select(false, g.use_win, merge_cxx, diag, seg, long_form, rp, 1, smem, c->stream);
	// (the two runtime queries cost a good fraction of a millisecond: once per context, kernel and LDS size — a -super7 run
	// relaxes 400 small stores on every worker context)
	int occ = 0;
	if (c->band_fn == fn && c->band_smem == smem) occ = c->band_occ;
	else {
		HIPCHK(c, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, (int)kBandThreads, smem) != hipSuccess || occ < 1) occ = 1;
		c->band_fn = fn; c->band_smem = smem; c->band_occ = occ;
		if (trace_on()) fprintf(stderr, "[mpcgpu] relax band: LDS attribute and occupancy of the kernel asked at %zu B (%d per CU)\n", smem, occ);
	}
	const u32 grid = std::max(std::min<u32>(ntiles, g.cus * (u32)occ), 1u);
	char kn[128];
	snprintf(kn, sizeof(kn), "relax_band_kernel<%u, %u, 2, %d, %s%s%s>", kBandThreads, g.kernel_slots, diag, seg ? "MpcRbSegmented<" : "",
		long_form ? "MpcRbLongCxx" : g.use_win ? (merge_cxx ? "MpcRbWinCxx" : "MpcRbWinAsm") : merge_cxx && !diag ? "MpcRbBlocksCxx" : "MpcRbBlocksAsm", seg ? "> " : "");
	c->relax_kernel_name = kn;
	if (trace_on()) {
		char ord[24] = "pairs";
		if (rp.by_rows) snprintf(ord, sizeof(ord), "blocks of %u rows", rp.by_rows);
		fprintf(stderr, "[mpcgpu] relax band: %s; lds=%zu B occ=%d grid=%u cell order=%s\n", c->tiles_desc.c_str(), smem, occ, grid, ord);
		fflush(stderr);
	}
	TimedSpan ts;
	if (span_begin(c, 3, &ts)) return 1;
	relax_band_select(true, g.use_win, merge_cxx, diag, seg, long_form, rp, grid, smem, c->stream);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts)) return 1;
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

// ---- whole-record tiles (relax_var_kernel)
struct VarFit { mpcgpu_ctx *c; u64 k0, k1; u32 max_slots; std::vector<u32> *leftover; bool too_big; };
// slots a tile needs: the cells of its pairs in [k0,k1), every pair rounded up to whole waves, in chunks of the workgroup's 1024 threads
static u32 var_tile_slots(const VarFit &vf, u32 x0, u32 nx, u32 y0, u32 ny)
{
	u64 cells = 0;
	for (u32 X = x0; X < x0 + nx; ++X)
		for (u32 Y = std::max(y0, X + 1); Y < y0 + ny; ++Y) {
			const u64 k = pair_pos(vf.c, X, Y);
			if (k >= vf.k0 && k < vf.k1) cells += ((u64)vf.c->all_nnz[k] + 63) & ~63ull;
		}
	return (u32)((cells + 1023) / 1024);
}
// a candidate tile whose cells fit the register slots goes to `tiles`; others are halved (Y first, then X); single pairs to the leftover list
static void var_emit_tile(VarFit &vf, const u32 *w, std::vector<u32> &tiles)
{
	const u32 slots = var_tile_slots(vf, w[0], w[1], w[2], w[3]);
	u32 a[6], b[6];
	if (slots == 0) return;
	if (slots <= vf.max_slots) tiles.insert(tiles.end(), w, w + 4);
	else if (halve_tile(w, false, a, b)) { var_emit_tile(vf, a, tiles); var_emit_tile(vf, b, tiles); }
	else if (vf.leftover) vf.leftover->insert(vf.leftover->end(), w, w + 4);
	else vf.too_big = true;
}
// Tiles of the primary geometry or the fallback out of a list of candidate tiles: a tile is kept when its cells fit the register slots and its
// records of one step, packed back to back, fit one staging buffer at EVERY step (the worst step of every tile is measured on
// the device); others are split (Y first, then X) and measured again. Single pairs that still do not fit go to `leftover`
// (when given: the fallback takes them) or fail the call.
static int var_build_tiles(mpcgpu_ctx *c, const StoreParams &sp, u64 k0, u64 k1, bool fallback, const std::vector<u32> &cand, std::vector<u32> &ok, std::vector<u32> *leftover)
{
	const u32 buf_bytes = var_buf_bytes(fallback);
	VarFit vf = {c, k0, k1, relax_slots(var_max_slots(fallback)), leftover, false};
	std::vector<u32> tiles;
	for (size_t t = 0; t + 3 < cand.size(); t += 4) { const u32 w[6] = {cand[t], cand[t + 1], cand[t + 2], cand[t + 3], 0, 0}; var_emit_tile(vf, w, tiles); }
	if (vf.too_big) return fail(c, "mpcgpu_cons_iter: a pair has more than %u stored cells (tile slot budget)", vf.max_slots * 1024);
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
			const u32 w[6] = {x0, nx, y0, ny, 0, 0};
			u32 a[6], b[6];
			if (fit[t] <= budget_blocks) { ok.insert(ok.end(), w, w + 4); continue; }
			++nsplit;
			if (halve_tile(w, false, a, b)) {
				if (var_tile_slots(vf, a[0], a[1], a[2], a[3])) next.insert(next.end(), a, a + 4);
				if (var_tile_slots(vf, b[0], b[1], b[2], b[3])) next.insert(next.end(), b, b + 4);
			}
			else if (leftover) leftover->insert(leftover->end(), {x0, nx, y0, ny});
			else return fail(c, "mpcgpu_cons_iter: the two records of pair (%u,%u) need %u bytes of LDS at some step, one staging buffer holds %u",
				x0, y0, fit[t] * 16, buf_bytes);
		}
		if (trace_on() && nsplit) { fprintf(stderr, "[mpcgpu] relax var: %u of %u tiles over the LDS budget (%u B), split\n", nsplit, nt, buf_bytes); fflush(stderr); }
		tiles.swap(next);
	}
	if (!tiles.empty()) return fail(c, "mpcgpu_cons_iter: tile splitting did not converge");
	return 0;
}
static std::string describe_var_tiles(const std::vector<u32> &ok)
{
	u32 hist[5][5] = {{0}};
	for (size_t t = 0; t + 3 < ok.size(); t += 4) hist[std::min(ok[t + 1], 4u)][std::min(ok[t + 3], 4u)]++;
	char b[256];
	int o = snprintf(b, sizeof(b), "%zu tiles:", ok.size() / 4);
	for (u32 a = 4; a >= 1; --a)
		for (u32 bb = 4; bb >= 1; --bb)
			if (hist[a][bb] && o < (int)sizeof(b) - 24) o += snprintf(b + o, sizeof(b) - o, " %ux%u x %u", a, bb, hist[a][bb]);
	return std::string(b);
}

int relax_var(mpcgpu_ctx *c, const StoreParams &sp, u64 k0, u64 k1)
{
	const u32 n = c->n;
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
		if (var_build_tiles(c, sp, k0, k1, false, cand, ok, c->var_mixed ? &left : nullptr)) return 1;
		if (!left.empty() && var_build_tiles(c, sp, k0, k1, true, left, ok2, nullptr)) return 1;
		c->tiles_desc = describe_var_tiles(ok);
		if (!ok2.empty()) c->tiles_desc += "; + 1 x 1024-thread workgroup per CU, 1 staging buffer of 160 KB for " + describe_var_tiles(ok2);
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

// mpcgpu_store.inc — builds the device store's record layouts (part of mpcgpu.cpp's translation unit): variable-size block records,
// window records and band tables (kernels_store.h, kernels_relaxb.h). The reference keeps one MySparseMx per pair (mysparsemx.h:6-98).

// ---- segments (StoreParams::pad_zbase). A record's start and a slab's end are 32-bit block indices inside their segment: a segment
// holds at most 2^32 - 1 blocks (64 GiB). MPCGPU_STORE_SEG_BLOCKS=<blocks> lowers that (a test hook: a store of a dozen short
// sequences then splits and runs the code a 70 GB store runs).
const u64 kStoreSegBlocksMax = 0xffffffffull;

// Cuts the n Z slabs of a record store — sizes: the n * n record sizes in blocks, Z-major — into the fewest runs of consecutive slabs
// of at most `limit` blocks each (greedy: a slab goes into the current run while it fits). z_first[g] = first Z of segment g,
// blocks[g] = its blocks. false: one slab alone is larger than the limit. The host-only planner behind mpcgpu_plan_store_segments.
bool plan_store_segments(u32 n, const u32 *sizes, u64 limit, std::vector<u32> &z_first, std::vector<u64> &blocks)
{
	z_first.assign(1, 0u);
	blocks.assign(1, 0ull);
	for (u32 Z = 0; Z < n; ++Z) {
		u64 slab = 0;
		for (u32 A = 0; A < n; ++A) slab += sizes[(u64)Z * n + A];
		if (slab > limit) return false;
		if (blocks.back() + slab > limit) { z_first.push_back(Z); blocks.push_back(0ull); }
		blocks.back() += slab;
	}
	return true;
}

u64 store_seg_limit()
{
	const char *e = getenv("MPCGPU_STORE_SEG_BLOCKS");
	const u64 v = (e && *e) ? strtoull(e, nullptr, 10) : 0ull;
	return (v == 0ull || v > kStoreSegBlocksMax) ? kStoreSegBlocksMax : v;
}

// off[b + 1] holds the size of record b on entry; on return off[b] = the block at which record b starts INSIDE ITS SEGMENT and
// zend[Z] = the block at which slab Z ends there (the end of a segment's last record is found nowhere else: the next table entry is
// the next segment's 0). One segment: the plain exclusive scan, off[n * n] = all blocks.
void segment_offsets(u32 n, std::vector<u32> &off, const std::vector<u32> &z_first, std::vector<u32> &zend)
{
	zend.resize(n);
	u64 run = 0;
	size_t g = 0;
	for (u32 Z = 0; Z < n; ++Z) {
		if (g + 1 < z_first.size() && Z == z_first[g + 1]) { ++g; run = 0; }
		for (u32 A = 0; A < n; ++A) {
			const u64 b = (u64)Z * n + A;
			const u32 sz = off[b + 1];
			off[b] = (u32)run;
			run += sz;
		}
		zend[Z] = (u32)run;
	}
	off[(u64)n * n] = (u32)run;
}

// what the context holds is large enough for this cut, allocation by allocation (DevBuf::ensure would then keep every one of them)
bool segments_held(const DevBuf &one, const SegStore &st, const std::vector<u64> &blocks)
{
	if (blocks.size() == 1) return one.cap >= std::max<u64>(blocks[0], 1) * 16;
	if (st.seg.size() != blocks.size()) return false;
	for (size_t g = 0; g < blocks.size(); ++g)
		if (st.seg[g].cap < std::max<u64>(blocks[g], 1) * 16) return false;
	return true;
}

// the segments' allocations (kept where they are large enough, as DevBuf::ensure does) and the two per-Z tables
int alloc_segments(mpcgpu_ctx *c, SegStore &st, const std::vector<u32> &z_first, const std::vector<u64> &blocks, const std::vector<u32> &zend)
{
	const u32 n = c->n;
	for (size_t g = blocks.size(); g < st.seg.size(); ++g) st.seg[g].release();
	st.seg.resize(blocks.size());
	std::vector<u64> zb(n);
	for (size_t g = 0; g < blocks.size(); ++g) {
		HIPCHK(c, st.seg[g].ensure(std::max<u64>(blocks[g], 1) * 16));
		const u32 z1 = g + 1 < blocks.size() ? z_first[g + 1] : n;
		for (u32 Z = z_first[g]; Z < z1; ++Z) zb[Z] = (u64)(uintptr_t)st.seg[g].p;
	}
	if (upload(c, st.zbase, zb) || upload(c, st.zend, zend)) return 1;
	HIPCHK(c, hipStreamSynchronize(c->stream)); // (the sources are locals)
	return 0;
}

// Builds the variable-size record store (rec_off table, records, entry positions). 0 = built (c->pad_var set), 1 = error,
// 2 = this run does not fit the layout's limits (the caller falls back to the fixed-size records / the gather kernel).
int build_var_store(mpcgpu_ctx *c)
{
	const u32 n = c->n;
	// MPCGPU_RELAX_LONG: the records' LONG form (kernels_store.h) — taken by itself exactly where the short form's field widths end (a
	// sequence above MPC_RV_MAXLEN, a record above 4095 blocks); 1: at any length (tests reach it with small shapes), 0: never (such
	// stores get the CSR slabs and the gather kernel, as they did before the long form existed: A/B and escape hatch)
	const int long_knob = env_int("MPCGPU_RELAX_LONG", -1);
	c->pad_long = false;
	if (c->max_len > MPC_RV_MAXLEN && (long_knob == 0 || c->max_len > MPC_RL_MAXLEN)) return 2;
	StoreParams sp0;
	fill_store_params(c, sp0);
	const u64 nn = (u64)n * n;
	HIPCHK(c, c->d_sizes.ensure(nn * 4));
	MPC_LAUNCH(var_size_kernel, (u32)std::min<u64>(nn, (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp0, c->d_sizes.as<u32>());
	HIPCHK(c, hipGetLastError());
	std::vector<u32> &off = c->v_off; // (kept: see mpcgpu_ctx)
	off.resize(nn + 1);
	HIPCHK(c, hipMemcpyAsync(off.data() + 1, c->d_sizes.p, nn * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	off[0] = 0;
	u32 max_rec = 0;
	u64 run = 0; // all blocks, in 64 bits: block offsets are 32-bit inside a SEGMENT (64 GB of records each)
	for (u64 b = 0; b < nn; ++b) { max_rec = std::max(max_rec, off[b + 1]); run += off[b + 1]; }
	if (max_rec > 4095u && long_knob == 0) return 2; // a block's distance field holds 16 bits of bytes
	const bool long_form = long_knob == 1 || c->max_len > MPC_RV_MAXLEN || max_rec > 4095u;
	if (long_form && (c->max_len > MPC_RL_MAXLEN || (u64)max_rec * 16 > 0xffffffffull)) return 2; // 16-bit columns, 32 bits of bytes
	const u64 seg_limit = store_seg_limit();
	std::vector<u32> seg_z, zend;
	std::vector<u64> seg_blocks;
	if (!plan_store_segments(n, off.data() + 1, seg_limit, seg_z, seg_blocks)) return 2; // one Z slab alone passes the limit (n * 4095 blocks: not below 2^20 sequences)
	const u32 nseg = (u32)seg_blocks.size();
	segment_offsets(n, off, seg_z, zend); // exclusive scan in place: off[b+1] holds size(b) on entry
	// whole-record tiles of relax_var_kernel (mpcgpu_relax.inc): the primary geometry (two 1024-thread workgroups per CU, 80 KB of
	// LDS each), plus a second launch of the fallback (one 1024-thread workgroup per CU with the whole 160 KB) for the pairs that do
	// not fit it — long or poorly aligned sequences: wide posterior rows, records of tens of KB (such runs end up with tiles of one
	// pair: two records of 20..40 KB per step for ~3 slots of cells); when a pair fits neither, not for whole-record tiles
	auto fits = [&](bool fallback) { // every single pair: its two records, and its cells
		return 2ull * max_rec * 16 <= var_buf_bytes(fallback) && (((u64)c->max_nnz + 63) & ~63ull) <= (u64)var_max_slots(fallback) * 1024u;
	};
	// (the long form is for band tiles only: relax_var_kernel keeps a cell's two row offsets inside the records in 16 bits each)
	const bool fits_primary = !long_form && fits(false), pairs_ok = !long_form && (fits_primary || fits(true));
	const char *tiles_mode = getenv("MPCGPU_RELAX_TILES"); // "pairs": whole-record tiles of relax_var_kernel only; "band": band tiles whatever the size
	// MPCGPU_RELAX_SMALL_PAIRS=<n> (default 0 = never; the drop-in binary sets 40): stores of <= n sequences whose pairs fit the
	// whole-record tiles take those. A shrub of -super7 (<= 32 sequences, 412 of them in a 10 000-sequence run) is relaxed in 0.3 ms
	// either way, but the band path builds window records and band tables and cuts its tiles on the device first: 4.6 ms of launches
	// and round trips per store against 0.06 (profiles/r10d_small_store_time.log) — the 0.7 s that run lost in round 4.
	const int small_n = env_int("MPCGPU_RELAX_SMALL_PAIRS", 0);
	// relax_var_kernel reads "the end of a run of records" as the next table entry and one base: a store in segments is for band tiles only
	const bool small_pairs = small_n > 0 && n <= (u32)small_n && fits_primary && !(tiles_mode && !strcmp(tiles_mode, "band")) && nseg == 1;
	const bool want_band = !(tiles_mode && !strcmp(tiles_mode, "pairs")) && !small_pairs && c->npairs < 0xffffffffull;
	if (nseg > 1 && tiles_mode && !strcmp(tiles_mode, "pairs"))
		return fail(c, "MPCGPU_RELAX_TILES=pairs: the whole-record tiles of relax_var_kernel do not read a record store in segments "
			"(%u segments of at most %llu blocks; band tiles do)", nseg, (u64)seg_limit);
	c->var_mixed = !fits_primary && pairs_ok;
	if (!pairs_ok && !want_band) return 2; // (with pairs_ok false, band tiles may still be an option: relax_band)
	if (nseg > 1 && !want_band) return 2;
	const u64 pos_bytes = (long_form ? 8 : 4) * std::max<u64>(c->total_entries, 1); // pos_f then pos_t: u16 each, u32 in the long form
	const u64 pad_bytes = run * 16 + pos_bytes;
	// the records of an earlier store are kept where this cut fits them allocation by allocation; otherwise they go BEFORE the
	// free-memory question is asked (a new cut of 70 GB beside the old one's segments would be refused, or fail in hipMalloc)
	const bool held = segments_held(c->d_pad, c->pad_seg, seg_blocks) && pos_bytes <= c->d_pos.cap;
	if (!segments_held(c->d_pad, c->pad_seg, seg_blocks)) { c->d_pad.release(); c->pad_seg.release(); }
	size_t freeb = 0, totb = 0;
	HIPCHK(c, hipMemGetInfo(&freeb, &totb));
	if (!(held || pad_bytes + ((u64)2 << 30) <= (u64)freeb)) return 2;
	c->d_rp.release(); c->d_ent.release(); c->d_mbase.release(); // slabs of an earlier run are not needed
	if (nseg == 1) {
		c->pad_seg.release();
		HIPCHK(c, c->d_pad.ensure(std::max<u64>(run, 1) * 16));
	} else { // every segment an allocation of its own (also: no single request of 70 GB)
		c->d_pad.release();
		if (alloc_segments(c, c->pad_seg, seg_z, seg_blocks, zend)) return 1;
	}
	HIPCHK(c, c->d_pos.ensure(pos_bytes));
	if (upload(c, c->d_rec_off, off)) return 1;
	HIPCHK(c, hipStreamSynchronize(c->stream)); // (the offsets live in the context: v_off; the wait orders the upload before the kernels that read the table)
	c->have_pad = true;
	c->pad_long = long_form;
	c->pad_lcap1 = c->max_len;
	c->var_max_rec_blocks = max_rec; c->var_total_blocks = run;
	c->tiles_k0 = c->tiles_k1 = ~0ull;
	{
		char b[512];
		snprintf(b, sizeof(b), "variable-size dense records: %u x %u records, %.2f GB, mean %.0f B, largest %u B; relax_var_kernel, 2 x 1024-thread workgroups per CU, 1 staging buffer of %u B",
			n, n, (double)run * 16 / 1e9, (double)run * 16 / (double)nn, max_rec * 16, var_buf_bytes(false));
		c->store_desc = b;
		if (c->var_mixed) c->store_desc += " (pairs whose records do not fit it: 1 x 1024-thread workgroup per CU with 160 KB, second launch)";
		if (nseg > 1) c->store_desc += " in " + std::to_string(nseg) + " segments of whole Z slabs";
		c->tiles_desc.clear(); c->relax_kernel_name.clear(); c->relax_fallback = false;
	}
	// band tables for relax_band_kernel (kernels_relaxb.h; MPCGPU_RELAX_TILES=pairs: whole-record tiles of relax_var_kernel only)
	c->band_ok = false;
	c->btiles_k0 = c->btiles_k1 = ~0ull;
	{
		const u32 nb1 = (c->max_len + MPC_RB_HB - 1) / MPC_RB_HB + 1;
		const u64 tab_bytes = (nn + 2 * c->npairs + 2ull * n) * nb1 * 4;
		size_t free2 = 0, tot2 = 0;
		HIPCHK(c, hipMemGetInfo(&free2, &tot2));
		if (want_band && (c->d_ovf_off.cap >= nn * nb1 * 4 || tab_bytes + ((u64)1 << 30) <= (u64)free2)) {
			HIPCHK(c, c->d_ovf_off.ensure(nn * nb1 * 4));
			HIPCHK(c, c->d_cell_off.ensure(std::max<u64>(c->npairs, 1) * nb1 * 4));
			HIPCHK(c, c->d_yr.ensure(std::max<u64>(c->npairs, 1) * nb1 * 4));
			HIPCHK(c, c->d_ovf_sum.ensure(3ull * n * nb1 * 4)); // sums, largest and smallest prefix over Z (ovf_stats_kernel)
			HIPCHK(c, c->d_ovf_maxc.ensure((u64)n * nb1 * 4));
			c->band_ok = true;
			c->band_nb1 = nb1;
			char b[256];
			snprintf(b, sizeof(b), "variable-size dense records: %u x %u records, %.2f GB, mean %.0f B, largest %u B, band index of %u rows",
				n, n, (double)run * 16 / 1e9, (double)run * 16 / (double)nn, max_rec * 16, (unsigned)MPC_RB_HB);
			c->store_desc = b; // (the tiles and the kernel are described when the first relax has cut them: relax_band)
			if (long_form) c->store_desc += ", band-long (32-bit block distances and entry positions)";
			if (nseg > 1) c->store_desc += ", in " + std::to_string(nseg) + " segments of whole Z slabs";
		}
		if (!c->band_ok && (!pairs_ok || nseg > 1)) { c->have_pad = false; c->pad_long = false; return 2; }
		c->var_pairs_ok = pairs_ok && nseg == 1;
	}
	StoreParams sp;
	fill_store_params(c, sp);
	if (trace_on()) {
		fprintf(stderr, "[mpcgpu] store: variable-size dense records, %u x %u records, %.2f GB (mean %.0f B, largest %u B)%s\n", n, n,
			(double)run * 16 / 1e9, (double)run * 16 / (double)nn, max_rec * 16, c->var_mixed ? ", relax_var fallback for the largest pairs" : "");
		fflush(stderr);
	}
	TimedSpan ts;
	if (span_begin(c, 2, &ts)) return 1;
	if (long_form) {
		// the two row scans of a workgroup in global scratch (a row sequence of 65 534 positions: 512 KB), so fewer workgroups in flight;
		// the record sizes have been read back: their buffer is free
		const u32 grid = (u32)std::min<u64>(nn, (u64)c->prop.multiProcessorCount * 4);
		HIPCHK(c, c->d_sizes.ensure(std::max<u64>((u64)grid * 2 * std::max(sp.lcap1, 1u) * 4, nn * 4)));
		MPC_LAUNCH(var_build_long_kernel, grid, 64, 0, c->stream, sp, c->d_sizes.as<u32>());
	}
	else MPC_LAUNCH(var_build_kernel, (u32)std::min<u64>(nn, (u64)c->prop.multiProcessorCount * 32), 64, (size_t)std::max(sp.lcap1, 1u) * 8, c->stream, sp);
	HIPCHK(c, hipGetLastError());
	// ---- window records (the Y operand of the direct-index merge): a second copy of the store whose rows are looked up by column.
	// Built when the rows are narrow — the windows then cost about what the blocks cost (1000 x L~400: 93 % of the rows span <= 4
	// columns); wide-row data (rdrp: half of the rows span >= 40 columns) keeps the walk of two block lists. MPCGPU_RELAX_FORM=walk: never.
	c->win_ok = false;
	{
		const char *form = getenv("MPCGPU_RELAX_FORM");
		// (the long form keeps block records for the Y operand: a window descriptor has 12 bits of column and 15 of value offset)
		if (c->band_ok && !long_form && !(form && !strcmp(form, "walk"))) {
			HIPCHK(c, c->d_sizes.ensure(nn * 4));
			HIPCHK(c, c->d_tilefit.ensure(nn * 4)); // (scratch: value dwords per record)
			HIPCHK(c, c->d_wflag.ensure(4));
			HIPCHK(c, hipMemsetAsync(c->d_wflag.p, 0, 4, c->stream));
			MPC_LAUNCH(win_size_kernel, (u32)std::min<u64>(nn, (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp, c->d_sizes.as<u32>(),
				c->d_tilefit.as<u32>(), c->d_wflag.as<u32>());
			HIPCHK(c, hipGetLastError());
			std::vector<u32> &woff = c->v_woff; // (kept: see mpcgpu_ctx)
			woff.resize(nn + 1);
			u32 wide = 0;
			HIPCHK(c, hipMemcpyAsync(woff.data() + 1, c->d_sizes.p, nn * 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(c, hipMemcpyAsync(&wide, c->d_wflag.p, 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(c, hipStreamSynchronize(c->stream));
			woff[0] = 0;
			u64 wrun = 0;
			for (u64 b = 0; b < nn; ++b) wrun += woff[b + 1];
			// the window records get a segmentation of their own (their slabs differ in size from the blocks')
			std::vector<u32> wseg_z, wzend;
			std::vector<u64> wseg_blocks;
			const bool wplan = plan_store_segments(n, woff.data() + 1, seg_limit, wseg_z, wseg_blocks);
			const u32 nwseg = wplan ? (u32)wseg_blocks.size() : 0u;
			if (wplan) segment_offsets(n, woff, wseg_z, wzend);
			const double ratio = (double)wrun / (double)std::max<u64>(run, 1);
			const double max_ratio = (double)env_int("MPCGPU_RELAX_WIN_PCT", 125) / 100.0;
			const bool wheld = wplan && segments_held(c->d_win, c->win_seg, wseg_blocks);
			if (!wheld) { c->d_win.release(); c->win_seg.release(); } // (as for the block records: before the free-memory question)
			size_t free3 = 0, tot3 = 0;
			HIPCHK(c, hipMemGetInfo(&free3, &tot3));
			const u64 need = wrun * 16 + 4 * std::max<u64>(c->total_entries, 1) + nn * c->band_nb1 * 4;
			if (!wide && wplan && ratio <= max_ratio && (wheld || need + ((u64)1 << 30) <= (u64)free3)) {
				if (nwseg == 1) {
					c->win_seg.release();
					HIPCHK(c, c->d_win.ensure(std::max<u64>(wrun, 1) * 16));
				} else {
					c->d_win.release();
					if (alloc_segments(c, c->win_seg, wseg_z, wseg_blocks, wzend)) return 1;
				}
				HIPCHK(c, c->d_pos_w.ensure(4 * std::max<u64>(c->total_entries, 1)));
				HIPCHK(c, c->d_wv_off.ensure(nn * c->band_nb1 * 4));
				HIPCHK(c, c->d_wsum.ensure(3ull * n * c->band_nb1 * 4));
				HIPCHK(c, c->d_wmaxc.ensure((u64)n * c->band_nb1 * 4));
				if (upload(c, c->d_wrec_off, woff)) return 1;
				HIPCHK(c, hipStreamSynchronize(c->stream)); // (as above: the offsets live in the context, v_woff)
				c->win_ok = true;
				c->win_total_blocks = wrun;
				fill_store_params(c, sp);
				MPC_LAUNCH(win_build_kernel, (u32)std::min<u64>(nn, (u64)c->prop.multiProcessorCount * 32), 64, (size_t)(std::max(sp.lcap1, 1u) + 1) * 4, c->stream, sp);
				HIPCHK(c, hipGetLastError());
				MPC_LAUNCH(win_pos_kernel, (u32)std::min<u64>(std::max<u64>(c->npairs, 1), (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp);
				HIPCHK(c, hipGetLastError());
				MPC_LAUNCH(ovf_stats_kernel, std::min<u32>(n, (u32)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp, c->d_wv_off.as<u32>(), c->band_nb1,
					c->d_wsum.as<u32>(), c->d_wmaxc.as<u32>(), 1);
				HIPCHK(c, hipGetLastError());
				char wb[160];
				snprintf(wb, sizeof(wb), " + window records for the Y operand (%.2f GB, %.0f %% of the blocks)", (double)wrun * 16 / 1e9, 100.0 * ratio);
				c->store_desc += wb;
				if (nwseg > 1) c->store_desc += " in " + std::to_string(nwseg) + " segments";
			} else {
				if (trace_on())
					fprintf(stderr, "[mpcgpu] store: no window records (%s; they would take %.0f %% of the block records' %.2f GB)\n",
						wide ? "a record's windows exceed 65535 values" : !wplan ? "one Z slab of them passes the segment limit" : ratio > max_ratio ? "rows too wide" : "device memory",
						100.0 * ratio, (double)run * 16 / 1e9);
			}
		}
	}
	if (!c->win_ok) release_windows(c); // none for this store (the walk, no band tables, too wide, no room): an earlier store's — tens of GB — go
	if (c->band_ok) {
		MPC_LAUNCH(band_index_kernel, (u32)std::min<u64>(std::max<u64>(c->npairs, 1), (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp, c->band_nb1,
			c->d_cell_off.as<u32>(), c->d_yr.as<u32>());
		HIPCHK(c, hipGetLastError());
		MPC_LAUNCH(ovf_stats_kernel, std::min<u32>(n, (u32)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp, c->d_ovf_off.as<u32>(), c->band_nb1,
			c->d_ovf_sum.as<u32>(), c->d_ovf_maxc.as<u32>(), 0);
		HIPCHK(c, hipGetLastError());
	}
	if (span_end(c, &ts)) return 1;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}


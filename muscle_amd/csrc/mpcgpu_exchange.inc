// mpcgpu_exchange.inc — shards, store import (whole / partial), values, relax + commit entry points and the result getters (part of
// mpcgpu.cpp's translation unit). Reference: SURVEY.md 8e (the exchange), consflat.cpp:5-23 (ConsIter and its buffer swap).
int mpcgpu_shard_info(mpcgpu_ctx *c, uint64_t *bytes, void **dev_ptr)
{
	if (!c) return 1;
	if (!c->have_shard) return fail(c, "mpcgpu_shard_info: no shard (call mpcgpu_calc_posteriors)");
	if (bytes) *bytes = c->shard_bytes;
	if (dev_ptr) *dev_ptr = c->d_shard.p;
	return 0;
}

int mpcgpu_shard_entries(mpcgpu_ctx *c, uint64_t *entries)
{
	if (!c) return 1;
	if (!c->have_shard) return fail(c, "mpcgpu_shard_entries: no shard (call mpcgpu_calc_posteriors)");
	u64 sum = 0;
	for (u32 v : c->sh_nnz) sum += v;
	if (entries) *entries = sum;
	return 0;
}

int mpcgpu_shard_export(mpcgpu_ctx *c, void *dev_dst)
{
	if (!c) return 1;
	if (!c->have_shard) return fail(c, "mpcgpu_shard_export: no shard (call mpcgpu_calc_posteriors)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(dev_dst, c->d_shard.p, c->shard_bytes, hipMemcpyDeviceToDevice, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

int mpcgpu_store_import_part(mpcgpu_ctx *c, uint32_t nshards, const uint64_t *k0, const uint64_t *k1, const uint64_t *bytes,
	const uint64_t *offsets, void *dev_all, uint64_t own_k0, uint64_t own_k1)
{
	if (!c) return 1;
	if (c->n == 0) return fail(c, "mpcgpu_store_import: call mpcgpu_set_seqs first");
	if (own_k0 > own_k1 || own_k1 > c->npairs) return fail(c, "mpcgpu_store_import_part: bad own range [%llu,%llu)", (u64)own_k0, (u64)own_k1);
	// where each shard lies in dev_all (offsets[s]; null: back to back in the order given); sorted by offset, no two may overlap. Checked
	// before anything changes: a rejected call leaves the current store as it was
	std::vector<u64> at(nshards, 0);
	{
		u64 run = 0;
		for (u32 s = 0; s < nshards; ++s) { at[s] = offsets ? offsets[s] : run; run += bytes[s]; if (at[s] & 3) return fail(c, "mpcgpu_store_import: shard %u is not word-aligned", s); }
		std::vector<u32> by_at(nshards);
		for (u32 s = 0; s < nshards; ++s) by_at[s] = s;
		std::sort(by_at.begin(), by_at.end(), [&](u32 a, u32 b) { return at[a] < at[b]; });
		for (u32 q = 0; q + 1 < nshards; ++q) {
			const u32 s = by_at[q], t = by_at[q + 1];
			if (bytes[s] > at[t] - at[s])
				return fail(c, "mpcgpu_store_import_part: shards %u and %u overlap ([%llu,+%llu) and [%llu,+%llu) bytes)", s, t, (u64)at[s], (u64)bytes[s], (u64)at[t], (u64)bytes[t]);
		}
	}
	HIPCHK(c, hipSetDevice(c->device));
	++c->epoch;
	c->have_store = false;
	c->tiles_k0 = c->tiles_k1 = ~0ull;
	const u32 n = c->n;
	// the forward planes of a row-block stage A may hold a large share of the device: give them back if the store (roughly four
	// times the packed records) could not be allocated next to them
	if (c->d_fm.cap > (8ull << 30)) {
		u64 packed_bytes = 0;
		for (u32 s = 0; s < nshards; ++s) packed_bytes += bytes[s];
		size_t free_now = 0, total_now = 0;
		HIPCHK(c, hipMemGetInfo(&free_now, &total_now));
		if ((u64)free_now < 5 * packed_bytes + (4ull << 30)) c->d_fm.release();
	}
	// ---- read shard headers, check coverage. The shards may lie anywhere in dev_all (offsets[s]; null: back to back in the order
	// given) and come in any order: sorted by their first position they must tile [0, pairs)
	std::vector<u32> by_k(nshards);
	for (u32 s = 0; s < nshards; ++s) by_k[s] = s;
	std::sort(by_k.begin(), by_k.end(), [&](u32 a, u32 b) { return k0[a] != k0[b] ? k0[a] < k0[b] : k1[a] < k1[b]; });
	c->all_nnz.assign(c->npairs, 0);
	c->all_ea.assign(c->npairs, 0.0f);
	c->h_pbase.assign(c->npairs + 1, 0);
	c->h_vbase.assign(c->npairs + 1, 0);
	u64 expect = 0, end_max = 0;
	// all headers are read back with ONE wait (a pair-sharded run with stage A in pieces imports world x pieces shards)
	std::vector<u64> hoff(nshards + 1, 0);
	for (u32 s = 0; s < nshards; ++s) {
		if (k1[s] < k0[s] || k1[s] > c->npairs) return fail(c, "mpcgpu_store_import: shard %u is [%llu,%llu)", s, (u64)k0[s], (u64)k1[s]);
		const u64 hdr = shard_header_bytes(k1[s] - k0[s]);
		if (bytes[s] < hdr) return fail(c, "mpcgpu_store_import: shard %u too small", s);
		hoff[s + 1] = hoff[s] + hdr;
	}
	std::vector<u8> &h = c->v_hdr; // (kept: see mpcgpu_ctx — 8 bytes per pair)
	h.resize(hoff[nshards]);
	for (u32 s = 0; s < nshards; ++s)
		HIPCHK(c, hipMemcpyAsync(h.data() + hoff[s], (const u8 *)dev_all + at[s], hoff[s + 1] - hoff[s], hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	for (u32 q = 0; q < nshards; ++q) {
		const u32 s = by_k[q];
		if (k0[s] != expect)
			return fail(c, "mpcgpu_store_import: shards must tile [0,%llu) (shard %u is [%llu,%llu), expected one that starts at %llu)",
				(u64)c->npairs, s, (u64)k0[s], (u64)k1[s], (u64)expect);
		const u64 np = k1[s] - k0[s];
		const u64 hdr = hoff[s + 1] - hoff[s];
		const u8 *hs = h.data() + hoff[s];
		u64 h2[2];
		memcpy(h2, hs, 16);
		if (h2[0] != np || hdr + h2[1] * 4 != bytes[s])
			return fail(c, "mpcgpu_store_import: shard %u header mismatch (pairs %llu vs %llu, bytes %llu vs %llu)", s,
				(u64)h2[0], (u64)np, (u64)(hdr + h2[1] * 4), (u64)bytes[s]);
		if (np) {
			memcpy(&c->all_nnz[k0[s]], hs + 16, np * 4);
			memcpy(&c->all_ea[k0[s]], hs + 16 + np * 4, np * 4);
		}
		u64 w = (at[s] + hdr) / 4;
		for (u64 k = k0[s]; k < k1[s]; ++k) {
			c->h_pbase[k] = w;
			w += rec_words(c->len[c->h_pair_x[k]], c->len[c->h_pair_y[k]], c->all_nnz[k]);
		}
		if (w * 4 != at[s] + bytes[s]) return fail(c, "mpcgpu_store_import: shard %u record sizes do not add up", s);
		end_max = std::max(end_max, at[s] + bytes[s]);
		expect = k1[s];
	}
	if (expect != c->npairs) return fail(c, "mpcgpu_store_import: shards cover %llu of %llu pairs", (u64)expect, (u64)c->npairs);
	c->h_pbase[c->npairs] = end_max / 4; // (a sentinel only: a pair's record length follows from its lengths and its entry count)
	for (u64 k = 0; k < c->npairs; ++k) c->h_vbase[k + 1] = c->h_vbase[k] + c->all_nnz[k];
	c->total_entries = c->h_vbase[c->npairs];
	c->max_nnz = 0;
	for (u64 k = 0; k < c->npairs; ++k) c->max_nnz = std::max(c->max_nnz, c->all_nnz[k]);
	c->max_len = 0;
	for (u32 i = 0; i < n; ++i) c->max_len = std::max(c->max_len, c->len[i]);
	c->st_packed = (const u32 *)dev_all;
	HIPCHK(c, c->d_vnext.ensure(std::max<u64>(c->total_entries, 1) * 4));
	if (upload(c, c->d_pbase, c->h_pbase) || upload(c, c->d_vbase, c->h_vbase)) return 1;
	// ---- a PARTIAL store: this context relaxes the positions [own_k0, own_k1) only, so it needs the records (A, Z) of the
	// sequences A those pairs touch and of no other (a rank of a block-partitioned run: the sequences of its blocks — half of the
	// store at 8 ranks). Everything per pair (packed records, values) stays complete.
	c->own_k0 = own_k0; c->own_k1 = own_k1;
	c->packed_stale = false;
	c->lazy_ranges.clear();
	c->partial = !(own_k0 == 0 && own_k1 == c->npairs);
	if (c->partial) {
		c->need.assign(n, 0);
		for (u64 k = own_k0; k < own_k1; ++k) { c->need[c->h_pair_x[k]] = 1; c->need[c->h_pair_y[k]] = 1; }
		u32 cnt = 0;
		for (u32 i = 0; i < n; ++i) cnt += c->need[i];
		if (cnt == n) c->partial = false; // (the rank's pairs touch every sequence: nothing to leave out)
		else if (upload(c, c->d_need, c->need)) return 1;
	}
	// ---- layout for relax: padded records + LDS-tiled kernel when a tile fits the LDS and the
	// records fit HBM; otherwise compact slabs + the gather kernel (MPCGPU_RELAX=gather forces it).
	// Both are device paths with identical results.
	c->have_pad = false;
	{
		// variable-size dense records + the LDS-tiled kernels (sequences longer than 4095 or records of more than 4095 blocks: the
		// records' long form, band tiles only); a run beyond that layout's limits (a band that no LDS holds, ...) gets compact CSR
		// slabs + the gather kernel
		// (MPCGPU_RELAX=gather forces it). Both are device paths with identical results.
		const char *mode = getenv("MPCGPU_RELAX");
		if (!(mode && !strcmp(mode, "gather"))) {
			const int rc = build_var_store(c);
			if (rc == 1) return 1;
			if (rc == 0) { c->have_store = true; return 0; }
		}
	}
	return build_slab_store(c);
}

int mpcgpu_store_import(mpcgpu_ctx *c, uint32_t nshards, const uint64_t *k0, const uint64_t *k1,
	const uint64_t *bytes, void *dev_all)
{
	if (!c) return 1;
	return mpcgpu_store_import_part(c, nshards, k0, k1, bytes, nullptr, dev_all, 0, c->npairs);
}

int mpcgpu_store_complete(mpcgpu_ctx *c)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_store_complete: no store");
	HIPCHK(c, hipSetDevice(c->device));
	if (refresh_packed(c)) return 1;
	if (!c->partial) { c->own_k0 = 0; c->own_k1 = c->npairs; return 0; }
	// the packed records hold the current values (every commit writes them): the records of ALL sequences are built from them
	c->partial = false;
	c->own_k0 = 0; c->own_k1 = c->npairs;
	c->have_store = false;
	c->tiles_k0 = c->tiles_k1 = ~0ull;
	const int rc = build_var_store(c);
	if (rc == 1) return 1;
	if (rc == 0) { c->have_store = true; return 0; }
	return build_slab_store(c);
}

int mpcgpu_build_store(mpcgpu_ctx *c)
{
	if (!c) return 1;
	if (!c->have_shard || c->shard_is_list || c->sh_k0 != 0 || c->sh_k1 != c->npairs)
		return fail(c, "mpcgpu_build_store: needs this context's shard to cover all pairs "
			"(multi-GPU callers use mpcgpu_store_import)");
	const uint64_t k0 = 0, k1 = c->npairs, bytes = c->shard_bytes;
	return mpcgpu_store_import(c, 1, &k0, &k1, &bytes, c->d_shard.p);
}

int mpcgpu_values_info(mpcgpu_ctx *c, void **dev_ptr, uint64_t *total_count)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_values_info: no store");
	if (dev_ptr) *dev_ptr = c->d_vnext.p;
	if (total_count) *total_count = c->total_entries;
	return 0;
}

int mpcgpu_values_slice(mpcgpu_ctx *c, uint64_t k0, uint64_t k1, uint64_t *first, uint64_t *count)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_values_slice: no store");
	if (k0 > k1 || k1 > c->npairs) return fail(c, "mpcgpu_values_slice: bad pair range");
	if (first) *first = c->h_vbase[k0];
	if (count) *count = c->h_vbase[k1] - c->h_vbase[k0];
	return 0;
}

int mpcgpu_values_export(mpcgpu_ctx *c, uint64_t first, uint64_t count, void *dev_dst)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_values_export: no store");
	if (count > c->total_entries || first > c->total_entries - count) return fail(c, "mpcgpu_values_export: range out of bounds");
	HIPCHK(c, hipSetDevice(c->device));
	if (count)
		HIPCHK(c, hipMemcpyAsync(dev_dst, c->d_vnext.as<float>() + first, count * 4, hipMemcpyDeviceToDevice, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

int mpcgpu_values_import(mpcgpu_ctx *c, uint64_t first, uint64_t count, const void *dev_src)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_values_import: no store");
	if (count > c->total_entries || first > c->total_entries - count) return fail(c, "mpcgpu_values_import: range out of bounds");
	HIPCHK(c, hipSetDevice(c->device));
	++c->epoch;
	if (count)
		HIPCHK(c, hipMemcpyAsync(c->d_vnext.as<float>() + first, dev_src, count * 4, hipMemcpyDeviceToDevice, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

int mpcgpu_cons_iter(mpcgpu_ctx *c, uint64_t k0, uint64_t k1)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_cons_iter: no store (call mpcgpu_build_store / mpcgpu_store_import)");
	if (k0 > k1 || k1 > c->npairs) return fail(c, "mpcgpu_cons_iter: bad pair range");
	if (c->partial && k0 != k1 && (k0 < c->own_k0 || k1 > c->own_k1))
		return fail(c, "mpcgpu_cons_iter: [%llu,%llu) is outside the range [%llu,%llu) this partial store was imported for (mpcgpu_store_import_part)",
			(u64)k0, (u64)k1, (u64)c->own_k0, (u64)c->own_k1);
	HIPCHK(c, hipSetDevice(c->device));
	++c->epoch;
	const u64 cnt = c->h_vbase[k1] - c->h_vbase[k0];
	c->work_entry_z = cnt * c->n;
	if (cnt == 0) return 0;
	StoreParams sp;
	fill_store_params(c, sp);
	if (c->have_pad) {
		if (c->band_ok) {
			int r = relax_band(c, sp, k0, k1);
			if (r == 2 && c->win_ok) {
				// no band fits with the Y rows as windows (one wide row can be most of the LDS): the same tiles with the Y rows as block
				// lists, i.e. the two-list walk; the window records are dropped
				if (trace_on()) fprintf(stderr, "[mpcgpu] relax: no band tile fits with window records: windows dropped, the walk is cut\n");
				release_windows(c);
				{ const size_t at = c->store_desc.find(" + window records"); if (at != std::string::npos) c->store_desc.erase(at); }
				c->btiles_k0 = c->btiles_k1 = ~0ull;
				fill_store_params(c, sp);
				r = relax_band(c, sp, k0, k1);
			}
			if (r != 2) return r;
			if (trace_on()) fprintf(stderr, "[mpcgpu] relax: no band tile fits: %s from here on\n", c->var_pairs_ok ? "whole-record tiles" : "CSR slabs");
			c->band_ok = false; // this store's rows do not cut into band tiles that fit: whole-record tiles from here on
		}
		if (c->var_pairs_ok) return relax_var(c, sp, k0, k1); // (never a store in segments: build_var_store)
		if (build_slab_store(c)) return 1; // neither: CSR slabs + the gather kernel (same results)
		fill_store_params(c, sp);
	}
	TimedSpan ts;
	if (span_begin(c, 3, &ts)) return 1;
	const u32 block = 256;
	const u64 blocks = (cnt + block - 1) / block;
	MPC_LAUNCH(relax_kernel, (u32)std::min<u64>(blocks, (u64)c->prop.multiProcessorCount * 64), block, 0, c->stream, sp,
		(u64)k0, (u64)k1);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts)) return 1;
	return 0;
}

int mpcgpu_cons_commit_range(mpcgpu_ctx *c, uint64_t first, uint64_t count)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_cons_commit: no store");
	if (count > c->total_entries || first > c->total_entries - count) return fail(c, "mpcgpu_cons_commit_range: range out of bounds");
	HIPCHK(c, hipSetDevice(c->device));
	++c->epoch;
	if (count == 0) return 0;
	StoreParams sp;
	fill_store_params(c, sp);
	TimedSpan ts;
	if (span_begin(c, 4, &ts)) return 1;
	const u32 block = 256;
	const u64 blocks = (count + block - 1) / block;
	const u32 grid = (u32)std::min<u64>(blocks, (u64)c->prop.multiProcessorCount * 64);
	if (c->have_pad) {
		// one wave per pair (kernels_store.h: commit_pairs_kernel): the pairs whose entries meet [first, first + count)
		const u64 ka = (u64)(std::upper_bound(c->h_vbase.begin(), c->h_vbase.end(), (u64)first) - c->h_vbase.begin()) - 1;
		const u64 kb = (u64)(std::lower_bound(c->h_vbase.begin(), c->h_vbase.end(), (u64)(first + count)) - c->h_vbase.begin());
		// a context that relaxes a part of the pairs only (a rank of a sharded run) writes the packed records of ITS pairs — what its
		// relax reads — and leaves the others' to refresh_packed (whoever reads them asks for it)
		const bool lazy = !(c->own_k0 == 0 && c->own_k1 == c->npairs);
		if (lazy) {
			c->packed_stale = true;
			// remember the range (merged with what is there: an iteration commits the same three ranges again)
			std::vector<std::pair<u64, u64> > &L = c->lazy_ranges;
			L.push_back(std::make_pair((u64)first, (u64)(first + count)));
			std::sort(L.begin(), L.end());
			size_t w = 0;
			for (size_t q = 1; q < L.size(); ++q) {
				if (L[q].first <= L[w].second) L[w].second = std::max(L[w].second, L[q].second);
				else L[++w] = L[q];
			}
			L.resize(w + 1);
		}
		const u64 pairs = std::min<u64>(kb, c->npairs) - ka;
		if (c->pad_long) // the record store's long form: 32-bit entry positions
			MPC_LAUNCH(commit_pairs_long_kernel, (u32)std::min<u64>(std::max<u64>(pairs, 1), (u64)c->prop.multiProcessorCount * 64), 64, 0, c->stream, sp, ka,
				std::min<u64>(kb, c->npairs), (u64)first, (u64)(first + count), c->own_k0, c->own_k1, lazy ? 1 : 0);
		else
		MPC_LAUNCH(commit_pairs_kernel, (u32)std::min<u64>(std::max<u64>(pairs, 1), (u64)c->prop.multiProcessorCount * 64), 64, 0, c->stream, sp, ka,
			std::min<u64>(kb, c->npairs), (u64)first, (u64)(first + count), c->own_k0, c->own_k1, lazy ? 1 : 0);
	}
	else MPC_LAUNCH(commit_kernel, grid, block, 0, c->stream, sp, (u64)first, (u64)(first + count));
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts)) return 1;
	return 0;
}

int mpcgpu_cons_commit(mpcgpu_ctx *c)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_cons_commit: no store");
	return mpcgpu_cons_commit_range(c, 0, c->total_entries);
}

// The getters speak MPCFlat::InitPairs pair numbers (mpcflat.cpp:145-155) whatever order the context keeps its pairs in
// (mpcgpu_set_pair_order): position of InitPairs pair k
static inline u64 pos_of(const mpcgpu_ctx *c, u64 k) { return c->ext2pos.empty() ? k : (u64)c->ext2pos[k]; }

int mpcgpu_get_ea(mpcgpu_ctx *c, uint64_t k0, uint64_t k1, float *ea)
{
	if (!c) return 1;
	if (k0 > k1 || k1 > c->npairs) return fail(c, "mpcgpu_get_ea: bad pair range");
	const bool shard_ok = c->have_shard && !c->shard_is_list;
	if (c->ext2pos.empty()) {
		if (c->have_store) { memcpy(ea, &c->all_ea[k0], (k1 - k0) * 4); return 0; }
		if (shard_ok && k0 >= c->sh_k0 && k1 <= c->sh_k1) { memcpy(ea, &c->sh_ea[k0 - c->sh_k0], (k1 - k0) * 4); return 0; }
		return fail(c, "mpcgpu_get_ea: range [%llu,%llu) not available", (u64)k0, (u64)k1);
	}
	for (u64 k = k0; k < k1; ++k) {
		const u64 q = pos_of(c, k);
		if (c->have_store) ea[k - k0] = c->all_ea[q];
		else if (shard_ok && q >= c->sh_k0 && q < c->sh_k1) ea[k - k0] = c->sh_ea[q - c->sh_k0];
		else return fail(c, "mpcgpu_get_ea: pair %llu not available", (u64)k);
	}
	return 0;
}

int mpcgpu_get_nnz(mpcgpu_ctx *c, uint64_t k0, uint64_t k1, uint32_t *nnz)
{
	if (!c) return 1;
	if (k0 > k1 || k1 > c->npairs) return fail(c, "mpcgpu_get_nnz: bad pair range");
	const bool shard_ok = c->have_shard && !c->shard_is_list;
	if (c->ext2pos.empty()) {
		if (c->have_store) { memcpy(nnz, &c->all_nnz[k0], (k1 - k0) * 4); return 0; }
		if (shard_ok && k0 >= c->sh_k0 && k1 <= c->sh_k1) { memcpy(nnz, &c->sh_nnz[k0 - c->sh_k0], (k1 - k0) * 4); return 0; }
		return fail(c, "mpcgpu_get_nnz: range [%llu,%llu) not available", (u64)k0, (u64)k1);
	}
	for (u64 k = k0; k < k1; ++k) {
		const u64 q = pos_of(c, k);
		if (c->have_store) nnz[k - k0] = c->all_nnz[q];
		else if (shard_ok && q >= c->sh_k0 && q < c->sh_k1) nnz[k - k0] = c->sh_nnz[q - c->sh_k0];
		else return fail(c, "mpcgpu_get_nnz: pair %llu not available", (u64)k);
	}
	return 0;
}

int mpcgpu_get_sparse_range(mpcgpu_ctx *c, uint64_t k0, uint64_t k1, uint32_t *offsets, void *values)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_get_sparse_range: no store (call mpcgpu_build_store / mpcgpu_store_import)");
	if (k0 > k1 || k1 > c->npairs) return fail(c, "mpcgpu_get_sparse_range: bad pair range");
	if (k0 == k1) return 0;
	HIPCHK(c, hipSetDevice(c->device));
	if (refresh_packed(c)) return 1;
	const bool listed = !c->ext2pos.empty(); // a custom pair order: the InitPairs range is a list of positions
	std::vector<u64> offbase(k1 - k0), valbase, klist;
	if (listed) { valbase.resize(k1 - k0); klist.resize(k1 - k0); }
	u64 o = 0, nval = 0;
	for (u64 k = k0; k < k1; ++k) {
		const u64 q = pos_of(c, k);
		offbase[k - k0] = o; o += c->len[c->h_pair_x[q]] + 1;
		if (listed) { klist[k - k0] = q; valbase[k - k0] = nval; }
		nval += c->all_nnz[q];
	}
	HIPCHK(c, c->d_exp_off.ensure(o * 4));
	HIPCHK(c, c->d_exp_val.ensure(std::max<u64>(nval, 1) * 8));
	if (upload(c, c->d_exp_offbase, offbase)) return 1;
	if (listed && (upload(c, c->d_exp_klist, klist) || upload(c, c->d_exp_valbase, valbase))) return 1;
	StoreParams sp;
	fill_store_params(c, sp);
	MPC_LAUNCH(export_kernel, (u32)std::min<u64>(k1 - k0, (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, sp,
		(u64)(listed ? 0 : k0), (u64)(listed ? k1 - k0 : k1), c->d_exp_offbase.as<u64>(), c->d_exp_off.as<u32>(), c->d_exp_val.as<u32>(),
		listed ? c->d_exp_klist.as<u64>() : (const u64 *)nullptr, listed ? c->d_exp_valbase.as<u64>() : (const u64 *)nullptr);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipMemcpyAsync(offsets, c->d_exp_off.p, o * 4, hipMemcpyDeviceToHost, c->stream));
	if (nval) HIPCHK(c, hipMemcpyAsync(values, c->d_exp_val.p, nval * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

int mpcgpu_get_sparse(mpcgpu_ctx *c, uint64_t k, uint32_t *offsets, void *values)
{
	return mpcgpu_get_sparse_range(c, k, k + 1, offsets, values);
}


// mpcgpu_sw.inc — host side of sw_kernel (kernels_sw.h): mpcgpu_sw_set_scores, mpcgpu_sw_scores, mpcgpu_sw_info, mpcgpu_sw_bins. Included by mpcgpu.cpp
// inside its extern "C" block. Everything here lives in buffers of its own (mpcgpu_ctx::sw): shard, store and stage-A scratch of the
// context are neither read nor written, and the store epoch stays where it is.

extern "C++" {
namespace {

template <int H, bool LONG> void launch_sw_t(const SwParams &p, u32 grid, size_t smem, hipStream_t st)
{
	auto kern = sw_kernel<H, LONG>;
	MPC_LAUNCH(kern, grid, 256, smem, st, p);
}
// bin 1 .. MPC_SW_HMAX: rows per lane; bin MPC_SW_HMAX + 1: the row-block kernel
void launch_sw(u32 bin, const SwParams &p, u32 grid, size_t smem, hipStream_t st)
{
	switch (bin) {
	case 1: launch_sw_t<1, false>(p, grid, smem, st); break;
	case 2: launch_sw_t<2, false>(p, grid, smem, st); break;
	case 3: launch_sw_t<3, false>(p, grid, smem, st); break;
	case 4: launch_sw_t<4, false>(p, grid, smem, st); break;
	case 5: launch_sw_t<5, false>(p, grid, smem, st); break;
	case 6: launch_sw_t<6, false>(p, grid, smem, st); break;
	case 7: launch_sw_t<7, false>(p, grid, smem, st); break;
	case 8: launch_sw_t<8, false>(p, grid, smem, st); break;
	default: launch_sw_t<MPC_SW_HMAX, true>(p, grid, smem, st); break;
	}
}
static_assert(MPC_SW_HMAX == 8, "launch_sw lists the bins");

// the letters of the registered sequences as sw_kernel reads them, and the padded substitution table
int sw_upload_inputs(mpcgpu_ctx *c)
{
	mpcgpu_ctx::SwState &w = c->sw;
	const u32 alpha = w.alpha, W = alpha + 3;
	std::vector<u8> &let = w.v_let;
	std::vector<u32> &off = w.v_off;
	let.clear();
	off.assign(c->n, 0);
	for (u32 i = 0; i < c->n; ++i) {
		off[i] = (u32)let.size();
		for (u8 b : c->raw[i]) {
			const u8 l = w.letter[b];
			let.push_back(l < alpha ? l : (u8)alpha);
		}
		let.push_back((u8)(alpha + 1));
	}
	const float ninf = -__builtin_inff();
	std::vector<float> tab((size_t)(alpha + 2) * W, 0.0f);
	for (u32 a = 0; a < alpha + 2; ++a)
		for (u32 b = 0; b < W; ++b) {
			float v = 0.0f;
			if (a < alpha && b < alpha) v = w.sub[(size_t)a * alpha + b];
			if (a == alpha + 1 || b > alpha) v = ninf;
			tab[(size_t)a * W + b] = v;
		}
	if (upload(c, w.d_let, let) || upload(c, w.d_off, off) || upload(c, w.d_tab, tab)) return 1;
	return 0;
}

} // namespace
} // extern "C++"

int mpcgpu_sw_set_scores(mpcgpu_ctx *c, const uint8_t letter_of_char[256], uint32_t alpha, const float *sub, float open, float ext)
{
	if (!c) return 1;
	if (!letter_of_char || !sub) return fail(c, "mpcgpu_sw_set_scores: NULL argument");
	if (alpha == 0 || alpha > MPC_SW_ALPHA_MAX) return fail(c, "mpcgpu_sw_set_scores: alphabet size %u is outside 1 .. %d", alpha, MPC_SW_ALPHA_MAX);
	if (!(open <= 0.0f) || !(ext <= 0.0f)) return fail(c, "mpcgpu_sw_set_scores: gap scores must not be positive (open %g, ext %g; sw.cpp:151-152)", open, ext);
	for (u32 q = 0; q < alpha * alpha; ++q)
		if (!(sub[q] - sub[q] == 0.0f)) return fail(c, "mpcgpu_sw_set_scores: substitution score %u is not finite", q);
	mpcgpu_ctx::SwState &w = c->sw;
	memcpy(w.letter, letter_of_char, 256);
	w.alpha = alpha;
	w.sub.assign(sub, sub + (size_t)alpha * alpha);
	w.open = open;
	w.ext = ext;
	w.have = true;
	return 0;
}

extern "C++" {
namespace {

// mpcgpu_sw_scores; d_dst != NULL: the results also (scores == NULL: only) go to device memory at d_dst, pair q at d_dst[q] (mpcgpu_sw_tree)
int sw_scores_run(mpcgpu_ctx *c, uint64_t npairs, const uint32_t *seq1, const uint32_t *seq2, float *scores, float *d_dst)
{
	mpcgpu_ctx::SwState &w = c->sw;
	if (!w.have) return fail(c, "mpcgpu_sw_scores: call mpcgpu_sw_set_scores first");
	if (c->n == 0) return fail(c, "mpcgpu_sw_scores: call mpcgpu_set_seqs / mpcgpu_set_seqs_registry first");
	if ((seq1 == nullptr) != (seq2 == nullptr)) return fail(c, "mpcgpu_sw_scores: seq1 and seq2 must both be given or both be NULL");
	const bool all = seq1 == nullptr;
	if (all && npairs != (u64)c->n * (c->n - 1) / 2)
		return fail(c, "mpcgpu_sw_scores: all pairs of %u sequences are %llu pairs, not %llu", c->n, (unsigned long long)((u64)c->n * (c->n - 1) / 2), (unsigned long long)npairs);
	if (npairs && !scores && !d_dst) return fail(c, "mpcgpu_sw_scores: NULL argument");
	const u32 LMAX = 65535;
	if (all) {
		for (u32 i = 0; i < c->n; ++i)
			if (c->len[i] > LMAX) return fail(c, "mpcgpu_sw_scores: sequence %u has %u positions, more than %u", i, c->len[i], LMAX);
	} else {
		for (u64 q = 0; q < npairs; ++q) {
			if (seq1[q] >= c->n || seq2[q] >= c->n) return fail(c, "mpcgpu_sw_scores: sequence index out of range in pair %llu", (unsigned long long)q);
			for (u32 i : {seq1[q], seq2[q]})
				if (c->len[i] > LMAX) return fail(c, "mpcgpu_sw_scores: sequence %u has %u positions, more than %u", i, c->len[i], LMAX);
		}
	}
	u64 letters = c->n;
	for (u32 i = 0; i < c->n; ++i) letters += c->len[i];
	if (letters > 0xffffffffull) return fail(c, "mpcgpu_sw_scores: %llu letters in all, more than a 32-bit offset addresses", (unsigned long long)letters);
	w.pairs = w.cells = w.batches = w.items = w.long_items = 0;
	for (u32 b = 0; b < MPC_SW_HMAX + 2; ++b) w.bin_items[b] = w.bin_groups[b] = 0;
	w.ms = 0.0;
	if (npairs == 0) return 0;
	HIPCHK(c, hipSetDevice(c->device));
	if (sw_upload_inputs(c)) return 1;

	// Batches: a result word per pair and an item per chain, in device memory of this call's own. MPCGPU_SW_BATCH = pairs per batch
	// (2^24: 64 MB of results), MPCGPU_SW_CHAIN_COLS = columns after which a chain takes no further pair (a pair is never cut).
	const u64 batch_cap = (u64)std::max(1, env_int("MPCGPU_SW_BATCH", 1 << 24));
	const u32 chain_cols = (u32)std::max(1, env_int("MPCGPU_SW_CHAIN_COLS", 8192));
	const u32 NB = MPC_SW_HMAX + 2; // bins 1 .. HMAX + 1 (0 unused)
	const size_t smem = (size_t)(w.alpha + 2) * (w.alpha + 3) * sizeof(float);
	const u32 cus = (u32)std::max(1, c->prop.multiProcessorCount);
	std::vector<SwItem> bins[MPC_SW_HMAX + 2];
	u32 ai = 0, aj = 1; // all pairs: the next pair in InitPairs order (mpcflat.cpp:139-159)
	for (u64 q0 = 0; q0 < npairs;) {
		const u64 B = std::min(batch_cap, npairs - q0);
		for (u32 b = 0; b < NB; ++b) bins[b].clear();
		SwItem cur = {0, 0, 0, 0};
		u32 cur_bin = 0, prev_y = 0;
		u64 cells = 0;
		auto flush = [&]() { if (cur.ncols) bins[cur_bin].push_back(cur); cur.ncols = 0; };
		for (u64 q = 0; q < B; ++q) {
			u32 x, y;
			if (all) {
				x = ai; y = aj;
				if (++aj == c->n) { ++ai; aj = ai + 1; }
			} else { x = seq1[q0 + q]; y = seq2[q0 + q]; }
			const u32 ly1 = c->len[y] + 1;
			cells += (u64)c->len[x] * c->len[y];
			if (cur.ncols && cur.x == x && y == prev_y + 1 && cur.ncols + ly1 <= chain_cols)
				cur.ncols += ly1;
			else {
				flush();
				cur.x = x; cur.col0 = w.v_off[y]; cur.ncols = ly1; cur.out0 = (u32)q;
				cur_bin = c->len[x] <= MPC_SW_BLOCK_ROWS ? (c->len[x] + 63) / 64 : MPC_SW_HMAX + 1;
			}
			prev_y = y;
		}
		flush();
		std::vector<SwItem> &items = w.v_items;
		items.clear();
		u32 first[MPC_SW_HMAX + 3];
		for (u32 b = 0; b < NB; ++b) { first[b] = (u32)items.size(); items.insert(items.end(), bins[b].begin(), bins[b].end()); }
		first[NB] = (u32)items.size();
		u32 long_cols = 0;
		for (const SwItem &it : bins[MPC_SW_HMAX + 1]) long_cols = std::max(long_cols, it.ncols);
		const u64 bnd_stride = ((u64)long_cols + 63) & ~63ull;
		u32 long_grid = 0;
		if (long_cols) {
			// a workgroup's four lines of M and D: the grid is what 256 MB of them allow
			const u64 per_block = 4 * 2 * bnd_stride * sizeof(float);
			long_grid = (u32)std::max<u64>(1, std::min<u64>(std::min<u64>((bins[MPC_SW_HMAX + 1].size() + 3) / 4, cus * 2), ((u64)256 << 20) / per_block));
			HIPCHK(c, w.d_bnd.ensure(long_grid * per_block));
		}
		if (upload(c, w.d_items, items)) return 1;
		HIPCHK(c, w.d_scores.ensure(B * sizeof(u32)));
		HIPCHK(c, w.d_queue.ensure(NB * sizeof(u32)));
		HIPCHK(c, hipMemsetAsync(w.d_scores.p, 0, B * sizeof(u32), c->stream));
		HIPCHK(c, hipMemsetAsync(w.d_queue.p, 0, NB * sizeof(u32), c->stream));
		hipEvent_t ea = nullptr, eb = nullptr;
		HIPCHK(c, hipEventCreate(&ea));
		HIPCHK(c, hipEventCreate(&eb));
		HIPCHK(c, hipEventRecord(ea, c->stream));
		for (u32 b = 1; b < NB; ++b) {
			const u32 cnt = first[b + 1] - first[b];
			if (!cnt) continue;
			SwParams p;
			p.let = w.d_let.as<u8>(); p.seq_off = w.d_off.as<u32>(); p.seq_len = c->d_seq_len.as<u32>();
			p.items = w.d_items.as<SwItem>() + first[b]; p.count = cnt; p.queue = w.d_queue.as<u32>() + b;
			p.sub = w.d_tab.as<float>(); p.alpha = w.alpha; p.open = w.open; p.ext = w.ext;
			p.scores = w.d_scores.as<u32>();
			p.bnd = w.d_bnd.as<float>(); p.bnd_stride = bnd_stride;
			const u32 grid = (b == MPC_SW_HMAX + 1) ? long_grid : std::min<u32>((cnt + 3) / 4, cus * 8);
			launch_sw(b, p, grid, smem, c->stream);
			HIPCHK(c, hipGetLastError());
			w.bin_items[b] += cnt; w.bin_groups[b] += grid;
		}
		HIPCHK(c, hipEventRecord(eb, c->stream));
		if (d_dst) HIPCHK(c, hipMemcpyAsync(d_dst + q0, w.d_scores.p, B * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
		if (scores) HIPCHK(c, hipMemcpyAsync(scores + q0, w.d_scores.p, B * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		float ms = 0;
		HIPCHK(c, hipEventElapsedTime(&ms, ea, eb));
		(void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
		w.ms += ms;
		w.pairs += B; w.cells += cells; w.batches += 1; w.items += items.size(); w.long_items += bins[MPC_SW_HMAX + 1].size();
		if (trace_on()) {
			fprintf(stderr, "[mpcgpu] sw: batch of %llu pairs, %zu chains (%zu in row blocks), %.3f ms\n", (unsigned long long)B, items.size(), bins[MPC_SW_HMAX + 1].size(), ms);
			fflush(stderr);
		}
		q0 += B;
	}
	return 0;
}

} // namespace
} // extern "C++"

int mpcgpu_sw_scores(mpcgpu_ctx *c, uint64_t npairs, const uint32_t *seq1, const uint32_t *seq2, float *scores)
{
	if (!c) return 1;
	return sw_scores_run(c, npairs, seq1, seq2, scores, nullptr);
}

int mpcgpu_sw_info(mpcgpu_ctx *c, uint64_t out[6])
{
	if (!c) return 1;
	if (!out) return fail(c, "mpcgpu_sw_info: NULL argument");
	const mpcgpu_ctx::SwState &w = c->sw;
	out[0] = w.pairs; out[1] = w.cells; out[2] = w.batches; out[3] = w.items; out[4] = w.long_items;
	out[5] = (u64)(w.ms * 1e6); // nanoseconds
	return 0;
}

int mpcgpu_sw_bins(mpcgpu_ctx *c, uint64_t items[10], uint64_t groups[10])
{
	if (!c) return 1;
	if (!items || !groups) return fail(c, "mpcgpu_sw_bins: NULL argument");
	static_assert(MPC_SW_HMAX + 2 == 10, "mpcgpu_sw_bins reports bins 0 .. MPC_SW_HMAX + 1");
	const mpcgpu_ctx::SwState &w = c->sw;
	for (u32 b = 0; b < MPC_SW_HMAX + 2; ++b) { items[b] = w.bin_items[b]; groups[b] = w.bin_groups[b]; }
	return 0;
}

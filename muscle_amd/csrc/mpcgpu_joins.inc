// mpcgpu_joins.inc — alignment of alignments on the device store: CalcAlnFlat, BuildPost, AlignAlns, the PProg join and pair lists
// (part of mpcgpu.cpp's translation unit). Reference: alnalnsflat.cpp:7-52, buildpostflat.cpp:18-106, alnmsasflat.cpp:4-50, alignpairflat.cpp:3-27.

// ---- the dispatchers' limits, each in one place (tests/_joins.py and tests/_align_pairs.py restate them)
static const size_t MPC_LDS_MAX = 160u * 1024u; // dynamic LDS one workgroup may ask for
static const u64 MPC_ROWS_PAIRS_MAX = 2048; // row form of BuildPost: ordered pairs n1 * n2 of a join
static const u64 MPC_ROWS_CELLS1_MAX = 1u << 26; // row form, one join: n1 * C1 entries of the column -> position table
static const u64 MPC_ROWS_CELLS1_MAX_BATCH = 1u << 22; // the same in a list of joins (why it is smaller: not recorded)
// the one-wave alignment (calc_aln_wave_kernel and its batch form): LY + 1 columns in a wave's registers, LX + 1 rows of traceback codes in LDS
static size_t aln_wave_smem(u64 lds_rows) { return (size_t)(lds_rows * MPC_ALNW_ROWBYTES + 16); }
static bool aln_wave_fits(u32 LX, u32 LY) { return (u64)LY + 1 <= MPC_ALNW_MAXW && aln_wave_smem((u64)LX + 1) <= MPC_LDS_MAX; }
// raise a CalcAlnFlat kernel's dynamic-LDS limit only when this call needs more than any before; which: the kernel's entry of aln_smem_set
// (0 one wave, 1 several waves, 2 LDS rows, 3 one wave per alignment of a batch, 4 column tiles, 5 one wave per picked slot)
static void aln_smem_raise(mpcgpu_ctx *c, int which, const void *kernel, size_t smem)
{
	if (smem <= c->aln_smem_set[which]) return;
	(void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
	c->aln_smem_set[which] = smem;
}

// ---- the result record of an alignment {u32 path length, f32 score, path of at most LX + LY letters}: written by the kernel, read by the host
static u64 aln_rec_stride(u64 Lsum) { return (8 + Lsum + 7) & ~7ull; } // from one record to the next where several lie together
static AlnParams aln_params(const float *post, u32 LX, u32 LY, char *tb, char *rev, char *rec) { return {post, LX, LY, tb, rev, rec + 8, (u32 *)rec, (float *)(rec + 4)}; }
static int aln_rec_read(mpcgpu_ctx *c, const char *who, const char *rec, u32 LX, u32 LY, char *path, u32 *pathlen, float *score)
{
	u32 n_path;
	memcpy(&n_path, rec, 4);
	if (n_path > LX + LY) return fail(c, "%s: path length %u out of range (internal error)", who, n_path);
	*pathlen = n_path;
	if (score) memcpy(score, rec + 4, 4);
	memcpy(path, rec + 8, n_path);
	return 0;
}

// CalcAlnFlat + TraceBackFlat on a dense LX x LY matrix already in device memory
static int run_calc_aln(mpcgpu_ctx *c, const float *d_post, uint32_t LX, uint32_t LY, char *path, uint32_t *pathlen, float *score)
{
	const u64 W = (u64)LY + 1;
	// one wavefront with the previous row in registers and the traceback codes in LDS when the matrix is small enough
	// (the progressive joins and refinement rounds of L~400 families are), else the workgroup kernel
	const int pick = env_int("MPCGPU_ALN_KERNEL", 0); // 0 = by size, 1 = one wave, 2 = several waves, 3 = LDS rows, 4 = LDS rows in column tiles
	const bool wave = aln_wave_fits(LX, LY) && (pick == 0 || pick == 1);
	// several waves, 4 columns per thread, previous row in registers: up to 4096 columns
	const u32 qthreads = (u32)((W + 4 * 64 - 1) / (4 * 64)) * 64;
	const bool quad = !wave && qthreads <= 1024 && (pick == 0 || pick == 2);
	const u32 qrows = quad ? (u32)std::min<u64>((u64)LX + 1, (150u * 1024u) / qthreads) : 0;
	// two DP rows of LY + 1 floats in LDS; wider than that (or MPCGPU_ALN_KERNEL=4): the same rows in column tiles, the tile's left
	// edge carried through device memory (calc_aln_tiled_kernel). MPCGPU_ALN_TILE: columns per tile (tests: several tiles of a small matrix)
	const size_t smem_rows = (size_t)(2 * W + MPC_ALN_THREADS / 64 + 4) * 4;
	const bool tiled = !wave && !quad && (pick == 4 || smem_rows > MPC_LDS_MAX);
	const u32 tile = tiled ? (u32)std::min<u64>(W, (u64)std::min(std::max(env_int("MPCGPU_ALN_TILE", 16384), 1), 16384)) : 0;
	const size_t smem = wave ? aln_wave_smem((u64)LX + 1) : quad ? (size_t)MPC_ALNQ_HDR + (size_t)qrows * qthreads : tiled ? (size_t)(2 * ((u64)tile + 1) + MPC_ALN_THREADS / 64 + 4) * 4 : smem_rows;
	if (tiled) HIPCHK(c, c->d_aln_bnd.ensure_grow(2 * ((u64)LX + 1) * 4));
	HIPCHK(c, c->d_aln_tb.ensure_grow(((u64)LX + 1) * (quad ? (u64)qthreads : W))); // letters per cell, or one byte per thread and row
	HIPCHK(c, c->d_aln_rev.ensure_grow((u64)LX + LY));
	HIPCHK(c, c->h_aln_res.ensure(8 + (u64)LX + LY)); // one result record, unpadded
	// the record is written straight into page-locked host memory (device-visible: hipHostMalloc): no copy back, one wait
	const AlnParams ap = aln_params(d_post, LX, LY, c->d_aln_tb.as<char>(), c->d_aln_rev.as<char>(), c->h_aln_res.as<char>());
	aln_smem_raise(c, wave ? 0 : quad ? 1 : tiled ? 4 : 2,
		wave ? (const void *)calc_aln_wave_kernel : quad ? (const void *)calc_aln_quad_kernel : tiled ? (const void *)calc_aln_tiled_kernel : (const void *)calc_aln_kernel, smem);
	if (trace_on()) { fprintf(stderr, "[mpcgpu] calc_aln %u x %u: %s\n", LX, LY, wave ? "one wave" : quad ? "waves, rows in registers" : tiled ? "rows in LDS, column tiles" : "rows in LDS"); fflush(stderr); }
	TimedSpan ts_aln;
	if (span_begin(c, 8, &ts_aln)) return 1;
	if (wave) MPC_LAUNCH(calc_aln_wave_kernel, 1, 64, smem, c->stream, ap);
	else if (quad) MPC_LAUNCH(calc_aln_quad_kernel, 1, qthreads, smem, c->stream, ap, qrows);
	else if (tiled) MPC_LAUNCH(calc_aln_tiled_kernel, 1, MPC_ALN_THREADS, smem, c->stream, ap, c->d_aln_bnd.as<float>(), tile);
	else MPC_LAUNCH(calc_aln_kernel, 1, MPC_ALN_THREADS, smem, c->stream, ap);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts_aln)) return 1;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return aln_rec_read(c, "mpcgpu_calc_aln", c->h_aln_res.as<char>(), LX, LY, path, pathlen, score);
}

// The finishing kernels (kernels_post.h) on ONE caller-supplied list of cells with Score >= MIN_SPARSE_SCORE — what fb_kernel
// would have emitted for a pair. Lets tests reach shapes of the candidate list the pair-HMM never produces (rows whose first
// cell lies beyond the EA frontier, empty rows, one-column matrices) and compare both kernels with the dense
// CalcAlnScoreFlat (calcalnscoreflat.cpp:4-32) / MySparseMx::FromPost (mysparsemx.cpp:115-152).
int mpcgpu_post_scores(mpcgpu_ctx *c, uint32_t LX, uint32_t LY, uint32_t ncand, const uint32_t *rows, const uint32_t *cols,
	const float *scores, int kernel, uint32_t batch, float *ea, uint32_t *nnz, uint32_t *offsets, void *values)
{
	if (!c) return 1;
	if (!c->have_hmm) return fail(c, "mpcgpu_post_scores: set_hmm first (expf variant)");
	if (LX == 0 || LY == 0 || LX > MPC_KEY_COL_MASK_LONG || LY > MPC_KEY_COL_MASK_LONG) return fail(c, "mpcgpu_post_scores: bad shape %u x %u", LX, LY);
	if (kernel < 0 || kernel > 2) return fail(c, "mpcgpu_post_scores: kernel %d (0 = post_rows_kernel, 1 = post_kernel, 2 = post_wide_kernel)", kernel);
	HIPCHK(c, hipSetDevice(c->device));
	++c->epoch;
	const u32 capc = std::max<u32>(ncand, 1);
	std::vector<u64> cand(capc, 0);
	const u32 long_min = LX > 1023u ? LX : 0xffffffffu; // 22-bit column keys unless the rows need more than 10 bits
	const u32 kshift = LX >= long_min ? MPC_KEY_ROW_SHIFT_LONG : MPC_KEY_ROW_SHIFT;
	for (u32 q = 0; q < ncand; ++q) {
		if (rows[q] >= LX || cols[q] >= LY) return fail(c, "mpcgpu_post_scores: cell %u out of range", q);
		u32 bits;
		memcpy(&bits, &scores[q], 4);
		cand[q] = ((u64)((rows[q] << kshift) | cols[q]) << 32) | bits;
	}
	const std::vector<u32> lens = {LX, LY}, zero = {0}, one = {1}, cnt = {ncand};
	DevBuf d_len, d_x, d_y, d_cnt, d_cand, d_res, d_out, d_sort, d_srow;
	auto free_all = [&]() { for (DevBuf *b : {&d_len, &d_x, &d_y, &d_cnt, &d_cand, &d_res, &d_out, &d_sort, &d_srow}) b->release(); };
	StageAGeom g; g.LXmax = LX; g.LYmax = LY; g.long_min = long_min; g.capc = capc; // of the one pair
	const u64 res_stride = g.res_stride();
	int rc = 0;
	do {
		if (upload(c, d_len, lens) || upload(c, d_x, zero) || upload(c, d_y, one) || upload(c, d_cnt, cnt) || upload(c, d_cand, cand)) { rc = 1; break; }
		if (d_res.ensure(res_stride * 4) != hipSuccess || d_out.ensure(16) != hipSuccess) { rc = fail(c, "mpcgpu_post_scores: out of device memory"); break; }
		const PostIO io = {d_x.as<u32>(), d_y.as<u32>(), d_len.as<u32>(), d_cand.as<u64>(), d_cnt.as<u32>(), d_res.as<u32>(), d_out.as<u32>(), d_out.as<float>() + 1, d_out.as<u32>() + 2, 1};
		if (kernel == 0) {
			if (!post_rows_fits(LX, LY, 1)) { rc = fail(c, "mpcgpu_post_scores: %u x %u does not fit the row-list kernel", LX, LY); break; }
			if (d_sort.ensure((u64)capc * 8 + 8) != hipSuccess) { rc = fail(c, "mpcgpu_post_scores: out of device memory"); break; }
			if (launch_post_rows(c, g, io, 1024, batch, 1, d_sort, false)) { rc = 1; break; }
		} else if (kernel == 2) {
			if (launch_post_wide(c, g, io, 1, false)) { rc = 1; break; }
		} else {
			PostParams pp;
			const size_t psmem = fill_post(c, g, io, 1024, pp);
			if (d_sort.ensure(pp.sort_stride * 8) != hipSuccess || d_srow.ensure(pp.srow_stride * 4) != hipSuccess) { rc = fail(c, "mpcgpu_post_scores: out of device memory"); break; }
			pp.sort_scratch = d_sort.as<u64>(); pp.srow_scratch = d_srow.as<float>();
			post_info_set(c, 1, 64, 1, 1);
			MPC_LAUNCH(post_kernel, 1, 64, psmem, c->stream, pp);
		}
		if (hipGetLastError() != hipSuccess) { rc = fail(c, "mpcgpu_post_scores: launch failed"); break; }
		u32 out[4] = {0, 0, 0, 0};
		if (hipMemcpyAsync(out, d_out.p, 12, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(c, "mpcgpu_post_scores: copy failed"); break; }
		if (out[2] & 1u) { rc = fail(c, "mpcgpu_post_scores: candidate overflow"); break; }
		if (nnz) *nnz = out[0];
		if (ea) memcpy(ea, &out[1], 4);
		if (offsets && values) { // MySparseMx layout: offsets[LX+1], {P, col} per entry
			std::vector<u32> rec(res_stride);
			if (hipMemcpyAsync(rec.data(), d_res.p, res_stride * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(c, "mpcgpu_post_scores: copy failed"); break; }
			u32 acc = 0;
			for (u32 i = 0; i < LX; ++i) { offsets[i] = acc; acc += rec[i]; }
			offsets[LX] = acc;
			memcpy(values, rec.data() + LX + LY, (size_t)out[0] * 8);
		}
	} while (0);
	free_all();
	return rc;
}

int mpcgpu_calc_aln(mpcgpu_ctx *c, const float *post, uint32_t LX, uint32_t LY, char *path, uint32_t *pathlen, float *score)
{
	if (!c) return 1;
	if (!post || !path || !pathlen) return fail(c, "mpcgpu_calc_aln: NULL argument");
	if (LX == 0 || LY == 0) return fail(c, "mpcgpu_calc_aln: empty matrix (%u x %u)", LX, LY);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, c->d_aln_post.ensure((u64)LX * LY * 4));
	HIPCHK(c, hipMemcpyAsync(c->d_aln_post.p, post, (u64)LX * LY * 4, hipMemcpyHostToDevice, c->stream));
	c->last_post_cells = (u64)LX * LY;
	return run_calc_aln(c, c->d_aln_post.as<float>(), LX, LY, path, pathlen, score); // syncs: the caller's buffer is done with
}

static u32 bits_for(u64 v) { u32 b = 1; while ((v >> b) != 0) ++b; return b; } // bits to hold values 0..v

int mpcgpu_align_alns(mpcgpu_ctx *c, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2, uint32_t C1,
	uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, char *path, uint32_t *pathlen, float *score)
{
	return mpcgpu_align_alns_w(c, n1, seq1, n2, seq2, C1, C2, pos2col1, pos2col2, nullptr, nullptr, path, pathlen, score);
}

// Buffers of the in-order reduction (kernels_prog.h): end of every cell's run, the list of runs, {runs, next run}. The
// generating kernel zeroes the output matrix and the two counters.
struct RunBufs { u32 *run_end, *heads, *counters; };
static int prepare_runs(mpcgpu_ctx *c, u64 M, u64 cells, RunBufs *rb)
{
	if (cells > 0xffffffffull) return fail(c, "mpcgpu_align_alns: %llu cells exceed this build's cell index", (u64)cells);
	const u64 maxruns = std::min<u64>(M, cells);
	HIPCHK(c, c->d_bp_runs.ensure_grow((cells + 2 * maxruns + 2) * 4));
	rb->run_end = c->d_bp_runs.as<u32>(); rb->heads = rb->run_end + cells; rb->counters = rb->heads + 2 * maxruns;
	return 0;
}
// post[cell] = the cell's records added in key order, 0 where there are none: list the runs of the sorted records, one wave per run.
static int reduce_runs(mpcgpu_ctx *c, const RunBufs &rb, const u32 *keys_sorted, const float *vals_sorted, u64 M, u64 cells)
{
	if (!M) return 0;
	const u64 maxruns = std::min<u64>(M, cells);
	const u32 grid_cap = (u32)c->prop.multiProcessorCount * 8;
	MPC_LAUNCH(build_post_heads_kernel, (u32)std::min<u64>((M + 255) / 256, grid_cap), 256, 0, c->stream, keys_sorted, (u64)M, rb.run_end, rb.heads,
		rb.counters);
	HIPCHK(c, hipGetLastError());
	// two waves per SIMD pulling runs from a queue (kernels_prog.h); MPCGPU_BP_WAVES: resident waves per SIMD
	const int bp_waves = 2; // (one: 0.238 s, two: 0.255, four: 0.298 of reduce launches in -align 1000 x 400, profiles/r11t; two is level on -super7)
	const u32 red_grid = (u32)c->prop.multiProcessorCount * (u32)bp_waves;
	MPC_LAUNCH(build_post_reduce_kernel, (u32)std::min<u64>((maxruns + 3) / 4, red_grid), 256, 0, c->stream, vals_sorted, (const u32 *)rb.run_end,
		(const u32 *)rb.heads, (const u32 *)rb.counters, rb.counters + 1, c->d_aln_post.as<float>());
	HIPCHK(c, hipGetLastError());
	return 0;
}

// The tail of the general path. The generating kernel left M {cell, value} records in the first halves of d_bp_keys / d_bp_vals: sort them by cell into
// the second halves (fewer than two: nothing to sort), add every cell's run in order. timed: under the spans of families 6 and 7 (build_post_impl's).
static int sort_reduce(mpcgpu_ctx *c, const RunBufs &rb, u64 M, u64 cells, bool timed)
{
	u32 *keys_in = c->d_bp_keys.as<u32>(), *keys_out = keys_in + std::max<u64>(M, 1);
	float *vals_in = c->d_bp_vals.as<float>(), *vals_out = vals_in + std::max<u64>(M, 1);
	TimedSpan ts;
	if (timed && span_begin(c, 6, &ts)) return 1;
	if (M > 1)
		HIPCHK(c, mpc_sort_pairs([&](size_t bytes) -> void * { return c->d_bp_tmp.ensure_grow(bytes) == hipSuccess ? c->d_bp_tmp.p : nullptr; },
			keys_in, keys_out, vals_in, vals_out, (size_t)M, bits_for(cells - 1), c->stream));
	if (timed && (span_end(c, &ts) || span_begin(c, 7, &ts))) return 1;
	if (reduce_runs(c, rb, M > 1 ? keys_out : keys_in, M > 1 ? vals_out : vals_in, M, cells)) return 1;
	return timed ? span_end(c, &ts) : 0;
}

// One join as its entry point received it: MSA1's and MSA2's rows (sequence indices), their position -> column maps one after the other,
// weights (NULL: none, or all 1.0f). len1, len2: residues of each side, the length of its maps.
struct JoinIn { u32 n1, n2, C1, C2; const u32 *seq1, *seq2, *map1, *map2; const float *w1, *w2; u64 len1, len2; };
// the row form of BuildPost (build_post_rows_kernel) takes it: needs the variable-size record store (every ordered pair by row)
static bool rows_form_fits(const mpcgpu_ctx *c, const JoinIn &j, u64 pairs_max, bool batch)
{
	return c->have_pad && (u64)j.n1 * j.n2 <= pairs_max && j.C2 <= 1024u && (u64)j.n1 * j.C1 <= (batch ? MPC_ROWS_CELLS1_MAX_BATCH : MPC_ROWS_CELLS1_MAX);
}
// two arrays of 4-byte items, one after the other
static void put_pair(void *dst, const void *a, size_t na, const void *b, size_t nb) { memcpy(dst, a, 4 * na); memcpy((char *)dst + 4 * na, b, 4 * nb); }

// A row's position -> column map lies inside its alignment's C columns and rises strictly (Sequence::GetPosToCol of an aligned row): two
// positions on one column would add twice into one cell of the matrix. unit: what `row` counts in the message ("row", or "in pair" for
// mpcgpu_align_msas); sfx: " (join j)" in a list of joins, else empty.
static int check_row_map(mpcgpu_ctx *c, const char *who, u32 side, const char *unit, u32 row, const u32 *map, u32 L, u32 C, const char *sfx)
{
	for (u32 pos = 0; pos < L; ++pos) {
		if (map[pos] >= C) return fail(c, "%s: column map of MSA%u out of range%s", who, side, sfx);
		if (pos && map[pos] <= map[pos - 1]) return fail(c, "%s: column map of MSA%u %s %u is not strictly increasing at position %u%s", who, side, unit, row, pos, sfx);
	}
	return 0;
}

// ---- the row form of BuildPost (kernels_prog.h: build_post_rows_kernel): a join's inputs are one slice of a page-locked host record,
// [seqs: n1+n2 u32][c2p: n1*C1 u32, MSA1's maps inverted][off2: n2+1 u32][maps2: len2 u32][weights: n1+n2 f32, when given]
static u64 rows_slice_bytes(const JoinIn &j) { return 4 * ((u64)j.n1 + j.n2 + (u64)j.n1 * j.C1 + j.n2 + 1 + j.len2 + (j.w1 ? (u64)j.n1 + j.n2 : 0)); }
// Validates the join (MSA1's maps, MSA2's maps, no sequence on both sides: before anything of it is launched) and writes its slice at `at` of hin.
// rp's pointers are formed from base: hin where the kernel reads the page-locked record, or its device copy; rp.post and rp.err are the caller's.
// join: the index in a list of joins, for the messages; -1: a single join.
static int stage_rows(mpcgpu_ctx *c, const char *who, int64_t join, const JoinIn &j, char *hin, const char *base, u64 at, BuildPostRowsParams &rp)
{
	char sfx[24] = "";
	if (join >= 0) snprintf(sfx, sizeof sfx, " (join %u)", (u32)join);
	const u64 o_seqs = at, o_c2p = o_seqs + 4 * ((u64)j.n1 + j.n2), o_off2 = o_c2p + 4 * (u64)j.n1 * j.C1, o_maps2 = o_off2 + 4 * ((u64)j.n2 + 1), o_w = o_maps2 + 4 * j.len2;
	u32 *seqs = (u32 *)(hin + o_seqs), *c2p = (u32 *)(hin + o_c2p), *off2 = (u32 *)(hin + o_off2), *maps2 = (u32 *)(hin + o_maps2);
	put_pair(seqs, j.seq1, j.n1, j.seq2, j.n2);
	for (u64 q = 0; q < (u64)j.n1 * j.C1; ++q) c2p[q] = MPC_BPR_GAP;
	u64 m = 0;
	for (u32 a = 0; a < j.n1; ++a) {
		const u32 L = c->len[j.seq1[a]];
		if (check_row_map(c, who, 1, "row", a, j.map1 + m, L, j.C1, sfx)) return 1;
		for (u32 pos = 0; pos < L; ++pos) c2p[(u64)a * j.C1 + j.map1[m + pos]] = pos;
		m += L;
	}
	off2[0] = 0;
	for (u32 b = 0; b < j.n2; ++b) off2[b + 1] = off2[b] + c->len[j.seq2[b]];
	memcpy(maps2, j.map2, 4 * (size_t)j.len2);
	for (u32 b = 0; b < j.n2; ++b)
		if (check_row_map(c, who, 2, "row", b, maps2 + off2[b], off2[b + 1] - off2[b], j.C2, sfx)) return 1;
	for (u32 a = 0; a < j.n1; ++a)
		for (u32 b = 0; b < j.n2; ++b) if (j.seq1[a] == j.seq2[b])
			return join < 0 ? fail(c, "mpcgpu_align_alns: sequence %u is in both alignments", j.seq1[a]) : fail(c, "%s: sequence %u is in both alignments of join %u", who, j.seq1[a], (u32)join);
	if (j.w1) put_pair(hin + o_w, j.w1, j.n1, j.w2, j.n2);
	fill_store_params(c, rp.s);
	rp.seq1 = (const u32 *)(base + o_seqs); rp.seq2 = rp.seq1 + j.n1; rp.n1 = j.n1; rp.n2 = j.n2; rp.C1 = j.C1; rp.C2 = j.C2;
	rp.c2p1 = (const u32 *)(base + o_c2p); rp.p2c2 = (const u32 *)(base + o_maps2); rp.off2 = (const u32 *)(base + o_off2);
	rp.w1 = j.w1 ? (const float *)(base + o_w) : nullptr; rp.w2 = j.w1 ? rp.w1 + j.n1 : nullptr;
	return 0;
}

// MPCGPU_TRACE & 4: host wall time of a join's phases (vectors, uploads, launches, calc_aln + syncs), summed per context: the shrub
// workers of -super7 call build_post_impl concurrently on their own contexts
struct LapTimer {
	mpcgpu_ctx *c; bool on = false; double t_prev = 0.0;
	static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
	void start() { static const bool host_trace = trace_host(); on = host_trace; t_prev = on ? now() : 0.0; }
	void lap(int k) { if (on) { const double t = now(); c->aa_trace_t[k] += t - t_prev; t_prev = t; } }
};

// build_post_impl's argument and length checks; starts the lap timer once the device is set, fills in len1 and len2 and drops weights
// that are all 1.0f (what MPCFlat::Run sets): (1*1)*P == P, skip the multiply
static int build_post_check(mpcgpu_ctx *c, JoinIn &j, const char *path, const uint32_t *pathlen, LapTimer &lt)
{
	if (!c->have_store) return fail(c, "mpcgpu_align_alns: no store (call mpcgpu_build_store / mpcgpu_store_import)");
	// BuildPost reads the records of any sequence: a partial store (a rank of a block-partitioned run) is completed first — once,
	// from the packed records, which hold the current values
	if ((c->partial || c->packed_stale) && mpcgpu_store_complete(c)) return 1;
	if (!j.seq1 || !j.seq2 || !j.map1 || !j.map2 || (path && !pathlen)) return fail(c, "mpcgpu_align_alns: NULL argument");
	if (j.n1 == 0 || j.n2 == 0 || j.C1 == 0 || j.C2 == 0) return fail(c, "mpcgpu_align_alns: empty alignment");
	HIPCHK(c, hipSetDevice(c->device));
	lt.start();
	j.len1 = j.len2 = 0;
	for (u32 a = 0; a < j.n1 + j.n2; ++a) {
		const u32 S = a < j.n1 ? j.seq1[a] : j.seq2[a - j.n1];
		if (S >= c->n) return fail(c, "mpcgpu_align_alns: sequence index %u out of range", S);
		(a < j.n1 ? j.len1 : j.len2) += c->len[S];
	}
	if ((j.w1 != nullptr) != (j.w2 != nullptr)) return fail(c, "mpcgpu_align_alns_w: give both weight arrays or neither");
	bool weighted = false;
	for (u32 a = 0; j.w1 && a < j.n1 + j.n2; ++a) weighted = weighted || (a < j.n1 ? j.w1[a] : j.w2[a - j.n1]) != 1.0f;
	if (!weighted) j.w1 = j.w2 = nullptr;
	return 0;
}

// Small joins: the whole matrix in one launch, inputs read from page-locked host memory, and the alignment when path != NULL.
// MPCGPU_BP: "sort": always the general path; "rows": this one whenever its limits but the pair count allow.
// 0 = done, 1 = error, 2 = not applicable, or a chunk of pairs overflowed the row kernel's list (very wide posterior rows): the
// general path does the join
static int build_post_rows(mpcgpu_ctx *c, const char *who, const JoinIn &j, LapTimer &lt, char *path, uint32_t *pathlen, float *score)
{
	const char *bp_mode = getenv("MPCGPU_BP");
	if (bp_mode && !strcmp(bp_mode, "sort")) return 2;
	const u64 pairs_max = (bp_mode && !strcmp(bp_mode, "rows")) ? ~0ull : MPC_ROWS_PAIRS_MAX;
	if (!rows_form_fits(c, j, pairs_max, false)) return 2;
	const u64 o_err = rows_slice_bytes(j); // the record: the join's slice, then the kernel's overflow flag
	HIPCHK(c, c->h_bp_in.ensure(o_err + 4));
	char *hin = c->h_bp_in.as<char>();
	BuildPostRowsParams rp;
	if (stage_rows(c, who, -1, j, hin, hin, 0, rp)) return 1;
	*(u32 *)(hin + o_err) = 0u;
	lt.lap(0);
	const u64 cells = (u64)j.C1 * j.C2;
	HIPCHK(c, c->d_aln_post.ensure_grow(cells * 4));
	rp.post = c->d_aln_post.as<float>(); rp.err = (u32 *)(hin + o_err);
	const u32 grid = std::min<u32>(j.C1, (u32)c->prop.multiProcessorCount * 8u);
	if (trace_on()) { fprintf(stderr, "[mpcgpu] build_post %u x %u rows, %u x %u columns: row kernel, grid %u\n", j.n1, j.n2, j.C1, j.C2, grid); fflush(stderr); }
	TimedSpan ts_rows;
	if (span_begin(c, 5, &ts_rows)) return 1;
	if (c->pad_long) { // the record store's long form: the same body with the long blocks' decode
		if (j.C2 <= 512u) MPC_LAUNCH(build_post_rows_long_kernel<8>, grid, 64, 8 * MPC_BPR_CAP, c->stream, rp);
		else MPC_LAUNCH(build_post_rows_long_kernel<16>, grid, 64, 8 * MPC_BPR_CAP, c->stream, rp);
	}
	else if (j.C2 <= 512u) MPC_LAUNCH(build_post_rows_kernel<8>, grid, 64, 8 * MPC_BPR_CAP, c->stream, rp);
	else MPC_LAUNCH(build_post_rows_kernel<16>, grid, 64, 8 * MPC_BPR_CAP, c->stream, rp);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts_rows)) return 1;
	lt.lap(2);
	c->last_post_cells = cells;
	int rc_rows = 0;
	if (!path) HIPCHK(c, hipStreamSynchronize(c->stream));
	else rc_rows = run_calc_aln(c, c->d_aln_post.as<float>(), j.C1, j.C2, path, pathlen, score); // ends with a wait for the stream
	lt.lap(3);
	return *(volatile u32 *)(hin + o_err) == 0u ? rc_rows : 2;
}

// The general path of BuildPost: a record per contribution, sorted by cell, every cell's run added in order. Everything the kernels
// need from this call in ONE page-locked record, one copy:
// [off: n1+n2+1 u64][coff: n1*n2+1 u64][seqs: n1+n2 u32][maps: len1+len2 u32][weights: n1+n2 f32, when given]
static int build_post_general(mpcgpu_ctx *c, const char *who, const JoinIn &j, LapTimer &lt)
{
	const u32 n1 = j.n1, n2 = j.n2;
	const u64 npairs12 = (u64)n1 * n2;
	const u64 o_off = 0, o_coff = o_off + 8 * ((u64)n1 + n2 + 1), o_seqs = o_coff + 8 * (npairs12 + 1), o_maps = o_seqs + 4 * ((u64)n1 + n2),
		o_w = o_maps + 4 * (j.len1 + j.len2), in_bytes = o_w + (j.w1 ? 4 * ((u64)n1 + n2) : 0);
	HIPCHK(c, c->h_bp_in.ensure(in_bytes));
	char *hin = c->h_bp_in.as<char>();
	u64 *off = (u64 *)(hin + o_off), *coff = (u64 *)(hin + o_coff);
	u32 *seqs = (u32 *)(hin + o_seqs), *maps = (u32 *)(hin + o_maps);
	put_pair(seqs, j.seq1, n1, j.seq2, n2);
	off[0] = 0;
	for (u32 a = 0; a < n1 + n2; ++a) off[a + 1] = off[a] + c->len[seqs[a]];
	put_pair(maps, j.map1, j.len1, j.map2, j.len2);
	for (u32 a = 0; a < n1; ++a) if (check_row_map(c, who, 1, "row", a, maps + off[a], (u32)(off[a + 1] - off[a]), j.C1, "")) return 1;
	for (u32 b = n1; b < n1 + n2; ++b) if (check_row_map(c, who, 2, "row", b - n1, maps + off[b], (u32)(off[b + 1] - off[b]), j.C2, "")) return 1;
	coff[0] = 0;
	for (u32 a = 0; a < n1; ++a)
		for (u32 b = 0; b < n2; ++b) {
			const u32 S = seqs[a], T = seqs[n1 + b];
			if (S == T) return fail(c, "mpcgpu_align_alns: sequence %u is in both alignments", S);
			const u64 k = S < T ? pair_pos(c, S, T) : pair_pos(c, T, S); // (position in the context's pair order: all_nnz is kept in it)
			coff[(u64)a * n2 + b + 1] = coff[(u64)a * n2 + b] + c->all_nnz[k];
		}
	if (j.w1) put_pair(hin + o_w, j.w1, n1, j.w2, n2);
	const u64 M = coff[npairs12];
	const u64 cells = (u64)j.C1 * j.C2;
	if (cells > 0xffffffffull) return fail(c, "mpcgpu_align_alns: %llu cells exceed this build's cell index", (u64)cells);
	if (M > 0xffffffffull) return fail(c, "mpcgpu_align_alns: %llu contributions exceed this build's record count", (u64)M);
	lt.lap(0);
	HIPCHK(c, c->d_bp_in.ensure_grow(in_bytes));
	HIPCHK(c, hipMemcpyAsync(c->d_bp_in.p, hin, in_bytes, hipMemcpyHostToDevice, c->stream));
	lt.lap(1);
	HIPCHK(c, c->d_bp_keys.ensure_grow(std::max<u64>(M, 1) * 4 * 2));
	HIPCHK(c, c->d_bp_vals.ensure_grow(std::max<u64>(M, 1) * 4 * 2));
	HIPCHK(c, c->d_aln_post.ensure_grow(cells * 4));
	RunBufs rb;
	if (prepare_runs(c, M, cells, &rb)) return 1;
	const char *din = c->d_bp_in.as<char>();
	BuildPostParams bp;
	fill_store_params(c, bp.s);
	bp.seq1 = (const u32 *)(din + o_seqs); bp.seq2 = bp.seq1 + n1; bp.n1 = n1; bp.n2 = n2;
	bp.p2c1 = (const u32 *)(din + o_maps); bp.p2c2 = bp.p2c1; // offsets below are into the one concatenated array
	bp.p2c1_off = (const u64 *)(din + o_off); bp.p2c2_off = bp.p2c1_off + n1;
	bp.C2 = j.C2; bp.coff = (const u64 *)(din + o_coff); bp.keys = c->d_bp_keys.as<u32>(); bp.vals = c->d_bp_vals.as<float>();
	bp.w1 = j.w1 ? (const float *)(din + o_w) : nullptr; bp.w2 = j.w1 ? bp.w1 + n1 : nullptr;
	bp.post = c->d_aln_post.as<float>(); bp.cells = cells; bp.counters = rb.counters;
	TimedSpan ts_bp;
	if (span_begin(c, 5, &ts_bp)) return 1;
	MPC_LAUNCH(build_post_gen_kernel, (u32)std::min<u64>(npairs12, (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, bp);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts_bp)) return 1;
	if (sort_reduce(c, rb, M, cells, true)) return 1;
	lt.lap(2);
	c->last_post_cells = cells;
	return 0;
}

// BuildPost on the device store (+ CalcAlnFlat when path != NULL): the body of mpcgpu_align_alns_w and mpcgpu_build_post, and of
// mpcgpu_align_alns_batch for the joins it runs one at a time (who: the entry point, for the messages about the caller's maps)
static int build_post_impl(mpcgpu_ctx *c, const char *who, JoinIn j, char *path, uint32_t *pathlen, float *score)
{
	if (!c) return 1;
	LapTimer lt{c};
	if (build_post_check(c, j, path, pathlen, lt)) return 1;
	const int rc_rows = build_post_rows(c, who, j, lt, path, pathlen, score);
	if (rc_rows != 2) return rc_rows;
	if (build_post_general(c, who, j, lt)) return 1;
	// the staging record is reused by the next call: drain the stream (run_calc_aln ends with a wait for it)
	if (!path) { // matrix only (mpcgpu_build_post)
		HIPCHK(c, hipStreamSynchronize(c->stream));
		return 0;
	}
	const int rc_aln = run_calc_aln(c, c->d_aln_post.as<float>(), j.C1, j.C2, path, pathlen, score);
	lt.lap(3);
	if (lt.on && (++c->aa_trace_n % 100) == 0)
		fprintf(stderr, "[mpcgpu] align_alns host seconds after %llu calls: vectors %.3f, uploads %.3f, launches %.3f, calc_aln+syncs %.3f\n",
			(unsigned long long)c->aa_trace_n, c->aa_trace_t[0], c->aa_trace_t[1], c->aa_trace_t[2], c->aa_trace_t[3]);
	return rc_aln;
}

int mpcgpu_align_alns_w(mpcgpu_ctx *c, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2, uint32_t C1,
	uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, const float *w1, const float *w2, char *path,
	uint32_t *pathlen, float *score)
{
	if (!c) return 1;
	if (!path || !pathlen) return fail(c, "mpcgpu_align_alns: NULL argument");
	const JoinIn j = {n1, n2, C1, C2, seq1, seq2, pos2col1, pos2col2, w1, w2, 0, 0};
	return build_post_impl(c, "mpcgpu_align_alns", j, path, pathlen, score);
}

// calc_aln_wave_batch_kernel, a workgroup of one wave per AlnParams record; lds_rows: the longest LX + 1 among them
static int launch_aln_wave_batch(mpcgpu_ctx *c, const AlnParams *ap, u32 n, u32 lds_rows)
{
	const size_t smem = aln_wave_smem(lds_rows);
	aln_smem_raise(c, 3, (const void *)calc_aln_wave_batch_kernel, smem);
	TimedSpan ts;
	if (span_begin(c, 8, &ts)) return 1;
	MPC_LAUNCH(calc_aln_wave_batch_kernel, n, 64, smem, c->stream, ap);
	HIPCHK(c, hipGetLastError());
	return span_end(c, &ts);
}

// A LIST of independent joins (the joins of one level of MPCFlat::ProgressiveAlign's guide tree, progalnflat.cpp:72-100: a join needs its
// two children, joins of different subtrees nothing of each other). The small ones — the row form of BuildPost and the one-wave
// alignment: what nearly all joins of a tree are — run TOGETHER: one launch builds every matrix (a workgroup per output row of a join),
// one launch aligns them (a workgroup per join), one copy in, one wait. 999 joins of a 1000-sequence tree one after the other are 999 x
// (two one-wave kernels + a round trip): 0.24 s of device time of which almost nothing is arithmetic. A join that does not fit the small
// forms (the few near the root) is aligned by build_post_impl, in list order. Same matrices, same paths: the per-join work is the
// single-join kernels' body.
// The plan: every join of the list as a JoinIn (its rows and maps follow the previous join's in seqs and pos2col), and which joins take
// the batched forms (small). Small implies C2 <= 511 (the one-wave alignment's LY + 1 <= MPC_ALNW_MAXW), so the row kernel's 8 columns
// per lane always do: there is no <16> batch launch.
static int plan_joins(mpcgpu_ctx *c, u32 njoins, const u32 *n1, const u32 *n2, const u32 *C1, const u32 *C2, const u32 *seqs, const u32 *pos2col,
	u32 path_stride, std::vector<JoinIn> &jn, std::vector<u32> &small)
{
	for (u32 j = 0; j < njoins; ++j) {
		JoinIn J = {n1[j], n2[j], C1[j], C2[j], seqs, seqs + n1[j], pos2col, nullptr, nullptr, nullptr, 0, 0};
		if (J.n1 == 0 || J.n2 == 0 || J.C1 == 0 || J.C2 == 0) return fail(c, "mpcgpu_align_alns_batch: join %u is empty", j);
		if ((u64)J.C1 + J.C2 > path_stride) return fail(c, "mpcgpu_align_alns_batch: path_stride %u too small for join %u", path_stride, j);
		for (u32 a = 0; a < J.n1 + J.n2; ++a) {
			if (seqs[a] >= c->n) return fail(c, "mpcgpu_align_alns_batch: sequence index %u out of range", seqs[a]);
			(a < J.n1 ? J.len1 : J.len2) += c->len[seqs[a]];
		}
		J.map2 = J.map1 + J.len1;
		seqs += J.n1 + J.n2; pos2col += J.len1 + J.len2;
		if (rows_form_fits(c, J, MPC_ROWS_PAIRS_MAX, true) && aln_wave_fits(J.C1, J.C2) && njoins > 1) small.push_back(j);
		jn.push_back(J);
	}
	return 0;
}

// where a join's share of each of a chunk's buffers starts (inputs, output rows, cells, traceback codes, reversed path, result record); the longest C1 + 1 so far
struct ChunkAt { u64 in = 0, row = 0, cell = 0, tb = 0, rev = 0, res = 0; u32 lds_rows = 0; };
// A chunk of the small joins js[0..left): as many as keep their matrices within 1 GiB, one join at least. at[q]: where join js[q] starts,
// at.back(): the totals of the at.size() - 1 joins taken.
static std::vector<ChunkAt> cut_join_chunk(const std::vector<JoinIn> &jn, const u32 *js, size_t left)
{
	std::vector<ChunkAt> at(1);
	for (size_t q = 0; q < left; ++q) {
		const JoinIn &j = jn[js[q]];
		ChunkAt t = at.back();
		t.in += rows_slice_bytes(j); t.row += j.C1; t.cell += (u64)j.C1 * j.C2; t.tb += ((u64)j.C1 + 1) * ((u64)j.C2 + 1); t.rev += (u64)j.C1 + j.C2;
		t.res += aln_rec_stride((u64)j.C1 + j.C2); t.lds_rows = std::max(t.lds_rows, j.C1 + 1);
		if (q && t.cell * 4 > ((u64)1 << 30)) break;
		at.push_back(t);
	}
	return at;
}

// One chunk of small joins js[0..at.size() - 1): every matrix in one launch, every alignment in the next. A list overflow of the row form
// (very wide posterior rows) hands nothing out and leaves done[] as it is: the chunk's joins then run one at a time.
static int run_join_chunk(mpcgpu_ctx *c, const std::vector<JoinIn> &jn, const u32 *js, const std::vector<ChunkAt> &at, u32 path_stride, char *paths,
	u32 *pathlens, float *scores, unsigned char *done)
{
	const ChunkAt &all = at.back();
	const u32 nb = (u32)at.size() - 1;
	// one page-locked record, copied to the device once: [rows table][BuildPost parameters][alignment parameters][the joins' inputs]
	const u64 o_rows = 0, o_bp = (o_rows + 8 * all.row + 15) & ~15ull, o_ap = (o_bp + (u64)nb * sizeof(BuildPostRowsParams) + 15) & ~15ull,
		o_in = (o_ap + (u64)nb * sizeof(AlnParams) + 15) & ~15ull, o_err = o_in + all.in, total = o_err + 16;
	HIPCHK(c, c->h_bp_in.ensure(total));
	HIPCHK(c, c->d_bp_in.ensure_grow(total));
	HIPCHK(c, c->d_aln_post.ensure_grow(all.cell * 4));
	HIPCHK(c, c->d_aln_tb.ensure_grow(all.tb));
	HIPCHK(c, c->d_aln_rev.ensure_grow(all.rev));
	HIPCHK(c, c->h_aln_res.ensure(all.res));
	char *hin = c->h_bp_in.as<char>();
	const char *din = c->d_bp_in.as<char>();
	u32 *rows = (u32 *)(hin + o_rows);
	BuildPostRowsParams *bp = (BuildPostRowsParams *)(hin + o_bp);
	AlnParams *ap = (AlnParams *)(hin + o_ap);
	for (u32 q = 0; q < nb; ++q) {
		const JoinIn &j = jn[js[q]];
		if (stage_rows(c, "mpcgpu_align_alns_batch", js[q], j, hin, din, o_in + at[q].in, bp[q])) return 1;
		bp[q].post = c->d_aln_post.as<float>() + at[q].cell; bp[q].err = (u32 *)(din + o_err);
		ap[q] = aln_params(bp[q].post, j.C1, j.C2, c->d_aln_tb.as<char>() + at[q].tb, c->d_aln_rev.as<char>() + at[q].rev, c->h_aln_res.as<char>() + at[q].res);
		for (u32 col = 0; col < j.C1; ++col) { rows[2 * (at[q].row + col)] = q; rows[2 * (at[q].row + col) + 1] = col; }
	}
	memset(hin + o_err, 0, 16);
	HIPCHK(c, hipMemcpyAsync(c->d_bp_in.p, hin, total, hipMemcpyHostToDevice, c->stream));
	const u32 grid = (u32)std::min<u64>(all.row, (u64)c->prop.multiProcessorCount * 32u);
	TimedSpan ts;
	if (span_begin(c, 5, &ts)) return 1;
	if (c->pad_long) MPC_LAUNCH(build_post_rows_batch_long_kernel<8>, grid, 64, 8 * MPC_BPR_CAP, c->stream, (const BuildPostRowsParams *)(din + o_bp), (const u32 *)(din + o_rows), (u32)all.row);
	else MPC_LAUNCH(build_post_rows_batch_kernel<8>, grid, 64, 8 * MPC_BPR_CAP, c->stream, (const BuildPostRowsParams *)(din + o_bp), (const u32 *)(din + o_rows), (u32)all.row);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts)) return 1;
	if (launch_aln_wave_batch(c, (const AlnParams *)(din + o_ap), nb, all.lds_rows)) return 1;
	u32 err = 0;
	HIPCHK(c, hipMemcpyAsync(&err, din + o_err, 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->last_post_cells = 0;
	if (err) return 0;
	for (u32 q = 0; q < nb; ++q) {
		const u32 j = js[q];
		if (aln_rec_read(c, "mpcgpu_align_alns_batch", c->h_aln_res.as<char>() + at[q].res, jn[j].C1, jn[j].C2, paths + (u64)j * path_stride, &pathlens[j],
			scores ? &scores[j] : nullptr)) return 1;
		done[j] = 1;
	}
	return 0;
}

int mpcgpu_align_alns_batch(mpcgpu_ctx *c, uint32_t njoins, const uint32_t *n1, const uint32_t *n2, const uint32_t *C1, const uint32_t *C2,
	const uint32_t *seqs, const uint32_t *pos2col, uint32_t path_stride, char *paths, uint32_t *pathlens, float *scores)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_align_alns_batch: no store (call mpcgpu_build_store / mpcgpu_store_import)");
	if (njoins && (!n1 || !n2 || !C1 || !C2 || !seqs || !pos2col || !paths || !pathlens)) return fail(c, "mpcgpu_align_alns_batch: NULL argument");
	if ((c->partial || c->packed_stale) && mpcgpu_store_complete(c)) return 1;
	HIPCHK(c, hipSetDevice(c->device));
	std::vector<JoinIn> jn;
	std::vector<u32> small;
	if (plan_joins(c, njoins, n1, n2, C1, C2, seqs, pos2col, path_stride, jn, small)) return 1;
	std::vector<unsigned char> done(njoins, 0);
	// ---- the small joins, in chunks whose matrices fit a budget of device memory
	for (size_t s0 = 0; s0 < small.size();) {
		const std::vector<ChunkAt> at = cut_join_chunk(jn, small.data() + s0, small.size() - s0);
		if (run_join_chunk(c, jn, small.data() + s0, at, path_stride, paths, pathlens, scores, done.data())) return 1;
		s0 += at.size() - 1;
	}
	// ---- the others, one after the other
	for (u32 j = 0; j < njoins; ++j)
		if (!done[j] && build_post_impl(c, "mpcgpu_align_alns_batch", jn[j], paths + (u64)j * path_stride, &pathlens[j], scores ? &scores[j] : nullptr)) return 1;
	return 0;
}

int mpcgpu_build_post(mpcgpu_ctx *c, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2, uint32_t C1,
	uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, const float *w1, const float *w2, float *post)
{
	if (!c) return 1;
	if (!post) return fail(c, "mpcgpu_build_post: NULL argument");
	const JoinIn j = {n1, n2, C1, C2, seq1, seq2, pos2col1, pos2col2, w1, w2, 0, 0};
	if (build_post_impl(c, "mpcgpu_build_post", j, nullptr, nullptr, nullptr)) return 1;
	return mpcgpu_get_last_post(c, C1, C2, post);
}

int mpcgpu_get_last_post(mpcgpu_ctx *c, uint32_t C1, uint32_t C2, float *post)
{
	if (!c) return 1;
	if (!post) return fail(c, "mpcgpu_get_last_post: NULL argument");
	if (c->last_post_cells == 0 || (u64)C1 * C2 != c->last_post_cells)
		return fail(c, "mpcgpu_get_last_post: the last matrix built on this context has %llu cells, not %u x %u", (u64)c->last_post_cells, C1, C2);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemcpyAsync(post, c->d_aln_post.p, (size_t)c->last_post_cells * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

int mpcgpu_align_msas(mpcgpu_ctx *c, uint32_t npairs, const uint32_t *seq1, const uint32_t *seq2, uint32_t C1, uint32_t C2,
	const uint32_t *pos2col1, const uint32_t *pos2col2, char *path, uint32_t *pathlen, float *score, float *ea_out)
{
	if (!c) return 1;
	if (c->n == 0) return fail(c, "mpcgpu_align_msas: call mpcgpu_set_seqs / mpcgpu_set_seqs_registry first");
	if (!seq1 || !seq2 || !pos2col1 || !pos2col2 || !path || !pathlen) return fail(c, "mpcgpu_align_msas: NULL argument");
	if (npairs == 0 || C1 == 0 || C2 == 0) return fail(c, "mpcgpu_align_msas: empty input");
	for (u32 q = 0; q < npairs; ++q)
		if (seq1[q] >= c->n || seq2[q] >= c->n) return fail(c, "mpcgpu_align_msas: sequence index out of range in pair %u", q);
	++c->epoch;
	// ---- stage A on the listed pairs (X = the MSA1 sequence, Y = the MSA2 sequence: calcpost.cpp:4-36)
	if (stage_a(c, npairs, seq1, seq2)) return 1;
	if (ea_out) memcpy(ea_out, c->sh_ea.data(), (size_t)npairs * 4);
	// ---- CalcPosteriorFlat3 (buildposterior3flat.cpp:19-85): Flat[col1*C2+col2] += Prob in pair-list order
	std::vector<u64> off1(npairs + 1, 0), off2(npairs + 1, 0), coff(npairs + 1, 0), rbase(npairs + 1, 0);
	rbase[0] = shard_header_bytes(npairs) / 4; // records follow the shard header (words)
	for (u32 q = 0; q < npairs; ++q) {
		off1[q + 1] = off1[q] + c->len[seq1[q]];
		off2[q + 1] = off2[q] + c->len[seq2[q]];
		coff[q + 1] = coff[q] + c->sh_nnz[q];
		rbase[q + 1] = rbase[q] + rec_words(c->len[seq1[q]], c->len[seq2[q]], c->sh_nnz[q]);
	}
	for (u32 q = 0; q < npairs; ++q) // (a row's map must rise strictly, as in build_post_impl)
		if (check_row_map(c, "mpcgpu_align_msas", 1, "in pair", q, pos2col1 + off1[q], c->len[seq1[q]], C1, "")
			|| check_row_map(c, "mpcgpu_align_msas", 2, "in pair", q, pos2col2 + off2[q], c->len[seq2[q]], C2, "")) return 1;
	const u64 M = coff[npairs];
	const u64 cells = (u64)C1 * C2;
	if (cells > 0xffffffffull) return fail(c, "mpcgpu_align_msas: %llu cells exceed this build's cell index", (u64)cells);
	if (M > 0xffffffffull) return fail(c, "mpcgpu_align_msas: %llu contributions exceed this build's record count", (u64)M);
	std::vector<u32> maps(off1[npairs] + off2[npairs]);
	memcpy(maps.data(), pos2col1, off1[npairs] * 4);
	memcpy(maps.data() + off1[npairs], pos2col2, off2[npairs] * 4);
	std::vector<u64> offs(off1);
	offs.insert(offs.end(), off2.begin(), off2.end());
	std::vector<u32> seqs(seq1, seq1 + npairs);
	seqs.insert(seqs.end(), seq2, seq2 + npairs);
	std::vector<u64> bases(coff);
	bases.insert(bases.end(), rbase.begin(), rbase.end());
	if (upload(c, c->d_bp_seq, seqs) || upload(c, c->d_bp_off, offs) || upload(c, c->d_bp_map, maps) || upload(c, c->d_bp_coff, bases))
		return 1;
	HIPCHK(c, c->d_bp_keys.ensure(std::max<u64>(M, 1) * 4 * 2));
	HIPCHK(c, c->d_bp_vals.ensure(std::max<u64>(M, 1) * 4 * 2));
	HIPCHK(c, c->d_aln_post.ensure(cells * 4));
	RunBufs rb;
	if (prepare_runs(c, M, cells, &rb)) return 1;
	BuildPostListParams lp;
	lp.seq_len = c->d_seq_len.as<u32>();
	lp.packed = c->d_shard.as<u32>();
	lp.seq1 = c->d_bp_seq.as<u32>(); lp.seq2 = lp.seq1 + npairs; lp.npairs = npairs;
	lp.p2c1 = c->d_bp_map.as<u32>(); lp.p2c2 = lp.p2c1 + off1[npairs];
	lp.off1 = c->d_bp_off.as<u64>(); lp.off2 = lp.off1 + (npairs + 1);
	lp.coff = c->d_bp_coff.as<u64>(); lp.rbase = lp.coff + (npairs + 1);
	lp.nnz = nullptr; // counts come from coff
	lp.C2 = C2; lp.keys = c->d_bp_keys.as<u32>(); lp.vals = c->d_bp_vals.as<float>();
	lp.post = c->d_aln_post.as<float>(); lp.cells = cells; lp.counters = rb.counters;
	MPC_LAUNCH(build_post_list_gen_kernel, (u32)std::min<u64>(npairs, (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, lp);
	HIPCHK(c, hipGetLastError());
	if (sort_reduce(c, rb, M, cells, false)) return 1;
	c->last_post_cells = cells;
	return run_calc_aln(c, c->d_aln_post.as<float>(), C1, C2, path, pathlen, score); // syncs before the vectors above die
}

// The one-wave alignments of n pairs (sx[q], sy[q]), their dense matrices at off[q] of c->d_aln_post, in ONE launch: parameters in (ap) and a
// record {length, score, path} per pair out (res, aln_rec_stride(Lsum_max) apart) through page-locked memory that the device addresses; one wait.
// ovf: candidate-overflow flags that the same wait brings back (the short list; else NULL): one of them set = 2, nothing handed out.
static int align_wave_batch(mpcgpu_ctx *c, u32 n, const u32 *sx, const u32 *sy, const u64 *off, u32 LXmax, u32 Lsum_max, AlnParams *ap, char *res, const u32 *ovf, u32 path_stride, char *paths, u32 *pathlens, float *scores, float *ea)
{
	const u64 rstride = aln_rec_stride(Lsum_max);
	for (u32 q = 0; q < n; ++q)
		ap[q] = aln_params(c->d_aln_post.as<float>() + off[q], c->len[sx[q]], c->len[sy[q]], nullptr, c->d_aln_rev.as<char>() + (u64)q * Lsum_max, res + (u64)q * rstride);
	if (launch_aln_wave_batch(c, ap, n, LXmax + 1)) return 1;
	HIPCHK(c, hipStreamSynchronize(c->stream)); // the one wait
	for (u32 q = 0; ovf && q < n; ++q) if (ovf[q] & 1u) return 2;
	for (u32 q = 0; q < n; ++q) {
		float sc;
		if (aln_rec_read(c, "mpcgpu_align_pairs", res + (u64)q * rstride, ap[q].LX, ap[q].LY, paths + (u64)q * path_stride, &pathlens[q], &sc)) return 1;
		if (scores) scores[q] = sc;
		if (ea) ea[q] = sc / (float)std::min(ap[q].LX, ap[q].LY); // alignpairflat.cpp:18 (uint -> float, IEEE divide)
	}
	return 0;
}

// ---- the front half of the short-list route, shared by align_pairs_small and search_chunk_fused (mpcgpu_search.inc)
// what the route asks of a list: no row-block pair, every alignment a one-wave alignment, the row-list finishing kernel. Lsum_max: the longest LX + LY
static bool short_list_fits(mpcgpu_ctx *c, const StageAGeom &g, u32 np, const u32 *px, const u32 *py, u32 *Lsum_max)
{
	if (g.LXlong) return false; // row-block pairs
	for (u32 q = 0; q < np; ++q) {
		const u32 LX = c->len[px[q]], LY = c->len[py[q]];
		if (!aln_wave_fits(LX, LY)) return false; // not a one-wave alignment
		*Lsum_max = std::max(*Lsum_max, LX + LY);
	}
	return post_rows_fits(g.LXmax, g.LYmax, 1024);
}
// the context now holds a list stage on these pairs, with nothing packed
static void short_list_mark(mpcgpu_ctx *c, u32 np, const u32 *px, const u32 *py)
{
	c->have_shard = c->have_store = false;
	c->shard_is_list = true;
	c->list_x.assign(px, px + np); c->list_y.assign(py, py + np);
	c->list_q0 = 0; c->ap_x.clear(); c->ap_y.clear();
	c->sh_k0 = 0; c->sh_k1 = np;
}
// the launch order by rows-per-lane bin H: order[np], and hcount[H] = pairs of bin H
static void short_list_order(mpcgpu_ctx *c, u32 np, const u32 *px, u32 *order, u32 *hcount)
{
	std::fill(hcount, hcount + MPC_HMAX + 1, 0u);
	std::vector<u32> keys(np);
	for (u32 q = 0; q < np; ++q) { const u32 H = (c->len[px[q]] + 63) / 64; hcount[H]++; keys[q] = (H << 16) | q; }
	std::sort(keys.begin(), keys.end());
	for (u32 q = 0; q < np; ++q) order[q] = keys[q] & 0xffffu;
}
// forward / backward, one launch per rows-per-lane bin; then probabilities, EA, sparsify (the candidate lists keep the probabilities): a
// workgroup per pair, the knobs of the general stage ignored. io, order: as the device reads them
static int short_list_sweeps(mpcgpu_ctx *c, const StageAGeom &g, const PostIO &io, const u32 *order, const u32 *hcount)
{
	FbParams fp;
	fill_fb_params(c, fp, io.pair_x, io.pair_y, g.capc, g.mega);
	if (launch_fb_bins(c, g, fp, order, hcount, 0)) return 1;
	return launch_post_rows(c, g, io, 1024, 64, io.count, c->d_sort_scratch, true);
}

// mpcgpu_align_pairs for a SHORT list (what UClust::Search and single AlignPairFlat calls send: 1..8 pairs): the kernels of the
// general path, driven with one wait. Everything the kernels read from the host (pair list, launch order, alignment parameters)
// and everything the host reads back (candidate-overflow flags, path records) lives in ONE page-locked record that the device
// addresses directly; nothing is packed into a shard (mpcgpu_get_list_sparse re-runs the general stage when somebody asks).
// 0 = done, 1 = error, 2 = not applicable (the caller takes the general path).
static int align_pairs_small(mpcgpu_ctx *c, u32 np, const u32 *px, const u32 *py, u32 path_stride, char *paths, u32 *pathlens,
	float *scores, float *ea)
{
	const StageAGeom g = stage_a_geom(c, np, px, py);
	u32 Lsum_max = 0;
	if (!short_list_fits(c, g, np, px, py, &Lsum_max)) return 2;
	short_list_mark(c, np, px, py);
	c->se.last = false;
	// ---- the page-locked record
	std::vector<u64> off(np + 1, 0);
	for (u32 q = 0; q < np; ++q) off[q + 1] = off[q] + (u64)c->len[px[q]] * c->len[py[q]];
	const u64 o_bx = 0, o_by = o_bx + 4 * (u64)np, o_order = o_by + 4 * (u64)np, o_off = (o_order + 4 * (u64)np + 7) & ~7ull,
		o_par = o_off + 8 * ((u64)np + 1), o_flags = o_par + (u64)np * sizeof(AlnParams), o_nnz = o_flags + 4 * (u64)np,
		o_ea = o_nnz + 4 * (u64)np, o_res = (o_ea + 4 * (u64)np + 7) & ~7ull, bytes = o_res + (u64)np * aln_rec_stride(Lsum_max);
	HIPCHK(c, c->h_ap.ensure(bytes));
	char *h = c->h_ap.as<char>();
	u32 *bx = (u32 *)(h + o_bx), *by = (u32 *)(h + o_by), *order = (u32 *)(h + o_order);
	memcpy(bx, px, 4 * (size_t)np);
	memcpy(by, py, 4 * (size_t)np);
	memcpy(h + o_off, off.data(), 8 * ((size_t)np + 1));
	u32 hcount[MPC_HMAX + 1];
	short_list_order(c, np, px, order, hcount);
	// ---- scratch
	if (ensure_pair_scratch(c, g, np)) return 1;
	HIPCHK(c, c->d_aln_post.ensure_grow(off[np] * 4));
	HIPCHK(c, c->d_aln_rev.ensure_grow((u64)np * Lsum_max + 16));
	// ---- sweeps and finishing kernel: sizes, EAs and flags straight into the record
	const PostIO io = {bx, by, c->d_seq_len.as<u32>(), c->d_cand.as<u64>(), c->d_cand_cnt.as<u32>(), c->d_res.as<u32>(), (u32 *)(h + o_nnz), (float *)(h + o_ea), (u32 *)(h + o_flags), np};
	if (short_list_sweeps(c, g, io, order, hcount)) return 1;
	// ---- dense thresholded posteriors, alignments
	DensePostParams dp;
	dp.pair_x = bx; dp.pair_y = by; dp.seq_len = c->d_seq_len.as<u32>();
	dp.cand = c->d_cand.as<u64>(); dp.capc = g.capc; dp.cand_cnt = c->d_cand_cnt.as<u32>(); dp.long_min = g.long_min;
	dp.out_off = (const u64 *)(h + o_off); dp.out = c->d_aln_post.as<float>();
	MPC_LAUNCH(dense_post_kernel, np, 256, 0, c->stream, dp);
	HIPCHK(c, hipGetLastError());
	c->last_post_cells = 0;
	const int rc = align_wave_batch(c, np, px, py, off.data(), g.LXmax, Lsum_max, (AlnParams *)(h + o_par), h + o_res, (const u32 *)(h + o_flags), path_stride, paths, pathlens, scores, ea);
	if (rc) return rc; // (2: a candidate list overflowed: the general path grows it and retries)
	c->sh_nnz.assign((const u32 *)(h + o_nnz), (const u32 *)(h + o_nnz) + np);
	c->sh_ea.assign((const float *)(h + o_ea), (const float *)(h + o_ea) + np);
	return 0;
}

// How many of the first nq pairs of (sx, sy) keep their dense matrices (LX * LY floats each) together in d_aln_post: a chunk whose matrices
// do not fit half of what is free (long pairs: 1.6 GB for 20 000 x 20 000) is halved like one that stage A has to split, down to a single pair
static int pairs_that_fit(mpcgpu_ctx *c, const u32 *sx, const u32 *sy, u32 *nq)
{
	size_t freeb = 0, totb = 0;
	HIPCHK(c, hipMemGetInfo(&freeb, &totb));
	const u64 room = (u64)((freeb + c->d_aln_post.cap) * 0.5);
	auto bytes_of = [&](u32 k) { u64 b = 0; for (u32 q = 0; q < k; ++q) b += (u64)c->len[sx[q]] * c->len[sy[q]] * 4; return b; };
	while (*nq > 1 && bytes_of(*nq) > room) *nq = (*nq + 1) / 2;
	return 0;
}

// The dense thresholded posteriors of the nq pairs of the stage-A batch just run, pair q at off[q] of d_aln_post, rebuilt from the
// candidate lists the batch left behind (every cell with Score >= MIN_SPARSE_SCORE, also those FromPost drops). d_pick (mpcgpu_search_pairs):
// matrix q is that of pair d_pick[q] of the batch, read on the device; NULL: of pair q. refusal: the entry point's words under MPCGPU_POST=sort
static int dense_posts(mpcgpu_ctx *c, const char *refusal, u32 nq, const std::vector<u64> &off, const u32 *d_pick)
{
	// Without the row-list finishing kernel the candidate lists still hold the scores (post_kernel sorts a copy): the raw builder forms
	// the probabilities itself. Only a list that does not FIT the row-list kernel goes that way; MPCGPU_POST=sort stays a refusal.
	const char *post_mode = getenv("MPCGPU_POST");
	if (!c->sa_post_rows && post_mode && !strcmp(post_mode, "sort")) return fail(c, "%s", refusal);
	HIPCHK(c, c->d_aln_post.ensure_grow(off[nq] * 4));
	if (upload(c, c->d_ap_off, off)) return 1;
	DensePostParams dp;
	dp.pair_x = c->d_bx.as<u32>(); dp.pair_y = c->d_by.as<u32>(); dp.seq_len = c->d_seq_len.as<u32>();
	dp.cand = c->d_cand.as<u64>(); dp.capc = c->sa_capc; dp.cand_cnt = c->d_cand_cnt.as<u32>(); dp.long_min = c->sa_long_min;
	dp.out_off = c->d_ap_off.as<u64>(); dp.out = c->d_aln_post.as<float>();
	if (c->sa_post_rows) {
		if (d_pick) MPC_LAUNCH(dense_post_pick_kernel, nq, 256, 0, c->stream, DensePostPickParams{dp, d_pick});
		else MPC_LAUNCH(dense_post_kernel, nq, 256, 0, c->stream, dp);
	} else {
		// zeroes by one memset on the stream, the scatter on (pairs) x (slabs of 256 candidates, as many as keep the chip busy)
		const u32 slabs = (u32)std::max<u64>(1, std::min<u64>(((u64)c->sa_capc + 255) / 256, ((u64)c->prop.multiProcessorCount * 8 + nq - 1) / nq));
		const DensePostRawParams rp = {dp, c->use_fma, slabs};
		// (the trace line and the timed span are mpcgpu_align_pairs' alone: mpcgpu_search_pairs counts no launch in slot 5)
		if (!d_pick && trace_on()) { fprintf(stderr, "[mpcgpu] align_pairs dense posteriors from raw candidates: %u pairs x %u slabs, %.1f MB\n", nq, slabs, (double)off[nq] * 4 / 1048576.0); fflush(stderr); }
		TimedSpan ts_dense;
		if (!d_pick && span_begin(c, 5, &ts_dense)) return 1;
		HIPCHK(c, hipMemsetAsync(c->d_aln_post.p, 0, off[nq] * 4, c->stream));
		if (d_pick) MPC_LAUNCH(dense_post_raw_pick_kernel, nq * slabs, 256, 0, c->stream, DensePostRawPickParams{rp, d_pick});
		else MPC_LAUNCH(dense_post_raw_kernel, nq * slabs, 256, 0, c->stream, rp);
		HIPCHK(c, hipGetLastError());
		if (!d_pick && span_end(c, &ts_dense)) return 1;
	}
	HIPCHK(c, hipGetLastError());
	c->last_post_cells = 0; // several matrices: not what mpcgpu_get_last_post hands out
	return 0;
}

// CalcAlnFlat on the nq dense matrices: one wavefront each in ONE launch when they all fit, else one after the other
static int align_dense(mpcgpu_ctx *c, u32 nq, const u32 *sx, const u32 *sy, const std::vector<u64> &off, u32 path_stride, char *paths, u32 *pathlens, float *scores, float *ea)
{
	u32 Lsum_max = 0, LXmax = 0;
	bool all_wave = true;
	for (u32 q = 0; q < nq; ++q) {
		const u32 LX = c->len[sx[q]], LY = c->len[sy[q]];
		Lsum_max = std::max(Lsum_max, LX + LY);
		LXmax = std::max(LXmax, LX);
		all_wave = all_wave && aln_wave_fits(LX, LY);
	}
	if (all_wave) {
		// one launch: parameters in, {length, score, path} out through page-locked memory
		HIPCHK(c, c->h_ap.ensure((u64)nq * (sizeof(AlnParams) + aln_rec_stride(Lsum_max))));
		HIPCHK(c, c->d_aln_rev.ensure_grow((u64)nq * Lsum_max + 16));
		AlnParams *ap = c->h_ap.as<AlnParams>();
		return align_wave_batch(c, nq, sx, sy, off.data(), LXmax, Lsum_max, ap, (char *)(ap + nq), nullptr, path_stride, paths, pathlens, scores, ea);
	}
	for (u32 q = 0; q < nq; ++q) {
		const u32 LX = c->len[sx[q]], LY = c->len[sy[q]];
		float sc = 0;
		if (run_calc_aln(c, c->d_aln_post.as<float>() + off[q], LX, LY, paths + (u64)q * path_stride, &pathlens[q], &sc)) return 1;
		if (scores) scores[q] = sc;
		if (ea) ea[q] = sc / (float)std::min(LX, LY);
	}
	return 0;
}

struct KeepList { mpcgpu_ctx *c; ~KeepList() { c->ap_keep = false; } }; // c->ap_keep (set by the owner) is dropped on every way out
// AlignPairFlat (alignpairflat.cpp:3-27) for a list of pairs: CalcPost (fwd + bwd + CalcPostFlat, calcpost.cpp:4-36) -> CalcAlnFlat on
// the DENSE thresholded posterior -> path; EA = Score / min(L1, L2). Stage A runs on the list (the kernels of
// mpcgpu_calc_posteriors), the dense matrices are rebuilt from the candidate lists (dense_posts), the alignments run one wavefront
// each in ONE launch when they fit (else one after the other: align_dense).
int mpcgpu_align_pairs(mpcgpu_ctx *c, uint32_t npairs, const uint32_t *seq1, const uint32_t *seq2, uint32_t path_stride, char *paths,
	uint32_t *pathlens, float *scores, float *ea)
{
	if (!c) return 1;
	if (c->n == 0) return fail(c, "mpcgpu_align_pairs: call mpcgpu_set_seqs / mpcgpu_set_seqs_registry first");
	if (!seq1 || !seq2 || !paths || !pathlens) return fail(c, "mpcgpu_align_pairs: NULL argument");
	for (u32 q = 0; q < npairs; ++q) {
		if (seq1[q] >= c->n || seq2[q] >= c->n) return fail(c, "mpcgpu_align_pairs: sequence index out of range in pair %u", q);
		if ((u64)c->len[seq1[q]] + c->len[seq2[q]] > path_stride) return fail(c, "mpcgpu_align_pairs: path_stride %u too small for pair %u", path_stride, q);
	}
	// the reference's own limit on a dense posterior (calcposteriorflat.cpp:54-61), before any device work
	for (u32 q = 0; q < npairs; ++q) {
		const u32 LX = c->len[seq1[q]], LY = c->len[seq2[q]];
		if (double(LX) * double(LY) * 5 + 100 > double(INT_MAX))
			return fail(c, "mpcgpu_align_pairs: pair %u is too long for a dense posterior: LX=%u, LY=%u, LX*LY*5 + 100 exceeds INT_MAX = %d", q, LX, LY, INT_MAX);
	}
	HIPCHK(c, hipSetDevice(c->device));
	++c->epoch;
	if (npairs >= 1 && npairs <= 64 && env_int("MPCGPU_PAIRS_SMALL", 1)) {
		const int rc = align_pairs_small(c, npairs, seq1, seq2, path_stride, paths, pathlens, scores, ea);
		if (rc != 2) return rc;
	}
	u32 chunk = 256; // pairs per stage-A call: their dense matrices (LX*LY floats each) live together
	KeepList keep_guard{c};
	c->ap_keep = true;
	c->ap_x.assign(seq1, seq1 + npairs); c->ap_y.assign(seq2, seq2 + npairs);
	for (u32 q0 = 0; q0 < npairs;) {
		const u32 *sx = seq1 + q0, *sy = seq2 + q0;
		u32 nq = std::min<u32>(chunk, npairs - q0);
		if (pairs_that_fit(c, sx, sy, &nq)) return 1;
		// the dense matrices are rebuilt from the candidate lists ONE stage-A batch leaves behind: a chunk that stage A had to
		// cut into several batches (long sequences, little free memory) is halved and run again, down to a single pair
		for (;;) {
			if (stage_a(c, nq, sx, sy)) return 1;
			c->list_q0 = q0; // what the last stage holds is pairs [q0, q0 + nq) of the caller's list
			if (c->sa_b0 == 0 && c->sa_B == nq) break;
			if (nq == 1) return fail(c, "mpcgpu_align_pairs: pair %u (%u x %u residues) does not fit one stage-A batch", q0, c->len[sx[0]], c->len[sy[0]]);
			nq = (nq + 1) / 2;
		}
		chunk = std::min(chunk, nq); // a halved chunk stays halved
		std::vector<u64> off(nq + 1, 0);
		for (u32 q = 0; q < nq; ++q) off[q + 1] = off[q] + (u64)c->len[sx[q]] * c->len[sy[q]];
		if (dense_posts(c, "mpcgpu_align_pairs: pair list with a sequence of more than ~12 000 residues (or MPCGPU_POST=sort): the row-list finishing kernel "
			"whose candidate lists this entry point rebuilds the dense posteriors from does not take them", nq, off, nullptr)) return 1;
		if (align_dense(c, nq, sx, sy, off, path_stride, paths + (u64)q0 * path_stride, pathlens + q0, scores ? scores + q0 : nullptr, ea ? ea + q0 : nullptr)) return 1;
		q0 += nq;
	}
	return 0;
}

int mpcgpu_get_list_sparse(mpcgpu_ctx *c, uint32_t q, uint32_t *nnz, uint32_t *offsets, void *values)
{
	if (!c) return 1;
	if (!c->shard_is_list) return fail(c, "mpcgpu_get_list_sparse: no list stage holds pair %u", q);
	if (c->se.last) return fail(c, "mpcgpu_get_list_sparse: the last list stage was mpcgpu_search_pairs, which keeps no sparse matrices (pair %u)", q);
	HIPCHK(c, hipSetDevice(c->device));
	// q indexes the list the CALLER passed. mpcgpu_align_pairs may have run that list in chunks (256 pairs, halved when stage A had to
	// split one): the last stage then holds pairs [list_q0, list_q0 + list_x.size()) of it. A pair outside that window gets a stage
	// of its own (same kernels, same bits) — never another pair's record.
	const bool want_record = offsets && values;
	if (c->ap_x.empty() && !c->have_shard && want_record) { c->ap_x = c->list_x; c->ap_y = c->list_y; c->list_q0 = 0; } // the short-list path packed nothing
	u32 ql = q;
	if (!c->ap_x.empty()) {
		if (q >= c->ap_x.size()) return fail(c, "mpcgpu_get_list_sparse: no list stage holds pair %u", q);
		KeepList keep_guard{c};
		c->ap_keep = true;
		bool inside = q >= c->list_q0 && q - c->list_q0 < c->list_x.size();
		if (inside && !c->have_shard && want_record) { // the general stage on the window's list packs the records
			const std::vector<u32> lx = c->list_x, ly = c->list_y;
			const u32 q0 = c->list_q0;
			if (stage_a(c, lx.size(), lx.data(), ly.data())) return 1;
			c->list_q0 = q0;
			inside = c->sa_b0 == 0 && c->sa_B == lx.size(); // (split into batches: the shard holds the last batch only)
		}
		if (!inside) {
			// the whole chunk that holds q is staged again and stays resident (a caller that reads q = 0, 1, 2 ... in order pays one stage
			// per 256 pairs, not one per pair: round-5 advisor finding); a chunk that stage A has to split falls back to the single pair
			const u32 q0 = (q / 256u) * 256u, nq = (u32)std::min<size_t>(256u, c->ap_x.size() - q0);
			const std::vector<u32> lx(c->ap_x.begin() + q0, c->ap_x.begin() + q0 + nq), ly(c->ap_y.begin() + q0, c->ap_y.begin() + q0 + nq);
			if (stage_a(c, nq, lx.data(), ly.data())) return 1;
			c->list_q0 = q0;
			if (!(c->sa_b0 == 0 && c->sa_B == nq)) {
				const u32 x = c->ap_x[q], y = c->ap_y[q];
				if (stage_a(c, 1, &x, &y)) return 1;
				c->list_q0 = q;
			}
		}
		ql = q - c->list_q0;
	}
	if (ql >= c->list_x.size() || ql >= c->sh_nnz.size()) return fail(c, "mpcgpu_get_list_sparse: no list stage holds pair %u", q);
	const u64 np = c->list_x.size();
	u64 w = shard_header_bytes(np) / 4;
	for (u32 k = 0; k < ql; ++k) w += rec_words(c->len[c->list_x[k]], c->len[c->list_y[k]], c->sh_nnz[k]);
	const u32 LX = c->len[c->list_x[ql]], LY = c->len[c->list_y[ql]], nz = c->sh_nnz[ql];
	if (nnz) *nnz = nz;
	if (!want_record) return 0;
	if (!c->have_shard) return fail(c, "mpcgpu_get_list_sparse: the list stage of pair %u left no packed records (internal error)", q);
	std::vector<u32> rowcnt(LX);
	HIPCHK(c, hipMemcpyAsync(rowcnt.data(), c->d_shard.as<u32>() + w, (size_t)LX * 4, hipMemcpyDeviceToHost, c->stream));
	if (nz) HIPCHK(c, hipMemcpyAsync(values, c->d_shard.as<u32>() + w + LX + LY, (size_t)nz * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	u32 acc = 0;
	for (u32 i = 0; i < LX; ++i) { offsets[i] = acc; acc += rowcnt[i]; }
	offsets[LX] = acc;
	if (acc != nz) return fail(c, "mpcgpu_get_list_sparse: record of pair %u is inconsistent (internal error)", q);
	return 0;
}


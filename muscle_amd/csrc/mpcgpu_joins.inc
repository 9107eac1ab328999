// mpcgpu_joins.inc — alignment of alignments on the device store: CalcAlnFlat, BuildPost, AlignAlns, the PProg join and pair lists
// (part of mpcgpu.cpp's translation unit). Reference: alnalnsflat.cpp:7-52, buildpostflat.cpp:18-106, alnmsasflat.cpp:4-50, alignpairflat.cpp:3-27.
// CalcAlnFlat + TraceBackFlat on a dense LX x LY matrix already in device memory
static int run_calc_aln(mpcgpu_ctx *c, const float *d_post, uint32_t LX, uint32_t LY, char *path, uint32_t *pathlen, float *score)
{
	const u64 W = (u64)LY + 1;
	// one wavefront with the previous row in registers and the traceback codes in LDS when the matrix is small enough
	// (the progressive joins and refinement rounds of L~400 families are), else the workgroup kernel
	const size_t smem_wave = (size_t)(LX + 1) * MPC_ALNW_ROWBYTES + 16;
	const int pick = env_int("MPCGPU_ALN_KERNEL", 0); // 0 = by size, 1 = one wave, 2 = several waves, 3 = LDS rows, 4 = LDS rows in column tiles
	const bool wave = W <= MPC_ALNW_MAXW && smem_wave <= 160u * 1024u && (pick == 0 || pick == 1);
	// several waves, 4 columns per thread, previous row in registers: up to 4096 columns
	const u32 qthreads = (u32)((W + 4 * 64 - 1) / (4 * 64)) * 64;
	const bool quad = !wave && qthreads <= 1024 && (pick == 0 || pick == 2);
	const u32 qrows = quad ? (u32)std::min<u64>((u64)LX + 1, (150u * 1024u) / qthreads) : 0;
	// two DP rows of LY + 1 floats in LDS; wider than that (or MPCGPU_ALN_KERNEL=4): the same rows in column tiles, the tile's left
	// edge carried through device memory (calc_aln_tiled_kernel). MPCGPU_ALN_TILE: columns per tile (tests: several tiles of a small matrix)
	const size_t smem_rows = (size_t)(2 * W + MPC_ALN_THREADS / 64 + 4) * 4;
	const bool tiled = !wave && !quad && (pick == 4 || smem_rows > 160u * 1024u);
	const u32 tile = tiled ? (u32)std::min<u64>(W, (u64)std::min(std::max(env_int("MPCGPU_ALN_TILE", 16384), 1), 16384)) : 0;
	const size_t smem = wave ? smem_wave : quad ? (size_t)MPC_ALNQ_HDR + (size_t)qrows * qthreads : tiled ? (size_t)(2 * ((u64)tile + 1) + MPC_ALN_THREADS / 64 + 4) * 4 : smem_rows;
	if (tiled) HIPCHK(c, c->d_aln_bnd.ensure_grow(2 * ((u64)LX + 1) * 4));
	HIPCHK(c, c->d_aln_tb.ensure_grow(((u64)LX + 1) * (quad ? (u64)qthreads : W))); // letters per cell, or one byte per thread and row
	HIPCHK(c, c->d_aln_rev.ensure_grow((u64)LX + LY));
	// one result record {path length, score, path}: one copy back, one wait
	const u64 res_bytes = 8 + (u64)LX + LY;
	HIPCHK(c, c->h_aln_res.ensure(res_bytes));
	AlnParams ap;
	ap.post = d_post; ap.LX = LX; ap.LY = LY;
	ap.tb = c->d_aln_tb.as<char>(); ap.rev = c->d_aln_rev.as<char>();
	// the record is written straight into page-locked host memory (device-visible: hipHostMalloc): no copy back, one wait
	ap.pathlen = c->h_aln_res.as<u32>(); ap.score = c->h_aln_res.as<float>() + 1; ap.path = c->h_aln_res.as<char>() + 8;
	const int which = wave ? 0 : quad ? 1 : tiled ? 4 : 2;
	if (smem > c->aln_smem_set[which]) { // raise the kernel's dynamic-LDS limit only when this call needs more than any before
		(void)hipFuncSetAttribute(wave ? (const void *)calc_aln_wave_kernel : quad ? (const void *)calc_aln_quad_kernel : tiled ? (const void *)calc_aln_tiled_kernel : (const void *)calc_aln_kernel,
			hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
		c->aln_smem_set[which] = smem;
	}
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
	const u32 n_path = c->h_aln_res.as<u32>()[0];
	if (n_path > LX + LY) return fail(c, "mpcgpu_calc_aln: path length %u out of range (internal error)", n_path);
	*pathlen = n_path;
	if (score) memcpy(score, c->h_aln_res.as<char>() + 4, 4);
	memcpy(path, c->h_aln_res.as<char>() + 8, n_path);
	return 0;
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
	HIPCHK(c, hipSetDevice(c->device));
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
		} else {
			PostParams pp;
			const size_t psmem = fill_post(c, g, io, 1024, pp);
			if (d_sort.ensure(pp.sort_stride * 8) != hipSuccess || d_srow.ensure(pp.srow_stride * 4) != hipSuccess) { rc = fail(c, "mpcgpu_post_scores: out of device memory"); break; }
			pp.sort_scratch = d_sort.as<u64>(); pp.srow_scratch = d_srow.as<float>();
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

// BuildPost on the device store (+ CalcAlnFlat when path != NULL): the body of mpcgpu_align_alns_w and mpcgpu_build_post (who: the
// entry point, for the messages about the caller's maps). A row's position -> column map must rise strictly (Sequence::GetPosToCol of
// an aligned row): two positions on one column would add twice into one cell of the matrix.
static int build_post_impl(mpcgpu_ctx *c, const char *who, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2, uint32_t C1,
	uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, const float *w1, const float *w2, char *path,
	uint32_t *pathlen, float *score)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_align_alns: no store (call mpcgpu_build_store / mpcgpu_store_import)");
	// BuildPost reads the records of any sequence: a partial store (a rank of a block-partitioned run) is completed first — once,
	// from the packed records, which hold the current values
	if ((c->partial || c->packed_stale) && mpcgpu_store_complete(c)) return 1;
	if (!seq1 || !seq2 || !pos2col1 || !pos2col2 || (path && !pathlen)) return fail(c, "mpcgpu_align_alns: NULL argument");
	if (n1 == 0 || n2 == 0 || C1 == 0 || C2 == 0) return fail(c, "mpcgpu_align_alns: empty alignment");
	HIPCHK(c, hipSetDevice(c->device));
	const u32 n = c->n;
	static const bool host_trace = trace_host(); // diagnostics: host wall time of this call's phases, summed
	double *acc_t = c->aa_trace_t; // per context: the shrub workers of -super7 call this concurrently on their own contexts
	u64 &acc_n = c->aa_trace_n;
	auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	double t_prev = host_trace ? now() : 0.0;
	auto lap = [&](int k) { if (host_trace) { const double t = now(); acc_t[k] += t - t_prev; t_prev = t; } };
	// ---- host: everything the kernels need from this call in ONE page-locked record, one copy:
	// [off: n1+n2+1 u64][coff: n1*n2+1 u64][seqs: n1+n2 u32][maps: len1+len2 u32][weights: n1+n2 f32, when not all 1.0f]
	u64 len1 = 0, len2 = 0;
	for (u32 a = 0; a < n1; ++a) {
		if (seq1[a] >= n) return fail(c, "mpcgpu_align_alns: sequence index %u out of range", seq1[a]);
		len1 += c->len[seq1[a]];
	}
	for (u32 b = 0; b < n2; ++b) {
		if (seq2[b] >= n) return fail(c, "mpcgpu_align_alns: sequence index %u out of range", seq2[b]);
		len2 += c->len[seq2[b]];
	}
	if ((w1 != nullptr) != (w2 != nullptr)) return fail(c, "mpcgpu_align_alns_w: give both weight arrays or neither");
	bool weighted = false; // all 1.0f (what MPCFlat::Run sets): (1*1)*P == P, skip the multiply
	if (w1) {
		for (u32 a = 0; a < n1; ++a) weighted = weighted || w1[a] != 1.0f;
		for (u32 b = 0; b < n2; ++b) weighted = weighted || w2[b] != 1.0f;
	}
	const u64 npairs12 = (u64)n1 * n2;
	// ---- small joins: the whole matrix in one launch, inputs read from page-locked host memory (kernels_prog.h:
	// build_post_rows_kernel). Needs the variable-size record store (every ordered pair by row).
	{
		const char *bp_mode = getenv("MPCGPU_BP"); // "sort": always the general path; "rows": the row kernel whenever its limits allow
		const bool want_rows = !(bp_mode && !strcmp(bp_mode, "sort"));
		const u64 pair_limit = (bp_mode && !strcmp(bp_mode, "rows")) ? ~0ull : 2048;
		if (want_rows && c->have_pad && npairs12 <= pair_limit && C2 <= 1024u && (u64)n1 * C1 <= (1u << 26)) {
			const u64 r_seqs = 0, r_c2p = r_seqs + 4 * ((u64)n1 + n2), r_off2 = r_c2p + 4 * (u64)n1 * C1, r_maps = r_off2 + 4 * ((u64)n2 + 1),
				r_w = r_maps + 4 * len2, r_err = r_w + (weighted ? 4 * ((u64)n1 + n2) : 0), r_bytes = r_err + 4;
			HIPCHK(c, c->h_bp_in.ensure(r_bytes));
			char *hin = c->h_bp_in.as<char>();
			u32 *seqs = (u32 *)(hin + r_seqs), *c2p = (u32 *)(hin + r_c2p), *off2 = (u32 *)(hin + r_off2), *maps2 = (u32 *)(hin + r_maps);
			memcpy(seqs, seq1, 4 * (size_t)n1);
			memcpy(seqs + n1, seq2, 4 * (size_t)n2);
			for (u64 q = 0; q < (u64)n1 * C1; ++q) c2p[q] = MPC_BPR_GAP;
			u64 at = 0;
			for (u32 a = 0; a < n1; ++a) {
				const u32 L = c->len[seq1[a]];
				for (u32 pos = 0; pos < L; ++pos) {
					const u32 col = pos2col1[at + pos];
					if (col >= C1) return fail(c, "%s: column map of MSA1 out of range", who);
					if (pos && col <= pos2col1[at + pos - 1]) return fail(c, "%s: column map of MSA1 row %u is not strictly increasing at position %u", who, a, pos);
					c2p[(u64)a * C1 + col] = pos;
				}
				at += L;
			}
			off2[0] = 0;
			for (u32 b = 0; b < n2; ++b) off2[b + 1] = off2[b] + c->len[seq2[b]];
			memcpy(maps2, pos2col2, 4 * len2);
			for (u32 b = 0; b < n2; ++b)
				for (u32 q = off2[b]; q < off2[b + 1]; ++q) {
					if (maps2[q] >= C2) return fail(c, "%s: column map of MSA2 out of range", who);
					if (q > off2[b] && maps2[q] <= maps2[q - 1]) return fail(c, "%s: column map of MSA2 row %u is not strictly increasing at position %u", who, b, q - off2[b]);
				}
			for (u32 a = 0; a < n1; ++a)
				for (u32 b = 0; b < n2; ++b) if (seq1[a] == seq2[b]) return fail(c, "mpcgpu_align_alns: sequence %u is in both alignments", seq1[a]);
			if (weighted) {
				float *w = (float *)(hin + r_w);
				memcpy(w, w1, 4 * (size_t)n1);
				memcpy(w + n1, w2, 4 * (size_t)n2);
			}
			*(u32 *)(hin + r_err) = 0u;
			lap(0);
			const u64 cells = (u64)C1 * C2;
			HIPCHK(c, c->d_aln_post.ensure_grow(cells * 4));
			BuildPostRowsParams rp;
			fill_store_params(c, rp.s);
			rp.seq1 = seqs; rp.seq2 = seqs + n1; rp.n1 = n1; rp.n2 = n2;
			rp.c2p1 = c2p; rp.p2c2 = maps2; rp.off2 = off2; rp.C1 = C1; rp.C2 = C2;
			rp.w1 = weighted ? (const float *)(hin + r_w) : nullptr; rp.w2 = weighted ? rp.w1 + n1 : nullptr;
			rp.post = c->d_aln_post.as<float>(); rp.err = (u32 *)(hin + r_err);
			const u32 grid = std::min<u32>(C1, (u32)c->prop.multiProcessorCount * 8u);
			if (trace_on()) { fprintf(stderr, "[mpcgpu] build_post %u x %u rows, %u x %u columns: row kernel, grid %u\n", n1, n2, C1, C2, grid); fflush(stderr); }
			TimedSpan ts_rows;
			if (span_begin(c, 5, &ts_rows)) return 1;
			if (C2 <= 512u) MPC_LAUNCH(build_post_rows_kernel<8>, grid, 64, 8 * MPC_BPR_CAP, c->stream, rp);
			else MPC_LAUNCH(build_post_rows_kernel<16>, grid, 64, 8 * MPC_BPR_CAP, c->stream, rp);
			HIPCHK(c, hipGetLastError());
			if (span_end(c, &ts_rows)) return 1;
			lap(2);
			c->last_post_cells = cells;
			int rc_rows = 0;
			if (!path) HIPCHK(c, hipStreamSynchronize(c->stream));
			else rc_rows = run_calc_aln(c, c->d_aln_post.as<float>(), C1, C2, path, pathlen, score); // ends with a wait for the stream
			lap(3);
			if (*(volatile u32 *)(hin + r_err) == 0u) return rc_rows;
			// a chunk of pairs overflowed the row kernel's list (very wide posterior rows): the general path below redoes the join
		}
	}
	const u64 o_off = 0, o_coff = o_off + 8 * ((u64)n1 + n2 + 1), o_seqs = o_coff + 8 * (npairs12 + 1), o_maps = o_seqs + 4 * ((u64)n1 + n2),
		o_w = o_maps + 4 * (len1 + len2), in_bytes = o_w + (weighted ? 4 * ((u64)n1 + n2) : 0);
	HIPCHK(c, c->h_bp_in.ensure(in_bytes));
	char *hin = c->h_bp_in.as<char>();
	u64 *off = (u64 *)(hin + o_off), *coff = (u64 *)(hin + o_coff);
	u32 *seqs = (u32 *)(hin + o_seqs), *maps = (u32 *)(hin + o_maps);
	memcpy(seqs, seq1, 4 * (size_t)n1);
	memcpy(seqs + n1, seq2, 4 * (size_t)n2);
	off[0] = 0;
	for (u32 a = 0; a < n1 + n2; ++a) off[a + 1] = off[a] + c->len[seqs[a]];
	memcpy(maps, pos2col1, len1 * 4);
	memcpy(maps + len1, pos2col2, len2 * 4);
	for (u32 a = 0; a < n1 + n2; ++a) {
		const u32 C = a < n1 ? C1 : C2, side = a < n1 ? 1 : 2, row = a < n1 ? a : a - n1;
		for (u64 q = off[a]; q < off[a + 1]; ++q) {
			if (maps[q] >= C) return fail(c, "%s: column map of MSA%u out of range", who, side);
			if (q > off[a] && maps[q] <= maps[q - 1]) return fail(c, "%s: column map of MSA%u row %u is not strictly increasing at position %u", who, side, row, (u32)(q - off[a]));
		}
	}
	coff[0] = 0;
	for (u32 a = 0; a < n1; ++a)
		for (u32 b = 0; b < n2; ++b) {
			const u32 S = seqs[a], T = seqs[n1 + b];
			if (S == T) return fail(c, "mpcgpu_align_alns: sequence %u is in both alignments", S);
			const u64 k = S < T ? pair_pos(c, S, T) : pair_pos(c, T, S); // (position in the context's pair order: all_nnz is kept in it)
			coff[(u64)a * n2 + b + 1] = coff[(u64)a * n2 + b] + c->all_nnz[k];
		}
	if (weighted) {
		float *w = (float *)(hin + o_w);
		memcpy(w, w1, 4 * (size_t)n1);
		memcpy(w + n1, w2, 4 * (size_t)n2);
	}
	const u64 M = coff[npairs12];
	const u64 cells = (u64)C1 * C2;
	if (cells > 0xffffffffull) return fail(c, "mpcgpu_align_alns: %llu cells exceed this build's cell index", (u64)cells);
	const u32 bc = bits_for(cells - 1);
	if (M > 0xffffffffull) return fail(c, "mpcgpu_align_alns: %llu contributions exceed this build's record count", (u64)M);
	lap(0);
	HIPCHK(c, c->d_bp_in.ensure_grow(in_bytes));
	HIPCHK(c, hipMemcpyAsync(c->d_bp_in.p, hin, in_bytes, hipMemcpyHostToDevice, c->stream));
	lap(1);
	HIPCHK(c, c->d_bp_keys.ensure_grow(std::max<u64>(M, 1) * 4 * 2));
	HIPCHK(c, c->d_bp_vals.ensure_grow(std::max<u64>(M, 1) * 4 * 2));
	HIPCHK(c, c->d_aln_post.ensure_grow(cells * 4));
	RunBufs rb;
	if (prepare_runs(c, M, cells, &rb)) return 1;
	u32 *keys_in = c->d_bp_keys.as<u32>(), *keys_out = keys_in + std::max<u64>(M, 1);
	float *vals_in = c->d_bp_vals.as<float>(), *vals_out = vals_in + std::max<u64>(M, 1);
	const char *din = c->d_bp_in.as<char>();
	BuildPostParams bp;
	fill_store_params(c, bp.s);
	bp.seq1 = (const u32 *)(din + o_seqs); bp.seq2 = bp.seq1 + n1; bp.n1 = n1; bp.n2 = n2;
	bp.p2c1 = (const u32 *)(din + o_maps); bp.p2c2 = bp.p2c1; // offsets below are into the one concatenated array
	bp.p2c1_off = (const u64 *)(din + o_off); bp.p2c2_off = bp.p2c1_off + n1;
	bp.C2 = C2; bp.coff = (const u64 *)(din + o_coff); bp.keys = keys_in; bp.vals = vals_in;
	bp.w1 = weighted ? (const float *)(din + o_w) : nullptr; bp.w2 = weighted ? bp.w1 + n1 : nullptr;
	bp.post = c->d_aln_post.as<float>(); bp.cells = cells; bp.counters = rb.counters;
	TimedSpan ts_bp;
	if (span_begin(c, 5, &ts_bp)) return 1;
	MPC_LAUNCH(build_post_gen_kernel, (u32)std::min<u64>(npairs12, (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, bp);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts_bp)) return 1;
	const u32 *keys_sorted = keys_in;
	const float *vals_sorted = vals_in;
	if (span_begin(c, 6, &ts_bp)) return 1;
	if (M > 1) {
		HIPCHK(c, mpc_sort_pairs([&](size_t bytes) -> void * { return c->d_bp_tmp.ensure_grow(bytes) == hipSuccess ? c->d_bp_tmp.p : nullptr; },
			keys_in, keys_out, vals_in, vals_out, (size_t)M, bc, c->stream));
		keys_sorted = keys_out;
		vals_sorted = vals_out;
	}
	if (span_end(c, &ts_bp)) return 1;
	if (span_begin(c, 7, &ts_bp)) return 1;
	if (reduce_runs(c, rb, keys_sorted, vals_sorted, M, cells)) return 1;
	if (span_end(c, &ts_bp)) return 1;
	lap(2);
	c->last_post_cells = cells;
	if (!path) { // matrix only (mpcgpu_build_post); the staging record is reused by the next call: drain the stream
		HIPCHK(c, hipStreamSynchronize(c->stream));
		return 0;
	}
	// the staging record is reused by the next call: run_calc_aln ends with a wait for the stream
	const int rc_aln = run_calc_aln(c, c->d_aln_post.as<float>(), C1, C2, path, pathlen, score);
	lap(3);
	if (host_trace && (++acc_n % 100) == 0)
		fprintf(stderr, "[mpcgpu] align_alns host seconds after %llu calls: vectors %.3f, uploads %.3f, launches %.3f, calc_aln+syncs %.3f\n",
			(unsigned long long)acc_n, acc_t[0], acc_t[1], acc_t[2], acc_t[3]);
	return rc_aln;
}

int mpcgpu_align_alns_w(mpcgpu_ctx *c, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2, uint32_t C1,
	uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, const float *w1, const float *w2, char *path,
	uint32_t *pathlen, float *score)
{
	if (!c) return 1;
	if (!path || !pathlen) return fail(c, "mpcgpu_align_alns: NULL argument");
	return build_post_impl(c, "mpcgpu_align_alns", n1, seq1, n2, seq2, C1, C2, pos2col1, pos2col2, w1, w2, path, pathlen, score);
}

// calc_aln_wave_batch_kernel, a workgroup of one wave per AlnParams record; lds_rows: the longest LX + 1 among them
static int launch_aln_wave_batch(mpcgpu_ctx *c, const AlnParams *ap, u32 n, u32 lds_rows)
{
	const size_t smem = (size_t)lds_rows * MPC_ALNW_ROWBYTES + 16;
	if (smem > c->aln_smem_set[3]) {
		(void)hipFuncSetAttribute((const void *)calc_aln_wave_batch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
		c->aln_smem_set[3] = smem;
	}
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
// forms (the few near the root) is aligned by mpcgpu_align_alns, in list order. Same matrices, same paths: the per-join work is the
// single-join kernels' body.
int mpcgpu_align_alns_batch(mpcgpu_ctx *c, uint32_t njoins, const uint32_t *n1, const uint32_t *n2, const uint32_t *C1, const uint32_t *C2,
	const uint32_t *seqs, const uint32_t *pos2col, uint32_t path_stride, char *paths, uint32_t *pathlens, float *scores)
{
	if (!c) return 1;
	if (!c->have_store) return fail(c, "mpcgpu_align_alns_batch: no store (call mpcgpu_build_store / mpcgpu_store_import)");
	if (njoins && (!n1 || !n2 || !C1 || !C2 || !seqs || !pos2col || !paths || !pathlens)) return fail(c, "mpcgpu_align_alns_batch: NULL argument");
	if ((c->partial || c->packed_stale) && mpcgpu_store_complete(c)) return 1;
	HIPCHK(c, hipSetDevice(c->device));
	const u32 n = c->n;
	// where each join's rows and maps start in the caller's arrays; which joins take the batched forms
	std::vector<u64> soff(njoins + 1, 0), moff(njoins + 1, 0);
	std::vector<u32> small;
	for (u32 j = 0; j < njoins; ++j) {
		if (n1[j] == 0 || n2[j] == 0 || C1[j] == 0 || C2[j] == 0) return fail(c, "mpcgpu_align_alns_batch: join %u is empty", j);
		if ((u64)C1[j] + C2[j] > path_stride) return fail(c, "mpcgpu_align_alns_batch: path_stride %u too small for join %u", path_stride, j);
		u64 len = 0;
		for (u32 a = 0; a < n1[j] + n2[j]; ++a) {
			const u32 S = seqs[soff[j] + a];
			if (S >= n) return fail(c, "mpcgpu_align_alns_batch: sequence index %u out of range", S);
			len += c->len[S];
		}
		soff[j + 1] = soff[j] + n1[j] + n2[j];
		moff[j + 1] = moff[j] + len;
		const bool rows_ok = c->have_pad && (u64)n1[j] * n2[j] <= 2048 && C2[j] <= 1024u && (u64)n1[j] * C1[j] <= (1u << 22);
		const bool wave_ok = (u64)C2[j] + 1 <= MPC_ALNW_MAXW && (size_t)(C1[j] + 1) * MPC_ALNW_ROWBYTES + 16 <= 160u * 1024u;
		if (rows_ok && wave_ok && njoins > 1) small.push_back(j);
	}
	std::vector<unsigned char> done(njoins, 0);
	// ---- the small joins, in chunks whose matrices fit a budget of device memory
	for (size_t s0 = 0; s0 < small.size();) {
		size_t s1 = s0;
		u64 cells = 0, tbb = 0, revb = 0, inb = 0, nrows = 0, resb = 0;
		u32 lds_rows = 0;
		while (s1 < small.size()) {
			const u32 j = small[s1];
			const u64 cj = (u64)C1[j] * C2[j];
			if (s1 > s0 && (cells + cj) * 4 > ((u64)1 << 30)) break;
			u64 len2 = 0;
			for (u32 b = 0; b < n2[j]; ++b) len2 += c->len[seqs[soff[j] + n1[j] + b]];
			cells += cj; tbb += ((u64)C1[j] + 1) * ((u64)C2[j] + 1); revb += (u64)C1[j] + C2[j]; nrows += C1[j];
			resb += (8 + (u64)C1[j] + C2[j] + 7) & ~7ull;
			inb += 4 * ((u64)n1[j] + n2[j] + (u64)n1[j] * C1[j] + n2[j] + 1 + len2);
			lds_rows = std::max(lds_rows, C1[j] + 1);
			++s1;
		}
		const u32 nb = (u32)(s1 - s0);
		// one page-locked record, copied to the device once: [rows table][BuildPost parameters][alignment parameters][the joins' inputs]
		const u64 o_rows = 0, o_bp = (o_rows + 8 * nrows + 15) & ~15ull, o_ap = (o_bp + (u64)nb * sizeof(BuildPostRowsParams) + 15) & ~15ull,
			o_in = (o_ap + (u64)nb * sizeof(AlnParams) + 15) & ~15ull, o_err = o_in + inb, total = o_err + 16;
		HIPCHK(c, c->h_bp_in.ensure(total));
		HIPCHK(c, c->d_bp_in.ensure_grow(total));
		HIPCHK(c, c->d_aln_post.ensure_grow(cells * 4));
		HIPCHK(c, c->d_aln_tb.ensure_grow(tbb));
		HIPCHK(c, c->d_aln_rev.ensure_grow(revb));
		HIPCHK(c, c->h_aln_res.ensure(resb));
		char *hin = c->h_bp_in.as<char>();
		const char *din = c->d_bp_in.as<char>();
		u32 *rows = (u32 *)(hin + o_rows);
		BuildPostRowsParams *bp = (BuildPostRowsParams *)(hin + o_bp);
		AlnParams *ap = (AlnParams *)(hin + o_ap);
		u64 at_in = o_in, at_row = 0, at_cell = 0, at_tb = 0, at_rev = 0, at_res = 0;
		bool any16 = false, any8 = false;
		for (u32 q = 0; q < nb; ++q) {
			const u32 j = small[s0 + q];
			const u32 *sj = seqs + soff[j], *mj = pos2col + moff[j];
			u32 *h_seqs = (u32 *)(hin + at_in);
			const u64 d_seqs = at_in;
			memcpy(h_seqs, sj, 4 * ((size_t)n1[j] + n2[j]));
			at_in += 4 * ((u64)n1[j] + n2[j]);
			u32 *c2p = (u32 *)(hin + at_in);
			const u64 d_c2p = at_in;
			at_in += 4 * (u64)n1[j] * C1[j];
			for (u64 e = 0; e < (u64)n1[j] * C1[j]; ++e) c2p[e] = MPC_BPR_GAP;
			u64 m = 0;
			for (u32 a = 0; a < n1[j]; ++a) {
				const u32 L = c->len[sj[a]];
				for (u32 pos = 0; pos < L; ++pos) {
					const u32 col = mj[m + pos];
					if (col >= C1[j]) return fail(c, "mpcgpu_align_alns_batch: column map of MSA1 out of range (join %u)", j);
					if (pos && col <= mj[m + pos - 1]) return fail(c, "mpcgpu_align_alns_batch: column map of MSA1 row %u is not strictly increasing at position %u (join %u)", a, pos, j);
					c2p[(u64)a * C1[j] + col] = pos;
				}
				m += L;
			}
			u32 *off2 = (u32 *)(hin + at_in);
			const u64 d_off2 = at_in;
			at_in += 4 * ((u64)n2[j] + 1);
			off2[0] = 0;
			for (u32 b = 0; b < n2[j]; ++b) off2[b + 1] = off2[b] + c->len[sj[n1[j] + b]];
			u32 *maps2 = (u32 *)(hin + at_in);
			const u64 d_maps2 = at_in;
			memcpy(maps2, mj + m, 4 * (size_t)off2[n2[j]]);
			at_in += 4 * (u64)off2[n2[j]];
			for (u32 b = 0; b < n2[j]; ++b)
				for (u32 e = off2[b]; e < off2[b + 1]; ++e) {
					if (maps2[e] >= C2[j]) return fail(c, "mpcgpu_align_alns_batch: column map of MSA2 out of range (join %u)", j);
					if (e > off2[b] && maps2[e] <= maps2[e - 1])
						return fail(c, "mpcgpu_align_alns_batch: column map of MSA2 row %u is not strictly increasing at position %u (join %u)", b, e - off2[b], j);
				}
			for (u32 a = 0; a < n1[j]; ++a)
				for (u32 b = 0; b < n2[j]; ++b) if (sj[a] == sj[n1[j] + b]) return fail(c, "mpcgpu_align_alns_batch: sequence %u is in both alignments of join %u", sj[a], j);
			BuildPostRowsParams &r = bp[q];
			fill_store_params(c, r.s);
			r.seq1 = (const u32 *)(din + d_seqs); r.seq2 = r.seq1 + n1[j]; r.n1 = n1[j]; r.n2 = n2[j];
			r.c2p1 = (const u32 *)(din + d_c2p); r.p2c2 = (const u32 *)(din + d_maps2); r.off2 = (const u32 *)(din + d_off2);
			r.C1 = C1[j]; r.C2 = C2[j]; r.w1 = nullptr; r.w2 = nullptr;
			r.post = c->d_aln_post.as<float>() + at_cell; r.err = (u32 *)(din + o_err);
			AlnParams &a = ap[q];
			a.post = r.post; a.LX = C1[j]; a.LY = C2[j];
			a.tb = c->d_aln_tb.as<char>() + at_tb; a.rev = c->d_aln_rev.as<char>() + at_rev;
			a.pathlen = (u32 *)(c->h_aln_res.as<char>() + at_res); a.score = (float *)(c->h_aln_res.as<char>() + at_res + 4); a.path = c->h_aln_res.as<char>() + at_res + 8;
			for (u32 col = 0; col < C1[j]; ++col) { rows[2 * (at_row + col)] = q; rows[2 * (at_row + col) + 1] = col; }
			at_row += C1[j]; at_cell += (u64)C1[j] * C2[j]; at_tb += ((u64)C1[j] + 1) * ((u64)C2[j] + 1); at_rev += (u64)C1[j] + C2[j];
			at_res += (8 + (u64)C1[j] + C2[j] + 7) & ~7ull;
			(C2[j] > 512u ? any16 : any8) = true;
		}
		memset(hin + o_err, 0, 16);
		HIPCHK(c, hipMemcpyAsync(c->d_bp_in.p, hin, total, hipMemcpyHostToDevice, c->stream));
		const u32 grid = (u32)std::min<u64>(nrows, (u64)c->prop.multiProcessorCount * 32u);
		TimedSpan ts;
		if (span_begin(c, 5, &ts)) return 1;
		if (any8) MPC_LAUNCH(build_post_rows_batch_kernel<8>, grid, 64, 8 * MPC_BPR_CAP, c->stream, (const BuildPostRowsParams *)(din + o_bp), (const u32 *)(din + o_rows), (u32)nrows);
		if (any16) MPC_LAUNCH(build_post_rows_batch_kernel<16>, grid, 64, 8 * MPC_BPR_CAP, c->stream, (const BuildPostRowsParams *)(din + o_bp), (const u32 *)(din + o_rows), (u32)nrows);
		HIPCHK(c, hipGetLastError());
		if (span_end(c, &ts)) return 1;
		if (launch_aln_wave_batch(c, (const AlnParams *)(din + o_ap), nb, lds_rows)) return 1;
		u32 err = 0;
		HIPCHK(c, hipMemcpyAsync(&err, din + o_err, 4, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		if (!err) { // (a list overflow of the row form — very wide posterior rows — leaves the chunk to the single-join path below)
			u64 r_at = 0;
			for (u32 q = 0; q < nb; ++q) {
				const u32 j = small[s0 + q];
				const char *res = c->h_aln_res.as<char>() + r_at;
				u32 np;
				memcpy(&np, res, 4);
				if (np > C1[j] + C2[j]) return fail(c, "mpcgpu_align_alns_batch: path length %u out of range (internal error)", np);
				pathlens[j] = np;
				if (scores) memcpy(&scores[j], res + 4, 4);
				memcpy(paths + (u64)j * path_stride, res + 8, np);
				done[j] = 1;
				r_at += (8 + (u64)C1[j] + C2[j] + 7) & ~7ull;
			}
		}
		c->last_post_cells = 0;
		s0 = s1;
	}
	// ---- the others, one after the other
	for (u32 j = 0; j < njoins; ++j) {
		if (done[j]) continue;
		const u32 *sj = seqs + soff[j], *mj = pos2col + moff[j];
		u64 len1 = 0;
		for (u32 a = 0; a < n1[j]; ++a) len1 += c->len[sj[a]];
		if (build_post_impl(c, "mpcgpu_align_alns_batch", n1[j], sj, n2[j], sj + n1[j], C1[j], C2[j], mj, mj + len1, nullptr, nullptr, paths + (u64)j * path_stride, &pathlens[j],
			scores ? &scores[j] : nullptr)) return 1;
	}
	return 0;
}

int mpcgpu_build_post(mpcgpu_ctx *c, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2, uint32_t C1,
	uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, const float *w1, const float *w2, float *post)
{
	if (!c) return 1;
	if (!post) return fail(c, "mpcgpu_build_post: NULL argument");
	if (build_post_impl(c, "mpcgpu_build_post", n1, seq1, n2, seq2, C1, C2, pos2col1, pos2col2, w1, w2, nullptr, nullptr, nullptr)) return 1;
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
	// (a row's map must rise strictly, as in build_post_impl)
	for (u32 q = 0; q < npairs; ++q) {
		for (u64 x = off1[q]; x < off1[q + 1]; ++x) {
			if (pos2col1[x] >= C1) return fail(c, "mpcgpu_align_msas: column map of MSA1 out of range");
			if (x > off1[q] && pos2col1[x] <= pos2col1[x - 1]) return fail(c, "mpcgpu_align_msas: column map of MSA1 in pair %u is not strictly increasing at position %u", q, (u32)(x - off1[q]));
		}
		for (u64 x = off2[q]; x < off2[q + 1]; ++x) {
			if (pos2col2[x] >= C2) return fail(c, "mpcgpu_align_msas: column map of MSA2 out of range");
			if (x > off2[q] && pos2col2[x] <= pos2col2[x - 1]) return fail(c, "mpcgpu_align_msas: column map of MSA2 in pair %u is not strictly increasing at position %u", q, (u32)(x - off2[q]));
		}
	}
	const u64 M = coff[npairs];
	const u64 cells = (u64)C1 * C2;
	if (cells > 0xffffffffull) return fail(c, "mpcgpu_align_msas: %llu cells exceed this build's cell index", (u64)cells);
	const u32 bc = bits_for(cells - 1);
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
	u32 *keys_in = c->d_bp_keys.as<u32>(), *keys_out = keys_in + std::max<u64>(M, 1);
	float *vals_in = c->d_bp_vals.as<float>(), *vals_out = vals_in + std::max<u64>(M, 1);
	BuildPostListParams lp;
	lp.seq_len = c->d_seq_len.as<u32>();
	lp.packed = c->d_shard.as<u32>();
	lp.seq1 = c->d_bp_seq.as<u32>(); lp.seq2 = lp.seq1 + npairs; lp.npairs = npairs;
	lp.p2c1 = c->d_bp_map.as<u32>(); lp.p2c2 = lp.p2c1 + off1[npairs];
	lp.off1 = c->d_bp_off.as<u64>(); lp.off2 = lp.off1 + (npairs + 1);
	lp.coff = c->d_bp_coff.as<u64>(); lp.rbase = lp.coff + (npairs + 1);
	lp.nnz = nullptr; // counts come from coff
	lp.C2 = C2; lp.keys = keys_in; lp.vals = vals_in;
	lp.post = c->d_aln_post.as<float>(); lp.cells = cells; lp.counters = rb.counters;
	MPC_LAUNCH(build_post_list_gen_kernel, (u32)std::min<u64>(npairs, (u64)c->prop.multiProcessorCount * 32), 64, 0, c->stream, lp);
	HIPCHK(c, hipGetLastError());
	const u32 *keys_sorted = keys_in;
	const float *vals_sorted = vals_in;
	if (M > 1) {
		HIPCHK(c, mpc_sort_pairs([&](size_t bytes) -> void * { return c->d_bp_tmp.ensure_grow(bytes) == hipSuccess ? c->d_bp_tmp.p : nullptr; },
			keys_in, keys_out, vals_in, vals_out, (size_t)M, bc, c->stream));
		keys_sorted = keys_out;
		vals_sorted = vals_out;
	}
	if (reduce_runs(c, rb, keys_sorted, vals_sorted, M, cells)) return 1;
	c->last_post_cells = cells;
	return run_calc_aln(c, c->d_aln_post.as<float>(), C1, C2, path, pathlen, score); // syncs before the vectors above die
}

// The one-wave alignments of n pairs (sx[q], sy[q]), their dense matrices at off[q] of c->d_aln_post, in ONE launch: parameters in (ap) and a
// record {length, score, path} per pair out (res, aln_rec_stride() apart) through page-locked memory that the device addresses; one wait.
// ovf: candidate-overflow flags that the same wait brings back (the short list; else NULL): one of them set = 2, nothing handed out.
static u64 aln_rec_stride(u32 Lsum_max) { return ((u64)8 + Lsum_max + 7) & ~7ull; }
static int align_wave_batch(mpcgpu_ctx *c, u32 n, const u32 *sx, const u32 *sy, const u64 *off, u32 LXmax, u32 Lsum_max, AlnParams *ap, char *res, const u32 *ovf, u32 path_stride, char *paths, u32 *pathlens, float *scores, float *ea)
{
	const u64 rstride = aln_rec_stride(Lsum_max);
	for (u32 q = 0; q < n; ++q) {
		char *r = res + (u64)q * rstride;
		ap[q].post = c->d_aln_post.as<float>() + off[q];
		ap[q].LX = c->len[sx[q]]; ap[q].LY = c->len[sy[q]];
		ap[q].tb = nullptr; ap[q].rev = c->d_aln_rev.as<char>() + (u64)q * Lsum_max;
		ap[q].pathlen = (u32 *)r; ap[q].score = (float *)(r + 4); ap[q].path = r + 8;
	}
	if (launch_aln_wave_batch(c, ap, n, LXmax + 1)) return 1;
	HIPCHK(c, hipStreamSynchronize(c->stream)); // the one wait
	for (u32 q = 0; ovf && q < n; ++q) if (ovf[q] & 1u) return 2;
	for (u32 q = 0; q < n; ++q) {
		const char *r = res + (u64)q * rstride;
		u32 n_path;
		memcpy(&n_path, r, 4);
		if (n_path > ap[q].LX + ap[q].LY) return fail(c, "mpcgpu_align_pairs: path length %u out of range (internal error)", n_path);
		pathlens[q] = n_path;
		float sc;
		memcpy(&sc, r + 4, 4);
		if (scores) scores[q] = sc;
		if (ea) ea[q] = sc / (float)std::min(ap[q].LX, ap[q].LY); // alignpairflat.cpp:18 (uint -> float, IEEE divide)
		memcpy(paths + (u64)q * path_stride, r + 8, n_path);
	}
	return 0;
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
	if (g.LXlong) return 2; // row-block pairs: general path
	u32 Lsum_max = 0;
	for (u32 q = 0; q < np; ++q) {
		const u32 LX = c->len[px[q]], LY = c->len[py[q]];
		if ((u64)LY + 1 > MPC_ALNW_MAXW || (size_t)(LX + 1) * MPC_ALNW_ROWBYTES + 16 > 160u * 1024u) return 2; // not a one-wave alignment
		Lsum_max = std::max(Lsum_max, LX + LY);
	}
	if (!post_rows_fits(g.LXmax, g.LYmax, 1024)) return 2;
	c->have_shard = c->have_store = false;
	c->shard_is_list = true;
	c->list_x.assign(px, px + np); c->list_y.assign(py, py + np);
	c->list_q0 = 0; c->ap_x.clear(); c->ap_y.clear();
	c->sh_k0 = 0; c->sh_k1 = np;
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
	u32 hcount[MPC_HMAX + 1] = {0};
	std::vector<u32> keys(np);
	for (u32 q = 0; q < np; ++q) { const u32 H = (c->len[px[q]] + 63) / 64; hcount[H]++; keys[q] = (H << 16) | q; }
	std::sort(keys.begin(), keys.end());
	for (u32 q = 0; q < np; ++q) order[q] = keys[q] & 0xffffu;
	// ---- scratch
	if (ensure_pair_scratch(c, g, np)) return 1;
	HIPCHK(c, c->d_aln_post.ensure_grow(off[np] * 4));
	HIPCHK(c, c->d_aln_rev.ensure_grow((u64)np * Lsum_max + 16));
	// ---- forward / backward, one launch per rows-per-lane bin
	FbParams fp;
	fill_fb_params(c, fp, bx, by, g.capc, g.mega);
	if (launch_fb_bins(c, g, fp, order, hcount, 0)) return 1;
	// ---- probabilities, EA, sparsify (the candidate lists keep the probabilities): a workgroup per pair, the knobs of the general stage ignored
	const PostIO io = {bx, by, c->d_seq_len.as<u32>(), c->d_cand.as<u64>(), c->d_cand_cnt.as<u32>(), c->d_res.as<u32>(), (u32 *)(h + o_nnz), (float *)(h + o_ea), (u32 *)(h + o_flags), np};
	if (launch_post_rows(c, g, io, 1024, 64, np, c->d_sort_scratch, true)) return 1;
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

struct KeepList { mpcgpu_ctx *c; ~KeepList() { c->ap_keep = false; } }; // c->ap_keep (set by the owner) is dropped on every way out
// AlignPairFlat (alignpairflat.cpp:3-27) for a list of pairs: CalcPost (fwd + bwd + CalcPostFlat, calcpost.cpp:4-36) -> CalcAlnFlat on
// the DENSE thresholded posterior -> path; EA = Score / min(L1, L2). Stage A runs on the list (the kernels of
// mpcgpu_calc_posteriors), the dense matrices are rebuilt from the candidate lists (every cell with Score >= MIN_SPARSE_SCORE, also
// those FromPost drops), the alignments run one wavefront each in ONE launch when they fit (else one after the other).
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
	if (npairs >= 1 && npairs <= 64 && env_int("MPCGPU_PAIRS_SMALL", 1)) {
		const int rc = align_pairs_small(c, npairs, seq1, seq2, path_stride, paths, pathlens, scores, ea);
		if (rc != 2) return rc;
	}
	u32 chunk = 256; // pairs per stage-A call: their dense matrices (LX*LY floats each) live together
	KeepList keep_guard{c};
	c->ap_keep = true;
	c->ap_x.assign(seq1, seq1 + npairs); c->ap_y.assign(seq2, seq2 + npairs);
	for (u32 q0 = 0; q0 < npairs;) {
		u32 nq = std::min<u32>(chunk, npairs - q0);
		// the chunk's dense matrices live together in d_aln_post: a chunk whose matrices do not fit half of what is free (long pairs: 1.6 GB
		// for 20 000 x 20 000) is halved like one that stage A has to split, down to a single pair
		{
			size_t freeb = 0, totb = 0;
			HIPCHK(c, hipMemGetInfo(&freeb, &totb));
			const u64 room = (u64)((freeb + c->d_aln_post.cap) * 0.5);
			auto bytes_of = [&](u32 k) { u64 b = 0; for (u32 q = 0; q < k; ++q) b += (u64)c->len[seq1[q0 + q]] * c->len[seq2[q0 + q]] * 4; return b; };
			while (nq > 1 && bytes_of(nq) > room) { nq = (nq + 1) / 2; chunk = nq; }
		}
		// the dense matrices below are rebuilt from the candidate lists ONE stage-A batch leaves behind: a chunk that stage A had to
		// cut into several batches (long sequences, little free memory) is halved and run again, down to a single pair
		for (;;) {
			if (stage_a(c, nq, seq1 + q0, seq2 + q0)) return 1;
			c->list_q0 = q0; // what the last stage holds is pairs [q0, q0 + nq) of the caller's list
			if (c->sa_b0 == 0 && c->sa_B == nq) break;
			if (nq == 1) return fail(c, "mpcgpu_align_pairs: pair %u (%u x %u residues) does not fit one stage-A batch", q0, c->len[seq1[q0]], c->len[seq2[q0]]);
			nq = (nq + 1) / 2;
			chunk = nq;
		}
		// Without the row-list finishing kernel the candidate lists still hold the scores (post_kernel sorts a copy): the raw builder forms
		// the probabilities itself. Only a list that does not FIT the row-list kernel goes that way; MPCGPU_POST=sort stays a refusal.
		const char *post_mode = getenv("MPCGPU_POST");
		if (!c->sa_post_rows && post_mode && !strcmp(post_mode, "sort"))
			return fail(c, "mpcgpu_align_pairs: pair list with a sequence of more than ~12 000 residues (or MPCGPU_POST=sort): the row-list finishing kernel "
				"whose candidate lists this entry point rebuilds the dense posteriors from does not take them");
		// dense matrices
		std::vector<u64> off(nq + 1, 0);
		u32 Lsum_max = 0, LXmax = 0;
		bool all_wave = true;
		for (u32 q = 0; q < nq; ++q) {
			const u32 LX = c->len[seq1[q0 + q]], LY = c->len[seq2[q0 + q]];
			off[q + 1] = off[q] + (u64)LX * LY;
			Lsum_max = std::max(Lsum_max, LX + LY);
			LXmax = std::max(LXmax, LX);
			all_wave = all_wave && (u64)LY + 1 <= MPC_ALNW_MAXW && (size_t)(LX + 1) * MPC_ALNW_ROWBYTES + 16 <= 160u * 1024u;
		}
		HIPCHK(c, c->d_aln_post.ensure_grow(off[nq] * 4));
		if (upload(c, c->d_ap_off, off)) return 1;
		DensePostParams dp;
		dp.pair_x = c->d_bx.as<u32>(); dp.pair_y = c->d_by.as<u32>(); dp.seq_len = c->d_seq_len.as<u32>();
		dp.cand = c->d_cand.as<u64>(); dp.capc = c->sa_capc; dp.cand_cnt = c->d_cand_cnt.as<u32>(); dp.long_min = c->sa_long_min;
		dp.out_off = c->d_ap_off.as<u64>(); dp.out = c->d_aln_post.as<float>();
		if (c->sa_post_rows) MPC_LAUNCH(dense_post_kernel, nq, 256, 0, c->stream, dp);
		else {
			// zeroes by one memset on the stream, the scatter on (pairs) x (slabs of 256 candidates, as many as keep the chip busy)
			DensePostRawParams rp;
			rp.d = dp; rp.use_fma = c->use_fma;
			rp.slabs = (u32)std::max<u64>(1, std::min<u64>(((u64)c->sa_capc + 255) / 256, ((u64)c->prop.multiProcessorCount * 8 + nq - 1) / nq));
			if (trace_on()) { fprintf(stderr, "[mpcgpu] align_pairs dense posteriors from raw candidates: %u pairs x %u slabs, %.1f MB\n", nq, rp.slabs, (double)off[nq] * 4 / 1048576.0); fflush(stderr); }
			TimedSpan ts_dense;
			if (span_begin(c, 5, &ts_dense)) return 1;
			HIPCHK(c, hipMemsetAsync(c->d_aln_post.p, 0, off[nq] * 4, c->stream));
			MPC_LAUNCH(dense_post_raw_kernel, nq * rp.slabs, 256, 0, c->stream, rp);
			HIPCHK(c, hipGetLastError());
			if (span_end(c, &ts_dense)) return 1;
		}
		HIPCHK(c, hipGetLastError());
		c->last_post_cells = 0; // several matrices: not what mpcgpu_get_last_post hands out
		if (all_wave) {
			// one launch: parameters in, {length, score, path} out through page-locked memory
			HIPCHK(c, c->h_ap.ensure((u64)nq * (sizeof(AlnParams) + aln_rec_stride(Lsum_max))));
			HIPCHK(c, c->d_aln_rev.ensure_grow((u64)nq * Lsum_max + 16));
			AlnParams *ap = c->h_ap.as<AlnParams>();
			if (align_wave_batch(c, nq, seq1 + q0, seq2 + q0, off.data(), LXmax, Lsum_max, ap, (char *)(ap + nq), nullptr, path_stride, paths + (u64)q0 * path_stride, pathlens + q0, scores ? scores + q0 : nullptr, ea ? ea + q0 : nullptr)) return 1;
		} else {
			for (u32 q = 0; q < nq; ++q) {
				const u32 LX = c->len[seq1[q0 + q]], LY = c->len[seq2[q0 + q]];
				float sc = 0;
				if (run_calc_aln(c, c->d_aln_post.as<float>() + off[q], LX, LY, paths + (u64)(q0 + q) * path_stride, &pathlens[q0 + q], &sc)) return 1;
				if (scores) scores[q0 + q] = sc;
				if (ea) ea[q0 + q] = sc / (float)std::min(LX, LY);
			}
		}
		q0 += nq;
	}
	return 0;
}

int mpcgpu_get_list_sparse(mpcgpu_ctx *c, uint32_t q, uint32_t *nnz, uint32_t *offsets, void *values)
{
	if (!c) return 1;
	if (!c->shard_is_list) return fail(c, "mpcgpu_get_list_sparse: no list stage holds pair %u", q);
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


// mpcgpu_ea.inc — host side of post_ea_kernel (kernels_postea.h) and post_wide_ea_kernel (kernels_postwea.h): mpcgpu_ea_scores,
// mpcgpu_ea_info, mpcgpu_ea_wide_info. Included by mpcgpu.cpp inside its
// extern "C" block, behind mpcgpu_stage_a.inc, whose dispatcher it drives: the forward/backward sweeps are stage A's (chains, fb_kernel, row
// blocks, structure profiles), batch by batch under the same MPCGPU_SCRATCH_GB, and only the finish differs — one float per pair, no
// records, no pack, no shard. What the call uses of the context is stage A's SCRATCH (candidate lists, planes, index arrays: nothing a
// later call reads) and buffers of its own (mpcgpu_ctx::ea); shard, store, committed values, the results and counters of the last stage A
// and the store epoch stay as they are.

extern "C++" {
namespace {

// post_ea_kernel over the B pairs of the current batch (index arrays c->d_bx / c->d_by): a persistent grid, as launch_post_rows sizes it
int launch_post_ea(mpcgpu_ctx *c, const StageAGeom &g, u32 sort_cap, u32 batch, u64 B)
{
	mpcgpu_ctx::EaState &e = c->ea;
	PostEaParams pe;
	pe.pair_x = c->d_bx.as<u32>(); pe.pair_y = c->d_by.as<u32>(); pe.seq_len = c->d_seq_len.as<u32>();
	pe.cand = c->d_cand.as<u64>(); pe.capc = g.capc; pe.cand_cnt = c->d_cand_cnt.as<u32>();
	pe.use_fma = c->use_fma;
	pe.lx_cap = g.LXmax + 2; pe.ly_cap = g.LYmax + 2;
	pe.sort_cap = std::min<u32>(g.capc, sort_cap); pe.sort_stride = g.capc;
	pe.batch = std::min<u32>(std::max<u32>(batch, 1u), 64u);
	const size_t fixed_lds = post_rows_fixed_lds(g);
	if (fixed_lds + (size_t)pe.sort_cap * 8 > 150 * 1024) pe.sort_cap = (u32)((150 * 1024 - fixed_lds) / 8); // (post_rows_fits: the arrays per position come first)
	const size_t smem = fixed_lds + (size_t)pe.sort_cap * 8;
	ensure_dyn_smem((const void *)post_ea_kernel, smem);
	int pocc = occ_blocks((const void *)post_ea_kernel, 64, smem);
	pocc = std::max(1, std::min(pocc, (int)((152 * 1024) / smem))); // (as for post_rows_kernel: 64-thread workgroups stop fitting at ~152 KB per CU)
	const u32 grid = (u32)std::max<u64>(std::min<u64>(B, (u64)c->prop.multiProcessorCount * (u32)pocc), 1);
	HIPCHK(c, e.d_sort.ensure(g.capc > pe.sort_cap ? (u64)grid * pe.sort_stride * 8 : 8));
	HIPCHK(c, e.d_ea.ensure(B * 4));
	pe.sort_scratch = e.d_sort.as<u64>();
	pe.ea = e.d_ea.as<float>();
	pe.count = (u32)B; pe.long_min = g.long_min;
	if (trace_on()) { fprintf(stderr, "[mpcgpu] post ea: %llu pairs, list of %u candidates in LDS, lds=%zu B blocks/CU=%d grid=%u\n", (unsigned long long)B, pe.sort_cap, smem, pocc, grid); fflush(stderr); }
	TimedSpan sp;
	if (span_begin(c, 1, &sp)) return 1;
	MPC_LAUNCH(post_ea_kernel, grid, 64, smem, c->stream, pe);
	HIPCHK(c, hipGetLastError());
	e.launches += 1;
	return span_end(c, &sp);
}

// post_wide_ea_kernel over the B pairs of the current batch: a workgroup of MPC_POSTW_THREADS per pair on a persistent grid, LDS and the
// slots per workgroup sized as launch_post_wide sizes them (two key slots of capc entries for lists beyond the LDS buffers, LXmax + 1 row
// starts, two DP rows of LYmax + 1 floats for pairs wider than the LDS rows, one info word), in buffers of mpcgpu_ctx::ea.
// MPCGPU_POSTW_LDS (tests): as there.
int launch_post_wide_ea(mpcgpu_ctx *c, const StageAGeom &g, u64 B)
{
	mpcgpu_ctx::EaState &e = c->ea;
	const u32 T = MPC_POSTW_THREADS;
	const int lds_env = env_int("MPCGPU_POSTW_LDS", -1);
	PostWideEaParams pw;
	pw.pair_x = c->d_bx.as<u32>(); pw.pair_y = c->d_by.as<u32>(); pw.seq_len = c->d_seq_len.as<u32>();
	pw.cand = c->d_cand.as<u64>(); pw.capc = g.capc; pw.cand_cnt = c->d_cand_cnt.as<u32>();
	pw.use_fma = c->use_fma;
	pw.lds_cap = std::min<u32>(g.capc, lds_env >= 0 ? std::min<u32>((u32)lds_env, 4096u) : 4096u); // (launch_post_wide: 137 KB at the most, one workgroup per CU)
	pw.srow_cap = std::min<u32>(g.LYmax + 1, lds_env >= 0 ? std::min<u32>((u32)lds_env, 4096u) : 4096u);
	const size_t smem = mpc_postw_smem(T, pw.lds_cap, pw.srow_cap);
	const int pocc = std::max(occ_blocks((const void *)post_wide_ea_kernel, T, smem), 1);
	const u32 grid = (u32)std::max<u64>(std::min<u64>(B, (u64)c->prop.multiProcessorCount * (u32)pocc), 1);
	pw.key_stride = g.capc; pw.rs_stride = (u64)g.LXmax + 1; pw.srow_stride = 2 * ((u64)g.LYmax + 1);
	HIPCHK(c, e.d_wkeys.ensure(g.capc > pw.lds_cap ? (u64)grid * 2 * pw.key_stride * 8 : 8));
	HIPCHK(c, e.d_wrs.ensure((u64)grid * pw.rs_stride * 4));
	HIPCHK(c, e.d_wsrow.ensure(g.LYmax + 1 > pw.srow_cap ? (u64)grid * pw.srow_stride * 4 : 8));
	HIPCHK(c, e.d_winfo.ensure((u64)grid * 8));
	HIPCHK(c, e.d_ea.ensure(B * 4));
	pw.key_scratch = e.d_wkeys.as<u64>(); pw.rs_scratch = e.d_wrs.as<u32>(); pw.srow_scratch = e.d_wsrow.as<float>();
	pw.info = e.d_winfo.as<u64>();
	pw.ea = e.d_ea.as<float>();
	pw.count = (u32)B; pw.long_min = g.long_min;
	if (trace_on()) { fprintf(stderr, "[mpcgpu] post wide ea: %llu pairs, %u threads per pair, lists of %u candidates and rows of %u floats in LDS, lds=%zu B grid=%u\n", (unsigned long long)B, T, pw.lds_cap, pw.srow_cap, smem, grid); fflush(stderr); }
	TimedSpan sp;
	if (span_begin(c, 1, &sp)) return 1;
	MPC_LAUNCH(post_wide_ea_kernel, grid, T, smem, c->stream, pw);
	HIPCHK(c, hipGetLastError());
	e.launches += 1; e.wide_launches += 1;
	return span_end(c, &sp);
}

// MPCGPU_EA_WIDE_MIN unset: the smallest m for which two sequences of m positions no longer fit the row-list arrays (12 115 at the default
// sort cap of 1024). post_rows_fits is monotone in both lengths, so the pairs whose longer sequence stays below m fit together whatever
// mix of row and column lengths their list holds.
u32 ea_wide_min_default(u32 sort_cap)
{
	u32 m = 1;
	const size_t fixed = 32 + 8 * (size_t)sort_cap; // post_rows_fits: (3 m + 6) * 4 + 8 + 8 * sort_cap <= 150 KB
	if (fixed < 150 * 1024) m = (u32)((150 * 1024 - fixed) / 12) + 1;
	while (m > 1 && !post_rows_fits(m - 1, m - 1, sort_cap)) --m;
	while (post_rows_fits(m, m, sort_cap)) ++m;
	return m;
}

// One sub-list of mpcgpu_ea_scores (n > 0 pairs px[], py[]; g = stage_a_geom of the sub-list) through stage A's sweeps and its finishing
// kernel — post_ea_kernel, or post_wide_ea_kernel for the wide pairs. Float q of the sub-list goes to ea[where[q]] (where == NULL: ea[q]).
int ea_sublist(mpcgpu_ctx *c, StageAGeom g, u64 n, const u32 *px, const u32 *py, u32 sort_cap, bool wide, const u64 *where, float *ea)
{
	mpcgpu_ctx::EaState &e = c->ea;
	const ScratchBudget budget = scratch_budget();
	ChainPlan chain; // (no fuse_plan: a fused bin would write records)
	if (chain_plan(c, g, budget.planes, chain)) return 1;
	const u32 post_batch = (u32)std::max(env_int("MPCGPU_POST_BATCH", 64), 1);
	// The batches as stage A queues them, without records and pack: fb(0) ea(0) copy(0) | fb(1) ea(1) copy(1) | ... on one stream; the host
	// prepares batch b + 1 and queues its sweeps before it waits for the floats of batch b (an event behind the copy).
	BatchPrep cur, nxt;
	u64 done = 0;
	if (prepare_batch(c, g, chain, budget.batch, n, px, py, 0, cur, false) || launch_fb_batch(c, g, chain, budget.planes, cur, false, false)) return 1;
	while (done < n) {
		const u64 B = cur.B;
		if (wide ? launch_post_wide_ea(c, g, B) : launch_post_ea(c, g, sort_cap, post_batch, B)) return 1;
		HIPCHK(c, e.h_ea.ensure(B * 4));
		HIPCHK(c, hipMemcpyAsync(e.h_ea.p, e.d_ea.p, B * 4, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipEventRecord(e.ev, c->stream));
		nxt.valid = false;
		if (done + B < n && (prepare_batch(c, g, chain, budget.batch, n, px, py, done + B, nxt, false) || launch_fb_batch(c, g, chain, budget.planes, nxt, true, false))) return 1;
		HIPCHK(c, hipEventSynchronize(e.ev));
		const float *got = e.h_ea.as<float>();
		bool overflow = false;
		for (u64 q = 0; q < B; ++q) overflow = overflow || got[q] < 0.0f; // MPC_EA_OVERFLOW
		if (overflow) {
			const u64 room = (u64)g.LXmax * g.LYmax;
			if (g.capc >= room) return fail(c, "mpcgpu_ea_scores: candidate overflow at full capacity (internal error)");
			if (trace_on()) { fprintf(stderr, "[mpcgpu] ea overflow: batch at pair %llu (%llu pairs) redone, capc %u -> %llu\n", (unsigned long long)done, (unsigned long long)B, g.capc, (unsigned long long)std::min<u64>((u64)g.capc * 2, room)); fflush(stderr); }
			g.capc = (u32)std::min<u64>((u64)g.capc * 2, room);
			e.regrowths += 1; e.wide_regrowths += wide ? 1 : 0;
			// this batch again with a larger candidate room: the next batch's sweeps, queued behind it, are drained and dropped
			HIPCHK(c, hipStreamSynchronize(c->stream));
			if (prepare_batch(c, g, chain, budget.batch, n, px, py, done, cur, false) || launch_fb_batch(c, g, chain, budget.planes, cur, false, false)) return 1;
			continue;
		}
		if (where) for (u64 q = 0; q < B; ++q) ea[where[done + q]] = got[q];
		else memcpy(ea + done, got, B * 4);
		done += B;
		e.batches += 1; e.wide_batches += wide ? 1 : 0;
		std::swap(cur, nxt);
		if (cur.valid) { // the next batch's index arrays become the current set
			std::swap(c->d_bx, c->d_bx_n); std::swap(c->d_by, c->d_by_n); std::swap(c->d_order, c->d_order_n);
			std::swap(c->d_chain_first, c->d_chain_first_n); std::swap(c->d_chain_cnt, c->d_chain_cnt_n);
		}
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

} // namespace
} // extern "C++"

int mpcgpu_ea_scores(mpcgpu_ctx *c, uint64_t npairs, const uint32_t *seq1, const uint32_t *seq2, float *ea)
{
	if (!c) return 1;
	mpcgpu_ctx::EaState &e = c->ea;
	// ---- everything that refuses a call comes first: no device work, no state touched
	if (c->n == 0) return fail(c, "mpcgpu_ea_scores: call mpcgpu_set_seqs_registry / mpcgpu_set_seqs first");
	if ((seq1 == nullptr) != (seq2 == nullptr)) return fail(c, "mpcgpu_ea_scores: seq1 and seq2 must both be given or both be NULL");
	const bool all = seq1 == nullptr;
	if (all && npairs != (u64)c->n * (c->n - 1) / 2)
		return fail(c, "mpcgpu_ea_scores: all pairs of %u sequences are %llu pairs, not %llu", c->n, (unsigned long long)((u64)c->n * (c->n - 1) / 2), (unsigned long long)npairs);
	if (npairs && !ea) return fail(c, "mpcgpu_ea_scores: NULL argument");
	if (!all)
		for (u64 q = 0; q < npairs; ++q)
			if (seq1[q] >= c->n || seq2[q] >= c->n) return fail(c, "mpcgpu_ea_scores: sequence index out of range in pair %llu", (unsigned long long)q);
	if (all) { // InitPairs order (mpcflat.cpp:145-155)
		std::vector<u32> vx, vy; // (built aside: a call refused below leaves the last call's lists)
		vx.reserve(npairs); vy.reserve(npairs);
		for (u32 i = 0; i < c->n; ++i)
			for (u32 j = i + 1; j < c->n; ++j) { vx.push_back(i); vy.push_back(j); }
		e.v_x.swap(vx); e.v_y.swap(vy);
	}
	const u32 *px = all ? e.v_x.data() : seq1, *py = all ? e.v_y.data() : seq2;
	// the envelope of mpcgpu_align_pairs: the reference's own test of a dense posterior (calcposteriorflat.cpp:54-61) ...
	for (u64 q = 0; q < npairs; ++q) {
		const u32 LX = c->len[px[q]], LY = c->len[py[q]];
		if (double(LX) * double(LY) * 5 + 100 > double(INT_MAX))
			return fail(c, "mpcgpu_ea_scores: pair %llu is too long for a dense posterior: LX=%u, LY=%u, LX*LY*5 + 100 exceeds INT_MAX = %d", (unsigned long long)q, LX, LY, INT_MAX);
	}
	StageAGeom g = stage_a_geom(c, npairs, px, py);
	// ... what the row-block sweeps ask of the lengths ...
	if (g.LXlong > MPC_KEY_COL_MASK_LONG || g.LYlong > MPC_KEY_COL_MASK_LONG)
		return fail(c, "mpcgpu_ea_scores: a pair of %u x %u positions is beyond this build's limit of %u per sequence once the row sequence is longer than %u",
			g.LXlong, g.LYlong, MPC_KEY_COL_MASK_LONG, g.long_min - 1);
	// ... and the LDS arrays of the row-list finishing code, which the NARROW pairs of the list share. MPCGPU_EA_WIDE=1 (unset = 0 in the library;
	// the drop-in binary sets 1): a pair whose longer sequence has at least MPCGPU_EA_WIDE_MIN positions is WIDE and finishes in
	// post_wide_ea_kernel, which has no such arrays; without it every pair is narrow and a list beyond the arrays is refused.
	const u32 sort_cap = (u32)std::max(env_int("MPCGPU_POST_SORT_CAP", 1024), 2);
	const bool wide_on = env_int("MPCGPU_EA_WIDE", 0) == 1;
	const u32 wide_min = wide_on ? (u32)std::max(env_int("MPCGPU_EA_WIDE_MIN", (int)ea_wide_min_default(sort_cap)), 1) : 0;
	u64 nwide = 0;
	if (wide_on)
		for (u64 q = 0; q < npairs; ++q) nwide += std::max(c->len[px[q]], c->len[py[q]]) >= wide_min ? 1 : 0;
	std::vector<u32> sx, sy; // the narrow pairs, then the wide ones, each in list order; sq: where in the caller's list
	std::vector<u64> sq;
	if (nwide != 0 && nwide != npairs) {
		sx.resize(npairs); sy.resize(npairs); sq.resize(npairs);
		u64 kn = 0, kw = npairs - nwide;
		for (u64 q = 0; q < npairs; ++q) {
			u64 &k = std::max(c->len[px[q]], c->len[py[q]]) >= wide_min ? kw : kn;
			sx[k] = px[q]; sy[k] = py[q]; sq[k] = q; ++k;
		}
		px = sx.data(); py = sy.data();
	}
	const u64 nnarrow = npairs - nwide;
	StageAGeom gn = g, gw = g; // (one sub-list: the geometry of the list)
	if (!sq.empty()) { gn = stage_a_geom(c, nnarrow, px, py); gw = stage_a_geom(c, nwide, px + nnarrow, py + nnarrow); }
	if (nnarrow && !post_rows_fits(gn.LXmax, gn.LYmax, sort_cap))
		return fail(c, "mpcgpu_ea_scores: sequences of %u and %u positions do not fit the LDS arrays of post_ea_kernel (roughly LXmax + 2 * LYmax <= 36 000; "
			"mpcgpu_align_pairs takes such pairs)", gn.LXmax, gn.LYmax);
	e.pairs = npairs; e.batches = e.regrowths = e.launches = 0;
	e.wide_pairs = nwide; e.wide_batches = e.wide_regrowths = e.wide_launches = 0;
	if (npairs == 0) return 0;

	HIPCHK(c, hipSetDevice(c->device));
	if (!e.ev) HIPCHK(c, hipEventCreateWithFlags(&e.ev, hipEventDisableTiming));
	const u64 *where = sq.empty() ? nullptr : sq.data();
	if (nnarrow && ea_sublist(c, gn, nnarrow, px, py, sort_cap, false, where, ea)) return 1;
	if (nwide && ea_sublist(c, gw, nwide, px + nnarrow, py + nnarrow, sort_cap, true, where ? where + nnarrow : nullptr, ea)) return 1;
	return 0;
}

int mpcgpu_ea_info(mpcgpu_ctx *c, uint64_t out[4])
{
	if (!c) return 1;
	if (!out) return fail(c, "mpcgpu_ea_info: NULL argument");
	const mpcgpu_ctx::EaState &e = c->ea;
	out[0] = e.pairs; out[1] = e.batches; out[2] = e.regrowths; out[3] = e.launches;
	return 0;
}

int mpcgpu_ea_wide_info(mpcgpu_ctx *c, uint64_t out[4])
{
	if (!c) return 1;
	if (!out) return fail(c, "mpcgpu_ea_wide_info: NULL argument");
	const mpcgpu_ctx::EaState &e = c->ea;
	out[0] = e.wide_pairs; out[1] = e.wide_batches; out[2] = e.wide_regrowths; out[3] = e.wide_launches;
	return 0;
}

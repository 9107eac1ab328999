// mpcgpu_ea.inc — host side of post_ea_kernel (kernels_postea.h): mpcgpu_ea_scores, mpcgpu_ea_info. Included by mpcgpu.cpp inside its
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
	// ... and the LDS arrays of the row-list finishing code (post_ea_kernel has no other form: kernels_postea.h)
	const u32 sort_cap = (u32)std::max(env_int("MPCGPU_POST_SORT_CAP", 1024), 2);
	if (!post_rows_fits(g.LXmax, g.LYmax, sort_cap))
		return fail(c, "mpcgpu_ea_scores: sequences of %u and %u positions do not fit the LDS arrays of post_ea_kernel (roughly LXmax + 2 * LYmax <= 36 000; "
			"mpcgpu_align_pairs takes such pairs)", g.LXmax, g.LYmax);
	e.pairs = npairs; e.batches = e.regrowths = e.launches = 0;
	if (npairs == 0) return 0;

	HIPCHK(c, hipSetDevice(c->device));
	const ScratchBudget budget = scratch_budget();
	ChainPlan chain; // (no fuse_plan: a fused bin would write records)
	if (chain_plan(c, g, budget.planes, chain)) return 1;
	const u32 post_batch = (u32)std::max(env_int("MPCGPU_POST_BATCH", 64), 1);
	if (!e.ev) HIPCHK(c, hipEventCreateWithFlags(&e.ev, hipEventDisableTiming));
	// The batches as stage A queues them, without records and pack: fb(0) ea(0) copy(0) | fb(1) ea(1) copy(1) | ... on one stream; the host
	// prepares batch b + 1 and queues its sweeps before it waits for the floats of batch b (an event behind the copy).
	BatchPrep cur, nxt;
	u64 done = 0;
	if (prepare_batch(c, g, chain, budget.batch, npairs, px, py, 0, cur, false) || launch_fb_batch(c, g, chain, budget.planes, cur, false, false)) return 1;
	while (done < npairs) {
		const u64 B = cur.B;
		if (launch_post_ea(c, g, sort_cap, post_batch, B)) return 1;
		HIPCHK(c, e.h_ea.ensure(B * 4));
		HIPCHK(c, hipMemcpyAsync(e.h_ea.p, e.d_ea.p, B * 4, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(c, hipEventRecord(e.ev, c->stream));
		nxt.valid = false;
		if (done + B < npairs && (prepare_batch(c, g, chain, budget.batch, npairs, px, py, done + B, nxt, false) || launch_fb_batch(c, g, chain, budget.planes, nxt, true, false))) return 1;
		HIPCHK(c, hipEventSynchronize(e.ev));
		const float *got = e.h_ea.as<float>();
		bool overflow = false;
		for (u64 q = 0; q < B; ++q) overflow = overflow || got[q] < 0.0f; // MPC_EA_OVERFLOW
		if (overflow) {
			const u64 room = (u64)g.LXmax * g.LYmax;
			if (g.capc >= room) return fail(c, "mpcgpu_ea_scores: candidate overflow at full capacity (internal error)");
			if (trace_on()) { fprintf(stderr, "[mpcgpu] ea overflow: batch at pair %llu (%llu pairs) redone, capc %u -> %llu\n", (unsigned long long)done, (unsigned long long)B, g.capc, (unsigned long long)std::min<u64>((u64)g.capc * 2, room)); fflush(stderr); }
			g.capc = (u32)std::min<u64>((u64)g.capc * 2, room);
			e.regrowths += 1;
			// this batch again with a larger candidate room: the next batch's sweeps, queued behind it, are drained and dropped
			HIPCHK(c, hipStreamSynchronize(c->stream));
			if (prepare_batch(c, g, chain, budget.batch, npairs, px, py, done, cur, false) || launch_fb_batch(c, g, chain, budget.planes, cur, false, false)) return 1;
			continue;
		}
		memcpy(ea + done, got, B * 4);
		done += B;
		e.batches += 1;
		std::swap(cur, nxt);
		if (cur.valid) { // the next batch's index arrays become the current set
			std::swap(c->d_bx, c->d_bx_n); std::swap(c->d_by, c->d_by_n); std::swap(c->d_order, c->d_order_n);
			std::swap(c->d_chain_first, c->d_chain_first_n); std::swap(c->d_chain_cnt, c->d_chain_cnt_n);
		}
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
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

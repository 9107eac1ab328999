// mpcgpu_search.inc — mpcgpu_search_pairs, mpcgpu_search_info: the loop of UClust::Search (uclust.cpp:44-54) for a list of queries in one
// call. Included by mpcgpu.cpp inside its extern "C" block, behind mpcgpu_joins.inc (whose short-list path and general path it follows).
//
// A GROUP is a query's candidate pairs in the order they are to be tried; the call returns every pair's EA, and for each group the first
// pair whose EA reaches min_ea with its path and score. Only that pair gets a dense posterior and a trace-back: the EA of a pair is known
// after the finishing kernel. The list runs in CHUNKS of MPCGPU_SEARCH_CHUNK pairs (512; at most 1024), cut wherever the count falls, also
// inside a group: the host knows after a chunk's one wait which groups have their hit, and a group that has one enters the later chunks
// with no candidates to try (its pairs are still swept: the caller gets every EA). A chunk takes one of two routes, with the same bits:
//   fused    what align_pairs_small asks of its list (no row-block pair, every alignment a one-wave alignment, the row-list finishing
//            kernel): sweeps and finishing kernel as there, then search_pick_kernel, dense_post_pick_kernel and calc_aln_wave_pick_kernel
//            (kernels_search.h, kernels_aln.h) on one stream, nothing read back in between, one wait.
//   general  everything else, a chunk whose candidate room overflowed on the fused route, and every chunk under MPCGPU_SEARCH_FUSED=0:
//            stage A as mpcgpu_align_pairs runs it (it regrows the room), the EAs read back, the picks made on the host, the dense
//            posteriors of the picked pairs alone (the indirect kernels again, the picks uploaded) and align_dense on them.

extern "C++" {
namespace {

const u32 SEARCH_CHUNK_DEFAULT = 512, SEARCH_CHUNK_MAX = 1024;

struct SearchOut { const u32 *group_first; u32 path_stride; char *paths; u32 *pathlens, *accepted; float *scores, *ea; };

// group g found its hit: pair q of the caller's list, whose result record {length, score, path} is rec
int search_accept(mpcgpu_ctx *c, const SearchOut &o, u32 g, u64 q, const char *rec, u32 LX, u32 LY, std::vector<u8> &open)
{
	if (aln_rec_read(c, "mpcgpu_search_pairs", rec, LX, LY, o.paths + (u64)g * o.path_stride, &o.pathlens[g], o.scores ? &o.scores[g] : nullptr)) return 1;
	o.accepted[g] = (u32)(q - o.group_first[g]);
	open[g] = 0;
	c->se.traced += 1;
	return 0;
}

int search_events(mpcgpu_ctx *c)
{
	if (!c->se.ev0) HIPCHK(c, hipEventCreate(&c->se.ev0));
	if (!c->se.ev1) HIPCHK(c, hipEventCreate(&c->se.ev1));
	return 0;
}
int search_elapsed(mpcgpu_ctx *c)
{
	float ms = 0;
	HIPCHK(c, hipEventSynchronize(c->se.ev1));
	HIPCHK(c, hipEventElapsedTime(&ms, c->se.ev0, c->se.ev1));
	c->se.ms += ms;
	return 0;
}

// One chunk on the fused route: pairs [q0, q0 + np) of the caller's list, grp[q] the group of pair q0 + q, open[g] = group g has no hit yet.
// 0 = done, 1 = error, 2 = not applicable, or a candidate list overflowed (nothing handed out): the general route takes the chunk
int search_chunk_fused(mpcgpu_ctx *c, u64 q0, u32 np, const u32 *px, const u32 *py, const u32 *grp, std::vector<u8> &open, float min_ea, const SearchOut &o)
{
	mpcgpu_ctx::SearchState &S = c->se;
	const StageAGeom g = stage_a_geom(c, np, px, py);
	u32 Lsum_max = 0;
	if (!short_list_fits(c, g, np, px, py, &Lsum_max)) return 2;
	short_list_mark(c, np, px, py);
	c->sh_nnz.clear(); c->sh_ea.clear();
	// ---- the slots: the runs of one group; a slot of a group that has its hit keeps count 0 and gets no matrix
	std::vector<u32> sg, sfirst, slen;
	for (u32 q = 0; q < np;) {
		u32 e = q;
		while (e < np && grp[e] == grp[q]) ++e;
		sg.push_back(grp[q]); sfirst.push_back(q); slen.push_back(e - q);
		q = e;
	}
	const u32 ns = (u32)sg.size();
	std::vector<u64> off(ns + 1, 0);
	for (u32 s = 0; s < ns; ++s) {
		u64 cells = 0;
		for (u32 q = sfirst[s]; open[sg[s]] && q < sfirst[s] + slen[s]; ++q) cells = std::max(cells, (u64)c->len[px[q]] * c->len[py[q]]);
		off[s + 1] = off[s] + cells;
	}
	// ---- the page-locked record: what the kernels read (copied to the device once) and what the host reads back
	const u64 rstride = aln_rec_stride(Lsum_max);
	const u64 o_bx = 0, o_by = o_bx + 4 * (u64)np, o_order = o_by + 4 * (u64)np, o_first = o_order + 4 * (u64)np, o_count = o_first + 4 * (u64)ns,
		o_off = (o_count + 4 * (u64)ns + 7) & ~7ull, in_bytes = o_off + 8 * ((u64)ns + 1),
		o_flags = in_bytes, o_ea = o_flags + 4 * (u64)np, o_pick = o_ea + 4 * (u64)np, o_acc = o_pick + 4 * (u64)ns,
		o_res = (o_acc + 4 * (u64)ns + 7) & ~7ull, bytes = o_res + (u64)ns * rstride;
	HIPCHK(c, S.h.ensure(bytes));
	char *h = S.h.as<char>();
	u32 *order = (u32 *)(h + o_order), *hfirst = (u32 *)(h + o_first), *hcnt = (u32 *)(h + o_count);
	memcpy(h + o_bx, px, 4 * (size_t)np);
	memcpy(h + o_by, py, 4 * (size_t)np);
	memcpy(h + o_off, off.data(), 8 * ((size_t)ns + 1));
	for (u32 s = 0; s < ns; ++s) { hfirst[s] = sfirst[s]; hcnt[s] = open[sg[s]] ? slen[s] : 0u; }
	u32 hcount[MPC_HMAX + 1];
	short_list_order(c, np, px, order, hcount);
	u32 *pick = (u32 *)(h + o_pick), *acc = (u32 *)(h + o_acc);
	for (u32 s = 0; s < ns; ++s) pick[s] = acc[s] = MPC_PICK_NONE;
	// ---- scratch
	if (ensure_pair_scratch(c, g, np)) return 1;
	HIPCHK(c, S.d_in.ensure_grow(in_bytes));
	HIPCHK(c, S.d_nnz.ensure_grow(4 * (u64)np));
	HIPCHK(c, S.d_ea.ensure_grow(4 * (u64)np));
	HIPCHK(c, S.d_flags.ensure_grow(4 * (u64)np));
	HIPCHK(c, c->d_aln_post.ensure_grow(std::max<u64>(off[ns], 1) * 4));
	HIPCHK(c, c->d_aln_rev.ensure_grow((u64)ns * Lsum_max + 16));
	if (search_events(c)) return 1;
	HIPCHK(c, hipMemcpyAsync(S.d_in.p, h, in_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, hipMemsetAsync(S.d_flags.p, 0, 4 * (size_t)np, c->stream));
	const char *d = S.d_in.as<char>();
	const u32 *bx = (const u32 *)(d + o_bx), *by = (const u32 *)(d + o_by);
	// ---- sweeps and finishing kernel (align_pairs_small): sizes, EAs and flags stay on the device
	const PostIO io = {bx, by, c->d_seq_len.as<u32>(), c->d_cand.as<u64>(), c->d_cand_cnt.as<u32>(), c->d_res.as<u32>(), S.d_nnz.as<u32>(), S.d_ea.as<float>(), S.d_flags.as<u32>(), np};
	if (short_list_sweeps(c, g, io, (const u32 *)(d + o_order), hcount)) return 1;
	// ---- the pick, and the dense posterior and alignment of the picked pairs alone
	HIPCHK(c, hipEventRecord(S.ev0, c->stream));
	SearchPickParams sp;
	sp.first = (const u32 *)(d + o_first); sp.count = (const u32 *)(d + o_count);
	sp.ea = S.d_ea.as<float>(); sp.flags = S.d_flags.as<u32>(); sp.min_ea = min_ea; sp.nslots = ns; sp.pick = pick; sp.acc = acc;
	MPC_LAUNCH(search_pick_kernel, (ns + MPC_SEARCH_WAVES - 1) / MPC_SEARCH_WAVES, 64 * MPC_SEARCH_WAVES, 0, c->stream, sp);
	HIPCHK(c, hipGetLastError());
	DensePostPickParams dp;
	dp.d.pair_x = bx; dp.d.pair_y = by; dp.d.seq_len = c->d_seq_len.as<u32>();
	dp.d.cand = c->d_cand.as<u64>(); dp.d.capc = g.capc; dp.d.cand_cnt = c->d_cand_cnt.as<u32>(); dp.d.long_min = g.long_min;
	dp.d.out_off = (const u64 *)(d + o_off); dp.d.out = c->d_aln_post.as<float>();
	dp.pick = pick;
	MPC_LAUNCH(dense_post_pick_kernel, ns, 256, 0, c->stream, dp);
	HIPCHK(c, hipGetLastError());
	c->last_post_cells = 0;
	AlnPickParams ap;
	ap.pick = pick; ap.pair_x = bx; ap.pair_y = by; ap.seq_len = c->d_seq_len.as<u32>();
	ap.post = c->d_aln_post.as<float>(); ap.out_off = (const u64 *)(d + o_off);
	ap.rev = c->d_aln_rev.as<char>(); ap.rev_stride = Lsum_max; ap.rec = h + o_res; ap.rec_stride = rstride;
	const size_t smem = aln_wave_smem((u64)g.LXmax + 1);
	aln_smem_raise(c, 5, (const void *)calc_aln_wave_pick_kernel, smem);
	TimedSpan ts;
	if (span_begin(c, 8, &ts)) return 1;
	MPC_LAUNCH(calc_aln_wave_pick_kernel, ns, 64, smem, c->stream, ap);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &ts)) return 1;
	HIPCHK(c, hipEventRecord(S.ev1, c->stream));
	HIPCHK(c, hipMemcpyAsync(h + o_flags, S.d_flags.p, 4 * (size_t)np, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(h + o_ea, S.d_ea.p, 4 * (size_t)np, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream)); // the one wait
	const u32 *flags = (const u32 *)(h + o_flags);
	for (u32 q = 0; q < np; ++q) if (flags[q] & 1u) return 2; // (its pick + dense + alignment time is not counted: nothing of it is handed out)
	if (search_elapsed(c)) return 1;
	if (o.ea) memcpy(o.ea + q0, h + o_ea, 4 * (size_t)np);
	for (u32 s = 0; s < ns; ++s) {
		if (pick[s] == MPC_PICK_NONE) continue;
		const u32 q = pick[s];
		if (!open[sg[s]] || q < sfirst[s] || q >= sfirst[s] + slen[s] || acc[s] != q - sfirst[s]) return fail(c, "mpcgpu_search_pairs: pick of slot %u out of range (internal error)", s);
		if (search_accept(c, o, sg[s], q0 + q, h + o_res + (u64)s * rstride, c->len[px[q]], c->len[py[q]], open)) return 1;
	}
	return 0;
}

// One chunk on the general route: stage A as mpcgpu_align_pairs runs it (a sub-chunk that stage A cuts into several batches is halved,
// down to one pair), the picks on the host from the EAs stage A read back, dense posterior and alignment for the picked pairs only
int search_chunk_general(mpcgpu_ctx *c, u64 q0, u32 np, const u32 *px, const u32 *py, const u32 *grp, std::vector<u8> &open, float min_ea, const SearchOut &o)
{
	mpcgpu_ctx::SearchState &S = c->se;
	u32 sub = np;
	for (u32 p0 = 0; p0 < np;) {
		const u32 *sx = px + p0, *sy = py + p0;
		u32 nq = std::min<u32>(sub, np - p0);
		for (;;) {
			if (stage_a(c, nq, sx, sy)) return 1;
			if (c->sa_b0 == 0 && c->sa_B == nq) break;
			if (nq == 1) return fail(c, "mpcgpu_search_pairs: pair %llu (%u x %u residues) does not fit one stage-A batch", (unsigned long long)(q0 + p0), c->len[sx[0]], c->len[sy[0]]);
			nq = (nq + 1) / 2;
		}
		sub = std::min(sub, nq);
		if (o.ea) memcpy(o.ea + q0 + p0, c->sh_ea.data(), 4 * (size_t)nq);
		// ---- uclust.cpp:44-54 on the host: the first pair of a group still open whose EA reaches the threshold
		std::vector<u32> pk, kx, ky;
		std::vector<u8> taken(open); // (open[] itself moves when the result is in)
		for (u32 q = 0; q < nq; ++q) {
			const u32 gq = grp[p0 + q];
			if (!taken[gq] || !(c->sh_ea[q] >= min_ea)) continue;
			taken[gq] = 0;
			pk.push_back(q); kx.push_back(sx[q]); ky.push_back(sy[q]);
		}
		// the picked pairs in runs whose dense matrices fit the device together (pairs_that_fit: halved down to one pair, as mpcgpu_align_pairs
		// bounds its chunks); the candidate lists of the whole batch stay where stage A left them
		for (u32 k0 = 0; k0 < (u32)pk.size();) {
			u32 nk = (u32)pk.size() - k0;
			if (pairs_that_fit(c, kx.data() + k0, ky.data() + k0, &nk)) return 1;
			const std::vector<u32> rpk(pk.begin() + k0, pk.begin() + k0 + nk);
			std::vector<u64> roff(nk + 1, 0);
			u32 stride = 1;
			for (u32 k = 0; k < nk; ++k) {
				roff[k + 1] = roff[k] + (u64)c->len[kx[k0 + k]] * c->len[ky[k0 + k]];
				stride = std::max(stride, c->len[kx[k0 + k]] + c->len[ky[k0 + k]]);
			}
			std::vector<char> tpaths((size_t)nk * stride);
			std::vector<u32> tlens(nk, 0);
			std::vector<float> tsc(nk, 0.0f);
			if (search_events(c)) return 1;
			HIPCHK(c, hipEventRecord(S.ev0, c->stream));
			// the dense posteriors of the picked pairs alone (positions rpk[] of the batch) at roff[] of d_aln_post
			if (upload(c, S.d_pick, rpk) || dense_posts(c, "mpcgpu_search_pairs: MPCGPU_POST=sort: the row-list finishing kernel whose candidate lists this entry point rebuilds the "
				"dense posteriors from is switched off", nk, roff, S.d_pick.as<u32>())) return 1;
			if (align_dense(c, nk, kx.data() + k0, ky.data() + k0, roff, stride, tpaths.data(), tlens.data(), tsc.data(), nullptr)) return 1;
			HIPCHK(c, hipEventRecord(S.ev1, c->stream));
			if (search_elapsed(c)) return 1;
			for (u32 k = 0; k < nk; ++k) {
				const u32 gk = grp[p0 + rpk[k]];
				memcpy(o.paths + (u64)gk * o.path_stride, tpaths.data() + (size_t)k * stride, tlens[k]);
				o.pathlens[gk] = tlens[k];
				if (o.scores) o.scores[gk] = tsc[k];
				o.accepted[gk] = (u32)(q0 + p0 + rpk[k] - o.group_first[gk]);
				open[gk] = 0;
				S.traced += 1;
			}
			k0 += nk;
		}
		p0 += nq;
	}
	return 0;
}

} // namespace
} // extern "C++"

int mpcgpu_search_pairs(mpcgpu_ctx *c, uint32_t ngroups, const uint32_t *group_first, const uint32_t *seq1, const uint32_t *seq2, float min_ea,
	uint32_t path_stride, char *paths, uint32_t *pathlens, uint32_t *accepted, float *scores, float *ea)
{
	if (!c) return 1;
	// ---- the refusals: before any device work, the context (epoch, scratch, what mpcgpu_search_info reports) left as it was
	if (c->n == 0) return fail(c, "mpcgpu_search_pairs: call mpcgpu_set_seqs / mpcgpu_set_seqs_registry first");
	if (!group_first || !seq1 || !seq2 || !paths || !pathlens || !accepted) return fail(c, "mpcgpu_search_pairs: NULL argument");
	if (group_first[0] != 0) return fail(c, "mpcgpu_search_pairs: group_first[0] is %u, not 0", group_first[0]);
	for (u32 g = 0; g < ngroups; ++g)
		if (group_first[g + 1] < group_first[g]) return fail(c, "mpcgpu_search_pairs: group_first is not ascending at group %u (%u after %u)", g, group_first[g + 1], group_first[g]);
	const u32 npairs = group_first[ngroups];
	for (u32 q = 0; q < npairs; ++q) {
		if (seq1[q] >= c->n || seq2[q] >= c->n) return fail(c, "mpcgpu_search_pairs: sequence index out of range in pair %u", q);
		if ((u64)c->len[seq1[q]] + c->len[seq2[q]] > path_stride) return fail(c, "mpcgpu_search_pairs: path_stride %u too small for pair %u", path_stride, q);
	}
	for (u32 q = 0; q < npairs; ++q) { // calcposteriorflat.cpp:54-61: mpcgpu_align_pairs' envelope
		const u32 LX = c->len[seq1[q]], LY = c->len[seq2[q]];
		if (double(LX) * double(LY) * 5 + 100 > double(INT_MAX))
			return fail(c, "mpcgpu_search_pairs: pair %u is too long for a dense posterior: LX=%u, LY=%u, LX*LY*5 + 100 exceeds INT_MAX = %d", q, LX, LY, INT_MAX);
	}
	HIPCHK(c, hipSetDevice(c->device));
	++c->epoch;
	mpcgpu_ctx::SearchState &S = c->se;
	S.groups = ngroups; S.pairs = npairs; S.traced = S.chunks = S.general = 0; S.ms = 0;
	const SearchOut o = {group_first, path_stride, paths, pathlens, accepted, scores, ea};
	std::vector<u32> grp(npairs);
	for (u32 g = 0; g < ngroups; ++g) {
		accepted[g] = MPC_PICK_NONE; pathlens[g] = 0;
		for (u32 q = group_first[g]; q < group_first[g + 1]; ++q) grp[q] = g;
	}
	std::vector<u8> open(ngroups, 1);
	const u32 chunk = (u32)std::min<int>(std::max(env_int("MPCGPU_SEARCH_CHUNK", (int)SEARCH_CHUNK_DEFAULT), 1), (int)SEARCH_CHUNK_MAX);
	const bool fused = env_int("MPCGPU_SEARCH_FUSED", 1) != 0;
	int rc = 0;
	for (u32 q0 = 0; q0 < npairs && !rc; q0 += chunk) {
		const u32 np = std::min<u32>(chunk, npairs - q0);
		S.chunks += 1;
		rc = fused ? search_chunk_fused(c, q0, np, seq1 + q0, seq2 + q0, grp.data() + q0, open, min_ea, o) : 2;
		if (rc == 2) {
			S.general += 1;
			rc = search_chunk_general(c, q0, np, seq1 + q0, seq2 + q0, grp.data() + q0, open, min_ea, o);
		}
	}
	// no sparse matrices are kept: mpcgpu_get_list_sparse refuses until another list stage has run
	c->have_shard = false; c->ap_x.clear(); c->ap_y.clear();
	S.last = true;
	return rc;
}

int mpcgpu_search_info(mpcgpu_ctx *c, uint64_t out[6])
{
	if (!c) return 1;
	if (!out) return fail(c, "mpcgpu_search_info: NULL argument");
	const mpcgpu_ctx::SearchState &S = c->se;
	out[0] = S.groups; out[1] = S.pairs; out[2] = S.traced; out[3] = S.chunks; out[4] = S.general;
	out[5] = (u64)(S.ms * 1e6); // nanoseconds
	return 0;
}

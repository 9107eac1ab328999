// mpcgpu_stage_a.inc — stage A (part of mpcgpu.cpp's translation unit): batching, chains, launches of the forward/backward and
// finishing kernels, the packed shard. Reference: MPCFlat::CalcPosteriors, mpcflat.cpp:239-251; CalcPosterior, calcposteriorflat.cpp:45-92.
// the constant part of a forward/backward launch: sequences, PairHMM scores, tables, candidate buffers (the work list, queue and
// forward-plane scratch are set per launch)
static void fill_fb_params(mpcgpu_ctx *c, FbParams &fp, const u32 *pair_x, const u32 *pair_y, u32 capc, bool mega)
{
	fp.seq_code = c->d_seq_code.as<u8>(); fp.seq_off = c->d_seq_off.as<u64>(); fp.seq_len = c->d_seq_len.as<u32>();
	fp.tSM = c->start[0]; fp.tSI = c->start[1]; fp.tSJ = c->start[3]; // pairhmm.h:11-19: M,IX,IY,JX,JY
	fp.tMM = c->trans[0 * 5 + 0]; fp.tMI = c->trans[0 * 5 + 1]; fp.tMJ = c->trans[0 * 5 + 3];
	fp.tII = c->trans[1 * 5 + 1]; fp.tIM = c->trans[1 * 5 + 0];
	fp.tJJ = c->trans[3 * 5 + 3]; fp.tJM = c->trans[3 * 5 + 0];
	fp.thr = c->thr; fp.A = c->A; fp.match = c->d_match.as<float>(); fp.ins = c->d_ins.as<float>();
	fp.pair_x = pair_x; fp.pair_y = pair_y;
	fp.cand = c->d_cand.as<u64>(); fp.capc = capc; fp.cand_cnt = c->d_cand_cnt.as<u32>();
	fp.total = c->d_total.as<float>();
	fp.mg_prof = mega ? c->d_mg_prof.as<u64>() : nullptr; fp.mg_ins = mega ? c->d_mg_ins.as<float>() : nullptr;
	fp.mg_tab = mega ? c->d_mg_tab.as<float>() : nullptr; fp.mg_tab_floats = mega ? c->mg_tab_floats : 0;
	for (u32 f = 0; f < MPC_MEGA_FMAX; ++f) { fp.mg_base[f] = mega ? c->mg_base[f] : 0; fp.mg_alpha[f] = mega ? c->mg_alpha[f] : 0; }
	fp.order = nullptr; fp.count = 0; fp.queue = nullptr; fp.fm_scratch = nullptr; fp.fm_stride = 0;
	fp.bnd = nullptr; fp.bnd_stride = 0; fp.bnd_ld = 0; fp.fm_block = 0;
}

// ---- the stage's limits, computed once from the pair list (stage_a, align_pairs_small; mpcgpu_post_scores fills in its one pair)
static const int SA_WAVES = 4, SA_BLOCK = 64 * SA_WAVES; // forward/backward kernels: waves, threads per workgroup
struct StageAGeom {
	u32 LXmax = 0, LYmax = 0;   // longest row / column sequence of the list
	u32 LXlong = 0, LYlong = 0; // ... over the row-block (LONG) pairs, LX >= long_min; 0: there are none
	u32 long_min = 0;
	u32 capc = 0;               // candidates per pair: stage_a's overflow retry doubles it HERE, every size below follows
	bool mega = false; size_t fb_smem = 0; u64 work_cells = 0;
	u64 res_stride() const { return (u64)LXmax + LYmax + 4 * (u64)capc; } // words of a pair's fixed-stride record
};
static StageAGeom stage_a_geom(const mpcgpu_ctx *c, u64 np, const u32 *px, const u32 *py)
{
	StageAGeom g;
	// X longer than 64*MPC_HMAX rows: row-block (LONG) kernels, 16-bit row/column candidate keys
	// Row sequences from 769 residues on take the row-block kernels: one block of 13..16 rows per lane needs 177..219 VGPRs (2 waves
	// per SIMD), blocks of 4 rows per lane 166 (3 waves): 300 x L~1000 fb 439 -> 366 ms; up to 12 rows per lane (<= 167 VGPRs)
	// the single block wins (400 x L~600: 228 against 297 ms). 1025 is where a single block stops being possible.
	g.long_min = (u32)std::min(std::max(env_int("MPCGPU_FB_LONG_MIN", 64 * 12 + 1), 2), 64 * MPC_HMAX + 1);
	for (u64 k = 0; k < np; ++k) {
		const u32 LX = c->len[px[k]], LY = c->len[py[k]];
		g.LXmax = std::max(g.LXmax, LX); g.LYmax = std::max(g.LYmax, LY);
		g.work_cells += (u64)(LX + 1) * (LY + 1);
		if (LX >= g.long_min) { g.LXlong = std::max(g.LXlong, LX); g.LYlong = std::max(g.LYlong, LY); }
	}
	g.capc = std::max((u32)std::max(env_int("MPCGPU_CAND_PER_ROW", 12), 1) * std::max(g.LXmax, g.LYmax), 1024u);
	g.mega = c->have_mega;
	g.fb_smem = (g.mega ? (size_t)c->mg_tab_floats : (size_t)c->A * c->A + c->A) * sizeof(float);
	return g;
}
// the row-list finishing kernel (no sorts, 3 LDS trips per EA row) takes a list whose sequences fit its LDS arrays (up to ~12 000
// positions: three arrays of one word per position + the sorted-list buffer of sort_cap entries in the CU's LDS)
static bool post_rows_fits(u32 LXmax, u32 LYmax, u32 sort_cap)
{
	return ((size_t)LXmax + 2 + 2 * ((size_t)LYmax + 2)) * 4 + 8 + 8 * (size_t)sort_cap <= 150 * 1024;
}

// MPCGPU_SCRATCH_GB, read once per stage. batch: the candidates and records of a batch — unset = 32 GB, 0 = no room at all = one pair per
// batch ("the smallest batches" of the tests). planes: the forward M planes of the chain and row-block kernels — unset = no cap, set
// = at least 1 GB (the planes of a long pair need their room whatever the batches get).
struct ScratchBudget { u64 batch, planes; };
static ScratchBudget scratch_budget()
{
	const char *s = getenv("MPCGPU_SCRATCH_GB");
	const bool set = s && *s;
	return {(u64)(set ? atoi(s) : 32) << 30, set ? (u64)std::max(atoi(s), 1) << 30 : ~0ull};
}

// Host side of a batch (sizing, bins, launch order): prepared for batch b+1 while the device runs batch b.
struct BatchPrep {
	bool valid = false;
	u64 B = 0;
	std::vector<u32> bx, by, order;
	u32 hcount[MPC_HMAX + 2];
	// chains of pairs with the same row sequence (fb_chain_kernel): members in `order` behind the single pairs
	std::vector<u32> chain_first, chain_cnt;
	u32 ccount[MPC_HMAX + 1];   // chains per rows-per-lane bin
	u32 cvmax[MPC_HMAX + 1];    // longest virtual column axis of a bin's chains
	u32 coop_pairs = 0, coop_waves = 0; // set by the launch: row-block pairs that went to fb_coop_kernel, and its waves per pair
	// fused bins (ChainPlan::fuse): `rest` lists the pairs the sweeps do not finish, for the separate finishing launch
	u64 fused = 0; // pairs the sweeps finish
	std::vector<u32> rest;
};

// Chains: consecutive pairs of the list with the same row sequence (the all-pairs order is full of them), each with
// LY + 1 >= T (kernels_fbc.h), up to MPCGPU_FB_CHAIN_MAX (default 16) pairs and as many columns as the forward M planes of the
// resident waves may take (a quarter of the free memory, 32 GB at most). MPCGPU_FB_CHAIN=0: every pair on its own (fb_kernel).
// With structure profiles (g.mega) the chains run in fb_chain_mega_kernel, bin by bin under MPCGPU_FB_CHAIN_MEGA (chain_plan).
struct ChainPlan {
	bool mega = false; // the chain kernel's MEGA instantiations (smem: the feature tables in front of the chain tables)
	bool on = false, grade = true; // grade = false: no shorter chains at the end of a launch (MPCGPU_FB_CHAIN_GRADE=0: tests)
	u32 max = 0; size_t smem = 0;
	u32 vcap[MPC_HMAX + 1] = {0}; // columns a chain of a rows-per-lane bin may have; 0: the bin takes no chains
	// fb_chain_post_kernel (fuse_plan): the bins whose chains are finished inside the sweeps, the LDS list of a wave there, any bin at all
	bool fuse[MPC_HMAX + 1] = {false}, fuse_any = false;
	u32 fuse_sort_cap[MPC_HMAX + 1] = {0};
	u32 post_batch = 64;
};
// bytes of the three per-position LDS arrays of the row-list finishing code
static size_t post_rows_fixed_lds(const StageAGeom &g) { return ((((size_t)g.LXmax + 2 + 2 * ((size_t)g.LYmax + 2)) * 4 + 7) & ~(size_t)7); }
static size_t fuse_smem(const ChainPlan &cp, const StageAGeom &g, u32 sort_cap) { return cp.smem + (size_t)SA_WAVES * (post_rows_fixed_lds(g) + 8 * (size_t)sort_cap); }

// Unset is 0: at 7 rows per lane (1000 x L~400) the fused kernel does not fit the sweeps' 128 registers without scratch memory, and
// neither that bin as fuse_plan now sizes it nor the bins that do fit have a device time on record (DESIGN.md 4.2: the one run of a
// fused H = 7, 880 against 542 ms, was of an earlier form at half the residency).
static const int kFbPostFuseDefault = 0;
// MPCGPU_FB_POST_FUSE. Which bins of the chain kernel finish their pairs inside the sweeps (fb_chain_post_kernel). 2 (the rule): a bin is fused when
// a workgroup with the waves' finishing slices — the per-position arrays and a list of at least 2 and at most min(capc, sort_cap) entries, as many
// as fit — is as often resident on a CU as the plain chain kernel's is and the instantiation uses no scratch memory (at 6 to 8 rows per lane the
// finishing code does not fit the 128 registers of the sweeps without spilling). 1: wherever the workgroup fits at all — with scratch memory,
// and at a lower residency where even a list of 2 entries costs the chain kernel's. 0 (and unset): never. Fusing needs the row-list finishing code
// (post_rows) and, with more than one batch, a second set of record buffers (the sweeps of batch b + 1 write records while those of
// batch b wait for their pack): the list is fused only when that set — the records of a batch at most — takes no more than a quarter of the free memory.
static int fuse_plan(mpcgpu_ctx *c, const StageAGeom &g, u64 np, u64 batch_budget, bool post_rows, u32 sort_cap, ChainPlan &cp)
{
	const int env = env_int("MPCGPU_FB_POST_FUSE", kFbPostFuseDefault);
	cp.post_batch = (u32)std::min(std::max(env_int("MPCGPU_POST_BATCH", 64), 1), 64);
	if (!cp.on || cp.mega || !post_rows || env == 0) return 0; // (the fused kernel is byte-only)
	size_t freeb = 0, totb = 0;
	HIPCHK(c, hipMemGetInfo(&freeb, &totb));
	const u64 owned = (u64)c->d_cand.cap + c->d_res.cap + c->d_res_n.cap + c->d_fm.cap;
	const u64 second = std::min<u64>(np * g.res_stride() * 4, std::min<u64>(batch_budget, (u64)((freeb + owned) * 0.4)));
	if (second > (freeb + c->d_res_n.cap) / 4) {
		if (trace_on()) { fprintf(stderr, "[mpcgpu] fb chain post: not fused, a second set of records (%llu B) is more than a quarter of the free memory (%zu B)\n", second, freeb + c->d_res_n.cap); fflush(stderr); }
		return 0;
	}
	const u32 top = std::max(std::min<u32>(g.capc, sort_cap), 2u);
	for (u32 H = 1; H <= MPC_HMAX; ++H) {
		if (!cp.vcap[H]) continue;
		const int occ0 = occ_fbc_h((int)H, false, SA_BLOCK, cp.smem);
		if (env != 1 && fbcp_spills_h((int)H)) continue; // held to the sweeps' registers, the finishing code spilled: not by the rule
		const int occ2 = occ_fbcp_h((int)H, SA_BLOCK, fuse_smem(cp, g, 2));
		const int need = occ2 >= occ0 ? occ0 : env == 1 ? 1 : occ0;
		if (occ2 < need) continue;
		u32 lo = 2, hi = top; // the largest list with which `need` workgroups stay resident
		while (lo < hi) {
			const u32 mid = lo + (hi - lo + 1) / 2;
			if (occ_fbcp_h((int)H, SA_BLOCK, fuse_smem(cp, g, mid)) >= need) lo = mid; else hi = mid - 1;
		}
		cp.fuse[H] = true; cp.fuse_sort_cap[H] = lo; cp.fuse_any = true;
	}
	return 0;
}
// MPCGPU_FB_CHAIN_MEGA. Which bins chain when structure profiles are loaded (fb_chain_mega_kernel<H> in place of fb_kernel<H, true>). 0: none.
// 1: every bin whose workgroup the chip takes. 2 (the rule): bin H only where fb_chain_mega_kernel<H> is resident at least as often as
// fb_kernel<H, true> — workgroups per CU at SA_BLOCK threads, each with its own LDS — and uses no scratch memory: the chain kernel
// carries the chain's bookkeeping beside the sweep's registers, and a bin that paid for it with residency would lose more than the fill
// and drain it saves. Unset is 0: the rule becomes the default only when every bin it enables has been MEASURED no slower than
// fb_kernel<H, true> beyond the run-to-run spread (DESIGN.md 4.1).
static const int kFbChainMegaDefault = 0;
static int chain_plan(mpcgpu_ctx *c, const StageAGeom &g, u64 planes_budget, ChainPlan &cp)
{
	const int mega_env = g.mega ? env_int("MPCGPU_FB_CHAIN_MEGA", kFbChainMegaDefault) : 1;
	cp.mega = g.mega;
	cp.on = env_int("MPCGPU_FB_CHAIN", 1) != 0 && mega_env != 0;
	cp.max = (u32)std::min(std::max(env_int("MPCGPU_FB_CHAIN_MAX", 16), 2), MPC_CHAIN_MAX);
	cp.grade = env_int("MPCGPU_FB_CHAIN_GRADE", 1) != 0;
	cp.smem = g.fb_smem + (size_t)SA_WAVES * MPC_CHAIN_TAB_BYTES; // the emission tables (MEGA: the feature tables), then the waves' chain tables
	if (!cp.on) return 0;
	size_t freeb = 0, totb = 0;
	HIPCHK(c, hipMemGetInfo(&freeb, &totb));
	// (a quarter of what is free, 32 GB at most — and no more than MPCGPU_SCRATCH_GB where that is set: several contexts on one
	// device, e.g. the eight of tests/test_gpu_parity.py::test_group_of_eight_contexts_config3_digests, each see the same free memory)
	const u64 fm_budget = std::min<u64>(std::min<u64>((u64)32 << 30, planes_budget), (u64)((freeb + c->d_fm.cap) * 0.25));
	bool any = false;
	for (u32 H = 1; H <= MPC_HMAX; ++H) {
		if (g.mega) { // the bin chains only where the knob lets it; elsewhere vcap stays 0 and build_chains leaves its pairs to fb_kernel
			const int occ_c = occ_fbcm_fit_h((int)H, SA_BLOCK, cp.smem);
			bool take = occ_c >= 1;
			if (take && mega_env != 1) take = occ_c >= occ_fb_h((int)H, true, SA_BLOCK, g.fb_smem) && !fbcm_spills_h((int)H);
			if (trace_on()) { fprintf(stderr, "[mpcgpu] fb chain mega: H=%u %s (workgroups per CU: chain %d, single %d)\n", H, take ? "chains" : "stays on fb_kernel", occ_c, occ_fb_h((int)H, true, SA_BLOCK, g.fb_smem)); fflush(stderr); }
			if (!take) continue;
		}
		const u64 waves = (u64)c->prop.multiProcessorCount * (u32)occ_fbc_h((int)H, g.mega, SA_BLOCK, cp.smem) * SA_WAVES;
		const u64 steps = fm_budget / (waves * H * 64 * 4);
		cp.vcap[H] = steps > 64 + 2 ? (u32)std::min<u64>(steps - 64, 1u << 24) : 0;
		any = any || cp.vcap[H];
	}
	if (g.mega && !any) cp.on = false; // no bin chains: the stage is the one MPCGPU_FB_CHAIN_MEGA=0 runs
	return 0;
}

// The chains of a batch. Every pair the chain kernel can take goes to it (a pair on its own is a chain of one), so a bin is ONE launch;
// the chains of a launch are served longest first, and the last ones are cut shorter (4, 2, 1 pairs for about one round of the resident
// waves each) so that the waves finish together. Out: the chains by bin, longest first; chained[q] = pair q is in one; P.cvmax.
struct Chain { u32 q0, cnt, H; u64 work; };
static void build_chains(const mpcgpu_ctx *c, const ChainPlan &cp, u32 long_min, BatchPrep &P, std::vector<Chain> &chains, std::vector<unsigned char> &chained)
{
	const u64 B = P.B;
	auto work_of = [c, &P](u32 q0, u32 cnt, u32 H, u32 T) {
		u64 V = 0;
		for (u32 k = 0; k < cnt; ++k) V += c->len[P.by[q0 + k]] + 1;
		return (V + T) * H;
	};
	u64 q = 0;
	while (q < B) {
		const u32 LX = c->len[P.bx[q]];
		const u32 H = (LX + 63) / 64;
		if (LX >= long_min || H < 1 || H > MPC_HMAX || c->len[P.by[q]] + 1 > cp.vcap[H]) { ++q; continue; }
		const u32 T = (LX + H - 1) / H;
		u64 e = q;
		u64 V = 0;
		while (e < B && P.bx[e] == P.bx[q] && e - q < cp.max) {
			const u32 LY = c->len[P.by[e]];
			if (LY + 1 < T || V + LY + 1 > cp.vcap[H]) break;
			V += LY + 1;
			++e;
		}
		if (e == q) e = q + 1; // a pair too short to chain: on its own
		chains.push_back({(u32)q, (u32)(e - q), H, 0});
		for (u64 k = q; k < e; ++k) chained[k] = 1;
		q = e;
	}
	for (Chain &ch : chains) { const u32 LX = c->len[P.bx[ch.q0]]; ch.work = work_of(ch.q0, ch.cnt, ch.H, (LX + ch.H - 1) / ch.H); }
	auto by_bin_and_work = [](const Chain &a, const Chain &b) { return a.H != b.H ? a.H < b.H : a.work != b.work ? a.work > b.work : a.q0 < b.q0; };
	std::sort(chains.begin(), chains.end(), by_bin_and_work);
	// the short end of every bin
	std::vector<Chain> graded;
	graded.reserve(chains.size() * 2);
	size_t lo = 0;
	while (lo < chains.size()) {
		size_t hi = lo;
		while (hi < chains.size() && chains[hi].H == chains[lo].H) ++hi;
		const u32 H = chains[lo].H;
		const u64 waves = (u64)c->prop.multiProcessorCount * (u32)occ_fbc_h((int)H, cp.mega, SA_BLOCK, cp.smem) * SA_WAVES;
		const u64 gw = std::max<u64>(waves, 1); // pairs per grade: one round of the resident waves
		u64 seen = 0; // pairs, counted from the end of the bin
		for (size_t k = hi; k-- > lo;) {
			const Chain &ch = chains[k];
			const u32 piece = !cp.grade ? ch.cnt : seen < gw ? 1u : seen < 3 * gw ? 2u : seen < 7 * gw ? 4u : ch.cnt;
			seen += ch.cnt;
			const u32 LX = c->len[P.bx[ch.q0]];
			for (u32 o = 0; o < ch.cnt; o += piece) {
				const u32 n = std::min(piece, ch.cnt - o);
				graded.push_back({ch.q0 + o, n, H, work_of(ch.q0 + o, n, H, (LX + H - 1) / H)});
			}
		}
		lo = hi;
	}
	std::sort(graded.begin(), graded.end(), by_bin_and_work);
	chains.swap(graded);
	for (const Chain &ch : chains) {
		u64 V = 0;
		for (u32 k = 0; k < ch.cnt; ++k) V += c->len[P.by[ch.q0 + k]] + 1;
		P.cvmax[ch.H] = std::max<u32>(P.cvmax[ch.H], (u32)V);
	}
}

// Batch [b0, b0 + B) of the list: B from the memory there is, the pairs binned by rows per lane and ordered by work.
// records = false (mpcgpu_ea_scores): the batch leaves no fixed-stride records, a pair costs its candidate room alone.
static int prepare_batch(mpcgpu_ctx *c, const StageAGeom &g, const ChainPlan &cp, u64 batch_budget, u64 np, const u32 *px, const u32 *py, u64 b0, BatchPrep &P, bool records = true)
{
	// ---- batch sizing: candidates + fixed-stride records per pair
	const u64 per_pair = (u64)g.capc * 8 + (records ? g.res_stride() * 4 : 0) + 64;
	size_t freeb = 0, totb = 0;
	HIPCHK(c, hipMemGetInfo(&freeb, &totb));
	// the scratch of the previous batch (or of an overflow retry) is already owned and gets reused: count it as available
	const u64 owned = (u64)c->d_cand.cap + c->d_res.cap + c->d_res_n.cap + c->d_fm.cap;
	// Fewer, larger batches save the tails of waves that finish alone. Round 5 (batch after batch): 16 GB = four batches at 1000 x L~400;
	// 24 GB / 3 batches: fb 551 -> 545 ms, step 1832 -> 1822; 32 / 2: 541, 1840 — the first batch's host preparation was not covered
	// by device work (profiles/r05a, r05c, r05d).
	// Round 6, with the batches as a pipeline (stage_a): 32 GB / 2 batches 1445.5 ms per step against 1465.8 (16 GB / 4), 1454.3 (24 / 3) and
	// 1472.0 (64 GB: one batch, fb 537 ms but nothing runs beside anything) on one box (profiles/r14o_bench_1000x400_s*.json) -> 32 GB.
	// (The slower cold run round 5 saw with 24 GB was the driver's release of the previous process's memory, not the size: DESIGN.md 4.1.)
	const u64 budget = std::min<u64>(batch_budget, (u64)((freeb + owned) * 0.4));
	// the batches that remain, of equal size (the last one is not a remainder of a few thousand pairs whose waves finish alone)
	const u64 bmax = std::min<u64>(std::max<u64>(1, budget / per_pair), 1u << 22);
	const u64 left = np - b0, nbat = (left + bmax - 1) / bmax;
	const u64 B = (left + nbat - 1) / nbat;
	P.B = B;
	// ---- bin by H, order by work (longest first)
	// one 64-bit key per pair: bin (5 bits) | work, descending (37 bits) | index (22 bits) — a plain integer sort (with a
	// three-array comparator it cost 9 ms per 125 000 pairs)
	P.bx.resize(B); P.by.resize(B); P.order.resize(B);
	std::vector<u64> keys;
	keys.reserve(B);
	for (u32 h = 0; h < MPC_HMAX + 2; ++h) P.hcount[h] = 0; // bin MPC_HMAX+1: the row-block (LONG) pairs
	for (u32 h = 0; h <= MPC_HMAX; ++h) P.ccount[h] = P.cvmax[h] = 0;
	P.chain_first.clear(); P.chain_cnt.clear();
	for (u64 q = 0; q < B; ++q) { P.bx[q] = px[b0 + q]; P.by[q] = py[b0 + q]; }
	std::vector<Chain> chains;
	std::vector<unsigned char> chained(B, 0);
	if (cp.on) build_chains(c, cp, g.long_min, P, chains, chained);
	for (u64 q = 0; q < B; ++q) {
		if (chained[q]) continue;
		const u32 LX = c->len[P.bx[q]], LY = c->len[P.by[q]];
		const bool lng = LX >= g.long_min;
		const u32 H = lng ? MPC_HMAX + 1 : (LX + 63) / 64;
		P.hcount[H]++;
		const u64 wk = lng ? (u64)LX * LY : (u64)(LY + (LX + H - 1) / H) * H; // < 2^37 (lengths < 2^16 when LONG, < 2^22 otherwise with H <= 16)
		keys.push_back(((u64)H << 59) | ((((u64)1 << 37) - 1 - wk) << 22) | q);
	}
	std::sort(keys.begin(), keys.end());
	u64 at = 0;
	for (; at < keys.size(); ++at) P.order[at] = (u32)(keys[at] & (((u64)1 << 22) - 1));
	// the chains: by bin, longest first; their members follow the other pairs in `order`
	for (const Chain &ch : chains) {
		P.ccount[ch.H]++;
		P.chain_first.push_back((u32)at);
		P.chain_cnt.push_back(ch.cnt);
		for (u32 k = 0; k < ch.cnt; ++k) P.order[at++] = ch.q0 + k;
	}
	// what the separate finishing launch is left with when bins are fused: the pairs outside the chain kernel and the chains of the other bins
	P.fused = 0; P.rest.clear();
	if (cp.fuse_any) {
		P.rest.assign(P.order.begin(), P.order.begin() + keys.size());
		for (const Chain &ch : chains) {
			if (cp.fuse[ch.H]) { P.fused += ch.cnt; continue; }
			for (u32 k = 0; k < ch.cnt; ++k) P.rest.push_back(ch.q0 + k);
		}
	}
	P.valid = true;
	return 0;
}

// candidate lists, totals and fixed-stride records of B pairs; the work-queue heads (single pairs per bin, then chains per bin), zeroed
static int ensure_pair_scratch(mpcgpu_ctx *c, const StageAGeom &g, u64 B, bool records = true)
{
	HIPCHK(c, c->d_cand.ensure(B * g.capc * 8));
	HIPCHK(c, c->d_cand_cnt.ensure(B * 4));
	HIPCHK(c, c->d_total.ensure(B * 4));
	if (records) HIPCHK(c, c->d_res.ensure(B * g.res_stride() * 4));
	HIPCHK(c, c->d_queue.ensure(4 * (2 * MPC_HMAX + 4)));
	HIPCHK(c, hipMemsetAsync(c->d_queue.p, 0, 4 * (2 * MPC_HMAX + 4), c->stream));
	return 0;
}

// ---- forward/backward, row-block pairs: cnt entries of `order` (fp: fill_fb_params)
// What both row-block kernels need to know of a launch: rows per lane, blocks and forward-plane floats of the longest pair, the line
// buffer's row length, the memory the planes may take and the workgroups of SA_BLOCK threads a CU keeps resident.
struct RowBlockPlan { u32 long_h = 0, nbmax = 0, ld = 0, occ = 0; u64 fm_block = 0, fm_stride = 0, fm_budget = 0; };
static int row_block_plan(mpcgpu_ctx *c, const StageAGeom &g, u32 cnt, u64 planes_budget, RowBlockPlan &rp)
{
	const u32 cus = (u32)c->prop.multiProcessorCount;
	const int long_h_env = env_int("MPCGPU_FB_LONG_H", 0); // 0 = chosen below, 1 / 4 / 7 = forced (1: tests reach several blocks with short sequences)
	const u32 LXlong = g.LXlong, LYlong = g.LYlong;
	rp.ld = (LYlong + 2 + 63) & ~63u;
	auto planes = [LXlong, LYlong](u32 h, u32 *nb, u64 *blk) { *nb = (LXlong + 64 * h - 1) / (64 * h); *blk = (u64)(LYlong + 64) * h * 64; return *blk * *nb; };
	// resident waves are bounded by the forward M planes they keep (LX*LY floats each)
	size_t freeb = 0, totb = 0;
	HIPCHK(c, hipMemGetInfo(&freeb, &totb));
	// (up to 45 % of what is free, counting the plane buffer already owned: 36 MB per 3000 x 3000 pair — with the 16 GB the
	// other scratch is held to, 444 waves were resident where the chip takes 2048. The buffer stays allocated — hipMalloc and
	// hipFree of ~100 GB take seconds — and is given back only when the store needs the room: mpcgpu_store_import)
	rp.fm_budget = std::min<u64>(planes_budget, (u64)((freeb + c->d_fm.cap) * 0.45));
	// rows per lane: 7 (217 VGPRs, 2 waves per SIMD), or 4 (166 VGPRs, 3 waves per SIMD; more blocks, more line-buffer
	// traffic) when the pairs and the memory for their forward planes can keep more than 2 waves per SIMD busy
	// (100 x L~3000: 517 -> 407 ms; 64 x L~6000, 875 waves fit: 1985 ms with 7 rows, 2190 with 4)
	rp.long_h = long_h_env == 1 ? 1u : long_h_env == MPC_LONG_H_SMALL ? (u32)MPC_LONG_H_SMALL : (u32)MPC_LONG_H;
	if (long_h_env == 0) {
		const u64 stride_small = planes(MPC_LONG_H_SMALL, &rp.nbmax, &rp.fm_block);
		const u64 waves_small = std::min<u64>(cnt, rp.fm_budget / (stride_small * 4 + 16ull * rp.ld * 4));
		if (waves_small > (u64)cus * 4 * 2) rp.long_h = MPC_LONG_H_SMALL;
	}
	rp.fm_stride = planes(rp.long_h, &rp.nbmax, &rp.fm_block);
	rp.occ = (u32)occ_fb_long((int)rp.long_h, g.mega, SA_BLOCK, g.fb_smem);
	return 0;
}

// fb_kernel<H, MEGA, LONG>: a wave per pair, its blocks one after the other
static int launch_fb_row_blocks(mpcgpu_ctx *c, const StageAGeom &g, const RowBlockPlan &rp, FbParams fp, const u32 *order, u32 cnt)
{
	const u32 cus = (u32)c->prop.multiProcessorCount;
	const u32 ld = rp.ld, occ = rp.occ;
	const u64 max_waves = rp.fm_budget / (rp.fm_stride * 4 + 16ull * ld * 4);
	if (max_waves < 1)
		return fail(c, "mpcgpu_calc_posteriors: not enough device memory for the forward plane of a %u x %u pair", g.LXlong, g.LYlong);
	u32 grid = std::min<u32>((cnt + SA_WAVES - 1) / SA_WAVES, cus * occ);
	grid = (u32)std::max<u64>(std::min<u64>(grid, max_waves / SA_WAVES), 1);
	const u32 wpb = max_waves < (u64)SA_WAVES ? (u32)max_waves : (u32)SA_WAVES; // fewer waves per workgroup when memory is that tight
	HIPCHK(c, c->d_fm.ensure((u64)grid * wpb * rp.fm_stride * 4));
	HIPCHK(c, c->d_bnd.ensure((u64)grid * wpb * 16 * ld * 4));
	if (trace_on()) {
		fprintf(stderr, "[mpcgpu] fb row blocks: H=%u pairs=%u blocks<=%u grid=%u x %u waves occ=%u fm=%.1f MB\n", rp.long_h, cnt, rp.nbmax,
			grid, wpb, occ, (double)grid * wpb * rp.fm_stride * 4 / 1048576.0);
		fflush(stderr);
	}
	fp.order = order; fp.count = cnt;
	fp.queue = c->d_queue.as<u32>() + MPC_HMAX + 1;
	fp.fm_scratch = c->d_fm.as<float>(); fp.fm_stride = rp.fm_stride; fp.fm_block = rp.fm_block;
	fp.bnd = c->d_bnd.as<float>(); fp.bnd_stride = 16ull * ld; fp.bnd_ld = ld;
	TimedSpan sp;
	if (span_begin(c, 0, &sp)) return 1;
	launch_fb_long((int)rp.long_h, g.mega, fp, grid, 64 * wpb, g.fb_smem, c->stream);
	HIPCHK(c, hipGetLastError());
	return span_end(c, &sp);
}

// fb_coop_kernel<H, MEGA> (kernels_fbcoop.h): a workgroup of W waves per pair, the blocks as a pipeline. Forward planes and line
// buffers (a row of 8 states per block boundary) are per resident WORKGROUP; with less memory than the resident workgroups need, fewer
// workgroups are launched. One launch of timer family 0, like launch_fb_row_blocks.
static int launch_fb_row_blocks_coop(mpcgpu_ctx *c, const StageAGeom &g, const RowBlockPlan &rp, FbParams fp, const u32 *order, u32 cnt, u32 W)
{
	const u32 cus = (u32)c->prop.multiProcessorCount;
	const u32 ld = rp.ld;
	const size_t smem = g.fb_smem + MPC_FB_COOP_LDS_BYTES;
	const u64 bnd_stride = (u64)rp.nbmax * 8 * ld;
	const u64 max_wgs = rp.fm_budget / (rp.fm_stride * 4 + bnd_stride * 4);
	if (max_wgs < 1)
		return fail(c, "mpcgpu_calc_posteriors: not enough device memory for the forward plane of a %u x %u pair", g.LXlong, g.LYlong);
	const u32 occ = (u32)std::max(occ_fb_coop((int)rp.long_h, g.mega, 64 * W, smem), 1);
	const u32 grid = (u32)std::max<u64>(std::min<u64>(std::min<u32>(cnt, cus * occ), max_wgs), 1);
	HIPCHK(c, c->d_fm.ensure((u64)grid * rp.fm_stride * 4));
	HIPCHK(c, c->d_bnd.ensure((u64)grid * bnd_stride * 4));
	if (trace_on()) {
		fprintf(stderr, "[mpcgpu] fb row blocks: H=%u pairs=%u blocks<=%u grid=%u x %u waves occ=%u fm=%.1f MB\n", rp.long_h, cnt, rp.nbmax,
			grid, W, occ, (double)grid * rp.fm_stride * 4 / 1048576.0);
		fprintf(stderr, "[mpcgpu] fb coop: W=%u waves per pair (fb_coop_kernel), line buffers %.1f MB\n", W, (double)grid * bnd_stride * 4 / 1048576.0);
		fflush(stderr);
	}
	fp.order = order; fp.count = cnt;
	fp.queue = c->d_queue.as<u32>() + MPC_HMAX + 1;
	fp.fm_scratch = c->d_fm.as<float>(); fp.fm_stride = rp.fm_stride; fp.fm_block = rp.fm_block;
	fp.bnd = c->d_bnd.as<float>(); fp.bnd_stride = bnd_stride; fp.bnd_ld = ld;
	TimedSpan sp;
	if (span_begin(c, 0, &sp)) return 1;
	launch_fb_coop((int)rp.long_h, g.mega, fp, grid, 64 * W, smem, c->stream);
	HIPCHK(c, hipGetLastError());
	return span_end(c, &sp);
}

// Waves per pair of a row-block launch: 0 = fb_kernel<.., LONG> (a wave per pair), 2.. = fb_coop_kernel with that many.
// MPCGPU_FB_COOP: 0 = never, 1 = the rule below, 2..16 = that many on every row-block launch, clamped to the waves of a workgroup
// the CU keeps resident for this instantiation (occ_fb_long: VGPRs) and to what the instantiation is compiled for.
// The rule: cooperative only when the launch leaves wave slots empty — fewer row-block pairs than the chip has resident waves for them —
// and the longest pair has at least two blocks; W = min(waves of a workgroup, blocks of the longest pair, resident waves / pairs).
// UNSET is 0 for now: the rule may choose the cooperative kernel only where it has been MEASURED faster than the single-wave kernel
// by more than the run-to-run spread, and no device time of a long pair has been recorded yet (DESIGN.md 1a) — the measurement
// (1 x 12 200^2, 8 x 6 000^2, 100 x 3 000^2, 64 x 6 000^2 with MPCGPU_FB_COOP = 0 / 1 / 2 / 4 / 16) sets kFbCoopDefault to 1 or leaves it.
static const int kFbCoopDefault = 0;
static u32 fb_coop_waves(const mpcgpu_ctx *c, const StageAGeom &g, const RowBlockPlan &rp, u32 cnt)
{
	const int env = env_int("MPCGPU_FB_COOP", kFbCoopDefault);
	if (env <= 0) return 0;
	const u32 wmax = std::min<u32>(std::min<u32>(rp.occ * SA_WAVES, fb_coop_wave_limit((int)rp.long_h, g.mega)), 16u);
	u32 W;
	if (env >= 2) W = std::min<u32>((u32)env, wmax);
	else {
		const u64 resident = (u64)c->prop.multiProcessorCount * rp.occ * SA_WAVES;
		if (rp.nbmax < 2 || cnt >= resident) return 0;
		W = (u32)std::min<u64>(std::min<u32>(wmax, rp.nbmax), resident / cnt);
	}
	return W >= 2 ? W : 0;
}

static int launch_fb_row_block_pairs(mpcgpu_ctx *c, const StageAGeom &g, const FbParams &fp, const u32 *order, u32 cnt, u64 planes_budget, BatchPrep &P)
{
	RowBlockPlan rp;
	if (row_block_plan(c, g, cnt, planes_budget, rp)) return 1;
	const u32 W = fb_coop_waves(c, g, rp, cnt);
	P.coop_pairs = W ? cnt : 0; P.coop_waves = W;
	return W ? launch_fb_row_blocks_coop(c, g, rp, fp, order, cnt, W) : launch_fb_row_blocks(c, g, rp, fp, order, cnt);
}

// ---- forward/backward, one fb_kernel launch per rows-per-lane bin: `order` lists hcount[1] pairs of bin 1, then hcount[2] of bin 2, ...
// stage_a (batch = its pairs): persistent waves, exactly as many workgroups as the chip keeps resident (VGPR-limited), index arrays in device
// memory. align_pairs_small (batch = 0): a wave per pair, unclamped, index arrays in page-locked memory.
static int launch_fb_bins(mpcgpu_ctx *c, const StageAGeom &g, FbParams fp, const u32 *order, const u32 *hcount, u64 batch)
{
	TimedSpan sp;
	u32 pos = 0;
	for (u32 H = 1; H <= MPC_HMAX; ++H) {
		if (!hcount[H]) continue;
		const u32 cnt = hcount[H];
		u32 grid = (cnt + SA_WAVES - 1) / SA_WAVES, occ = 0;
		if (batch) {
			occ = (u32)occ_fb_h((int)H, g.mega, SA_BLOCK, g.fb_smem);
			grid = std::max(std::min<u32>(grid, (u32)c->prop.multiProcessorCount * occ), 1u);
		}
		const u64 fm_stride = (u64)(g.LYmax + 64) * H * 64;
		HIPCHK(c, c->d_fm.ensure((u64)grid * SA_WAVES * fm_stride * 4));
		if (trace_on()) {
			if (batch) fprintf(stderr, "[mpcgpu] fb H=%u pairs=%u grid=%u block=%d occ=%u capc=%u batch=%llu fm=%.1f MB\n", H, cnt, grid,
				SA_BLOCK, occ, g.capc, batch, (double)grid * SA_WAVES * fm_stride * 4 / 1048576.0);
			else fprintf(stderr, "[mpcgpu] align_pairs short list: fb H=%u pairs=%u\n", H, cnt);
			fflush(stderr);
		}
		fp.order = order + pos; fp.count = cnt;
		fp.queue = c->d_queue.as<u32>() + H;
		fp.fm_scratch = c->d_fm.as<float>(); fp.fm_stride = fm_stride;
		if (span_begin(c, 0, &sp)) return 1;
		launch_fb_h((int)H, g.mega, fp, grid, SA_BLOCK, g.fb_smem, c->stream);
		HIPCHK(c, hipGetLastError());
		if (span_end(c, &sp)) return 1;
		pos += cnt;
	}
	return 0;
}

// ---- forward/backward, the chains of a batch (kernels_fbc.h): one launch per bin; order, first, cnt: the batch's arrays on the device
// post: where a fused bin (plan.fuse) leaves records, sizes and flags; its waves' slots for lists beyond their LDS list are c->d_fuse_sort
static int launch_fb_chains(mpcgpu_ctx *c, const StageAGeom &g, const ChainPlan &plan, const FbParams &fp, const BatchPrep &P, const u32 *order, const u32 *first, const u32 *cnts, const FbChainPost &post)
{
	const u32 cus = (u32)c->prop.multiProcessorCount;
	TimedSpan sp;
	u32 cpos = 0;
	for (u32 H = 1; H <= MPC_HMAX; ++H) {
		if (!P.ccount[H]) continue;
		const u32 cnt = P.ccount[H];
		const bool fuse = plan.fuse[H];
		const size_t smem = fuse ? fuse_smem(plan, g, plan.fuse_sort_cap[H]) : plan.smem;
		const u32 occ = (u32)std::max(fuse ? occ_fbcp_h((int)H, SA_BLOCK, smem) : occ_fbc_h((int)H, plan.mega, SA_BLOCK, plan.smem), 1);
		const u32 grid = std::max(std::min<u32>((cnt + SA_WAVES - 1) / SA_WAVES, cus * occ), 1u);
		const u64 fm_stride = (u64)(P.cvmax[H] + 64) * H * 64;
		HIPCHK(c, c->d_fm.ensure((u64)grid * SA_WAVES * fm_stride * 4));
		if (trace_on()) {
			fprintf(stderr, "[mpcgpu] fb chains H=%u chains=%u grid=%u occ=%u longest axis=%u fm=%.1f MB\n", H, cnt, grid, occ, P.cvmax[H],
				(double)grid * SA_WAVES * fm_stride * 4 / 1048576.0);
			u64 members = 0;
			for (u32 k = 0; k < cnt; ++k) members += P.chain_cnt[cpos + k];
			fprintf(stderr, "[mpcgpu] fb chain members H=%u pairs=%llu capc=%u batch=%llu\n", H, members, g.capc, P.B);
			if (fuse) fprintf(stderr, "[mpcgpu] fb chain post: H=%u finishes its %llu pairs in the sweeps, list of %u candidates in LDS, lds=%zu B per workgroup\n", H, members, plan.fuse_sort_cap[H], smem);
			fflush(stderr);
		}
		FbChainParams cp;
		cp.f = fp;
		cp.f.order = order; cp.f.count = cnt;
		cp.f.queue = c->d_queue.as<u32>() + (MPC_HMAX + 2) + H;
		cp.f.fm_scratch = c->d_fm.as<float>(); cp.f.fm_stride = fm_stride;
		cp.chain_first = first + cpos; cp.chain_cnt = cnts + cpos;
		if (fuse) {
			FbChainPostParams fpp;
			fpp.c = cp; fpp.post = post;
			fpp.post.sort_cap = plan.fuse_sort_cap[H];
			fpp.post.wave_lds = (u32)(post_rows_fixed_lds(g) + 8 * (size_t)fpp.post.sort_cap);
			fpp.post.sort_stride = g.capc;
			HIPCHK(c, c->d_fuse_sort.ensure(g.capc > fpp.post.sort_cap ? (u64)grid * SA_WAVES * g.capc * 8 : 8));
			fpp.post.sort_scratch = c->d_fuse_sort.as<u64>();
			if (span_begin(c, 0, &sp)) return 1;
			launch_fbcp_h((int)H, fpp, grid, SA_BLOCK, smem, c->stream);
		} else {
			if (span_begin(c, 0, &sp)) return 1;
			launch_fbc_h((int)H, plan.mega, cp, grid, SA_BLOCK, plan.smem, c->stream);
		}
		HIPCHK(c, hipGetLastError());
		if (span_end(c, &sp)) return 1;
		cpos += cnt;
	}
	return 0;
}

// The sweeps of a batch: its index arrays go up (the NEXT set while the current batch is on the device), then row blocks, single pairs, chains.
// records = false (mpcgpu_ea_scores; never with fused bins): no room for records, sizes, EA and flags — the sweeps leave candidate lists only.
static int launch_fb_batch(mpcgpu_ctx *c, const StageAGeom &g, const ChainPlan &plan, u64 planes_budget, BatchPrep &P, bool into_next, bool records = true)
{
	DevBuf &dbx = into_next ? c->d_bx_n : c->d_bx, &dby = into_next ? c->d_by_n : c->d_by, &dord = into_next ? c->d_order_n : c->d_order;
	DevBuf &dcf = into_next ? c->d_chain_first_n : c->d_chain_first, &dcc = into_next ? c->d_chain_cnt_n : c->d_chain_cnt;
	// With fused bins the sweeps write records, sizes and flags: those of the next batch go to the second set (this batch's are still to be read)
	const bool alt = into_next && plan.fuse_any;
	DevBuf &dres = alt ? c->d_res_n : c->d_res, &dnnz = alt ? c->d_nnz_n : c->d_nnz, &dea = alt ? c->d_ea_n : c->d_ea, &dflags = alt ? c->d_flags_n : c->d_flags;
	const u64 B = P.B;
	if (upload(c, dbx, P.bx) || upload(c, dby, P.by) || upload(c, dord, P.order)) return 1;
	if (!P.chain_first.empty() && (upload(c, dcf, P.chain_first) || upload(c, dcc, P.chain_cnt))) return 1;
	if (plan.fuse_any && upload(c, into_next ? c->d_rest_n : c->d_rest, P.rest)) return 1;
	if (ensure_pair_scratch(c, g, B, records)) return 1;
	if (records) {
		HIPCHK(c, dres.ensure(B * g.res_stride() * 4));
		HIPCHK(c, dnnz.ensure(B * 4));
		HIPCHK(c, dea.ensure(B * 4));
		HIPCHK(c, dflags.ensure(B * 4));
	}
	FbChainPost post;
	post.lx_cap = g.LXmax + 2; post.ly_cap = g.LYmax + 2; post.sort_cap = 0; post.wave_lds = 0;
	post.batch = plan.post_batch; post.use_fma = c->use_fma;
	post.sort_scratch = nullptr; post.sort_stride = 0;
	post.res = dres.as<u32>(); post.res_stride = g.res_stride();
	post.nnz = dnnz.as<u32>(); post.ea = dea.as<float>(); post.flags = dflags.as<u32>();
	FbParams fp;
	fill_fb_params(c, fp, dbx.as<u32>(), dby.as<u32>(), g.capc, g.mega);
	P.coop_pairs = P.coop_waves = 0;
	if (P.hcount[MPC_HMAX + 1]) { // the order lists the row-block pairs last: bins ascend
		u32 first = 0;
		for (u32 H = 1; H <= MPC_HMAX; ++H) first += P.hcount[H];
		if (launch_fb_row_block_pairs(c, g, fp, dord.as<u32>() + first, P.hcount[MPC_HMAX + 1], planes_budget, P)) return 1;
	}
	return launch_fb_bins(c, g, fp, dord.as<u32>(), P.hcount, B) || launch_fb_chains(c, g, plan, fp, P, dord.as<u32>(), dcf.as<u32>(), dcc.as<u32>(), post);
}

// ---- the finishing kernels (probabilities, sort, EA, sparsify). Where a launch finds its pairs and candidate lists and leaves records, sizes
// and flags: the batch's device buffers (stage_a), page-locked memory for the outputs (align_pairs_small), buffers of its own (mpcgpu_post_scores)
struct PostIO { const u32 *pair_x, *pair_y, *seq_len; u64 *cand; const u32 *cand_cnt; u32 *res, *nnz; float *ea; u32 *flags; u32 count; const u32 *sel = nullptr; u32 nsel = 0; }; // sel: the nsel pairs (of count) to finish, NULL: all

// what mpcgpu_post_info reports: every finishing launch states its kernel (0 row-list, 1 sort, 2 wide), workgroup and pairs
static void post_info_set(mpcgpu_ctx *c, u32 kernel, u32 threads, u32 grid, u64 pairs) { c->pi_kernel = kernel; c->pi_threads = threads; c->pi_grid = grid; c->pi_pairs = pairs; }

// post_rows_kernel over io.count pairs that post_rows_fits(). sort_cap: entries of the LDS list of a pair's candidates; batch: cells of a row per
// EA pass (stage_a passes MPCGPU_POST_SORT_CAP and MPCGPU_POST_BATCH, the others ignore the knobs). grid = 0: a persistent grid, as many workgroups
// as are resident; else a workgroup per pair. scratch: a slot per workgroup for lists longer than sort_cap. timed = false: not in the launch counters.
static int launch_post_rows(mpcgpu_ctx *c, const StageAGeom &g, const PostIO &io, u32 sort_cap, u32 batch, u32 grid, DevBuf &scratch, bool timed)
{
	PostRowsParams pr;
	pr.pair_x = io.pair_x; pr.pair_y = io.pair_y; pr.seq_len = io.seq_len;
	pr.cand = io.cand; pr.capc = g.capc; pr.cand_cnt = io.cand_cnt;
	pr.use_fma = c->use_fma;
	pr.lx_cap = g.LXmax + 2; pr.ly_cap = g.LYmax + 2;
	pr.sort_cap = std::min<u32>(g.capc, sort_cap); pr.sort_stride = g.capc;
	pr.batch = std::min<u32>(std::max<u32>(batch, 1u), 64u);
	const size_t fixed_lds = ((((size_t)pr.lx_cap + 2 * (size_t)pr.ly_cap) * 4 + 7) & ~(size_t)7);
	if (fixed_lds + (size_t)pr.sort_cap * 8 > 150 * 1024) pr.sort_cap = (u32)((150 * 1024 - fixed_lds) / 8); // long sequences: the arrays per position come first
	const size_t smem = fixed_lds + (size_t)pr.sort_cap * 8;
	if (smem > 64 * 1024) HIPCHK(c, hipFuncSetAttribute((const void *)post_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
	if (!grid) {
		int pocc = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pocc, (const void *)post_rows_kernel, 64, smem) != hipSuccess || pocc < 1) pocc = 1;
		// The persistent grid must not be larger than what is really resident, or its last workgroups run as a second round
		// (measured, per batch of 125 000 pairs: 15 248 B of LDS, 10 workgroups per CU reported: 12.7 ms; 15 760 B, still 10
		// reported: 22.5 ms; 17 296 B, 9 reported: 14.1 ms — 64-thread workgroups stop fitting at ~152 KB per CU, not 160)
		pocc = std::max(1, std::min(pocc, (int)((152 * 1024) / smem)));
		// (behind fused sweeps the launch finishes what they left, which may be nothing: it stays, as the place in the stream the sizes wait for)
		grid = (u32)std::max<u64>(std::min<u64>(io.sel ? io.nsel : io.count, (u64)c->prop.multiProcessorCount * (u32)pocc), 1);
		if (trace_on()) { fprintf(stderr, "[mpcgpu] post rows: list of %u candidates in LDS, lds=%zu B blocks/CU=%d grid=%u\n", pr.sort_cap, smem, pocc, grid); fflush(stderr); }
	}
	HIPCHK(c, scratch.ensure(g.capc > pr.sort_cap ? (u64)grid * pr.sort_stride * 8 : 8));
	pr.sort_scratch = scratch.as<u64>();
	pr.res = io.res; pr.res_stride = g.res_stride();
	pr.nnz = io.nnz; pr.ea = io.ea; pr.flags = io.flags;
	pr.count = io.sel ? io.nsel : io.count; pr.long_min = g.long_min; pr.sel = io.sel;
	post_info_set(c, 0, 64, grid, pr.count);
	TimedSpan sp;
	if (timed && span_begin(c, 1, &sp)) return 1;
	MPC_LAUNCH(post_rows_kernel, grid, 64, smem, c->stream, pr);
	HIPCHK(c, hipGetLastError());
	return timed ? span_end(c, &sp) : 0;
}

// PostParams of post_kernel (the general finishing kernel) but for its two per-workgroup scratch buffers; returns the dynamic LDS. sort_cap: LDS
// sort buffer capacity (entries, rounded up to a power of two): pairs with more candidates sort in the global scratch. The kernel is
// latency-bound (one wave per pair), so LDS per workgroup trades against resident waves.
static size_t fill_post(const mpcgpu_ctx *c, const StageAGeom &g, const PostIO &io, u32 sort_cap, PostParams &pp)
{
	pp.pair_x = io.pair_x; pp.pair_y = io.pair_y; pp.seq_len = io.seq_len;
	pp.cand = io.cand; pp.capc = g.capc; pp.cand_cnt = io.cand_cnt;
	pp.use_fma = c->use_fma;
	pp.sort_stride = next_pow2(std::max<u32>(g.capc, 2));
	pp.sort_cap = std::min<u32>((u32)pp.sort_stride, next_pow2(sort_cap));
	pp.srow_cap = std::min<u32>(g.LYmax + 1, 2048u);
	pp.srow_stride = 2 * ((u64)g.LYmax + 1);
	pp.res = io.res; pp.res_stride = g.res_stride();
	pp.nnz = io.nnz; pp.ea = io.ea; pp.flags = io.flags;
	pp.count = io.count; pp.long_min = g.long_min;
	return (size_t)pp.sort_cap * 8 + (size_t)pp.srow_cap * 2 * 4;
}

// MPCGPU_POST_WIDE: 0 = never post_wide_kernel, 1 = always (also lists that fit the row-list kernel), unset = the rule: a batch that
// post_rows_fits() rejects goes to the wide kernel when kPostWideDefault says so. The rule may choose the wide kernel only where it
// has been MEASURED no slower than post_kernel on each of 1 x 12 200^2, 300 x 20 000, 300 x 60 000, 6 000 x 60 000, 64 x 13 000^2
// (DESIGN.md 1a). Measured so far: 70 against 342 ms, 13 against 150 ms and 89 against 413 ms of finishing time for the first, second
// and last; the two widest have no figure for post_kernel yet, so the default stays post_kernel and the wide kernel is opt-in.
static const int kPostWideDefault = 0;
static int post_wide_env() { return env_int("MPCGPU_POST_WIDE", -1); }

// post_wide_kernel (kernels_postw.h) over io.count pairs: a workgroup of MPC_POSTW_THREADS per pair. grid = 0: a persistent grid, as
// many workgroups as are resident. Per workgroup, in context-owned buffers: two key slots of capc entries (lists beyond the LDS
// buffers), LXmax + 1 row starts, two DP rows of LYmax + 1 floats (pairs wider than the LDS rows), one word for mpcgpu_post_info.
// MPCGPU_POSTW_LDS (tests): entries sorted in LDS and floats of an LDS DP row at most; 0 = everything through the global slots.
static int launch_post_wide(mpcgpu_ctx *c, const StageAGeom &g, const PostIO &io, u32 grid, bool timed)
{
	const u32 T = MPC_POSTW_THREADS;
	const int lds_env = env_int("MPCGPU_POSTW_LDS", -1);
	PostWideParams pw;
	pw.pair_x = io.pair_x; pw.pair_y = io.pair_y; pw.seq_len = io.seq_len;
	pw.cand = io.cand; pw.capc = g.capc; pw.cand_cnt = io.cand_cnt;
	pw.use_fma = c->use_fma;
	// 4096 entries in each of the two key buffers (64 KB) and 4096 floats in each DP row (32 KB) beside 41 KB of tables: 137 KB, one
	// workgroup of 16 waves per CU either way
	pw.lds_cap = std::min<u32>(g.capc, lds_env >= 0 ? std::min<u32>((u32)lds_env, 4096u) : 4096u);
	pw.srow_cap = std::min<u32>(g.LYmax + 1, lds_env >= 0 ? std::min<u32>((u32)lds_env, 4096u) : 4096u);
	const size_t smem = mpc_postw_smem(T, pw.lds_cap, pw.srow_cap);
	ensure_dyn_smem((const void *)post_wide_kernel, smem);
	if (!grid) {
		int pocc = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pocc, (const void *)post_wide_kernel, (int)T, smem) != hipSuccess || pocc < 1) pocc = 1;
		grid = (u32)std::min<u64>(io.count, (u64)c->prop.multiProcessorCount * (u32)pocc);
	}
	pw.key_stride = g.capc; pw.rs_stride = (u64)g.LXmax + 1; pw.srow_stride = 2 * ((u64)g.LYmax + 1);
	HIPCHK(c, c->d_sort_scratch.ensure(g.capc > pw.lds_cap ? (u64)grid * 2 * pw.key_stride * 8 : 8));
	HIPCHK(c, c->d_pw_rs.ensure((u64)grid * pw.rs_stride * 4));
	HIPCHK(c, c->d_srow_scratch.ensure(g.LYmax + 1 > pw.srow_cap ? (u64)grid * pw.srow_stride * 4 : 8));
	HIPCHK(c, c->d_pw_info.ensure((u64)grid * 8));
	pw.key_scratch = c->d_sort_scratch.as<u64>(); pw.rs_scratch = c->d_pw_rs.as<u32>(); pw.srow_scratch = c->d_srow_scratch.as<float>();
	pw.info = c->d_pw_info.as<u64>();
	pw.res = io.res; pw.res_stride = g.res_stride();
	pw.nnz = io.nnz; pw.ea = io.ea; pw.flags = io.flags;
	pw.count = io.count; pw.long_min = g.long_min;
	if (trace_on()) { fprintf(stderr, "[mpcgpu] post wide: %u threads per pair, lists of %u candidates and rows of %u floats in LDS, lds=%zu B grid=%u\n", T, pw.lds_cap, pw.srow_cap, smem, grid); fflush(stderr); }
	post_info_set(c, 2, T, grid, io.count);
	TimedSpan sp;
	if (timed && span_begin(c, 1, &sp)) return 1;
	MPC_LAUNCH(post_wide_kernel, grid, T, smem, c->stream, pw);
	HIPCHK(c, hipGetLastError());
	return timed ? span_end(c, &sp) : 0;
}

// The finishing kernel of the current batch (its index arrays are the current set: c->d_bx, c->d_by), and the event its sizes wait for.
// rest: with fused bins (ChainPlan::fuse_any), the pairs the sweeps left (c->d_rest); NULL: every pair of the batch
static int launch_post_batch(mpcgpu_ctx *c, const StageAGeom &g, bool post_rows, bool post_wide, u32 sort_cap, u64 B, const std::vector<u32> *rest)
{
	PostIO io = {c->d_bx.as<u32>(), c->d_by.as<u32>(), c->d_seq_len.as<u32>(), c->d_cand.as<u64>(), c->d_cand_cnt.as<u32>(), c->d_res.as<u32>(), c->d_nnz.as<u32>(), c->d_ea.as<float>(), c->d_flags.as<u32>(), (u32)B};
	if (rest) { io.sel = c->d_rest.as<u32>(); io.nsel = (u32)rest->size(); }
	if (post_rows) {
		if (launch_post_rows(c, g, io, sort_cap, (u32)std::max(env_int("MPCGPU_POST_BATCH", 64), 1), 0, c->d_sort_scratch, true)) return 1;
	} else if (post_wide) {
		if (launch_post_wide(c, g, io, 0, true)) return 1;
	} else {
		PostParams pp;
		const size_t psmem = fill_post(c, g, io, sort_cap, pp);
		ensure_dyn_smem((const void *)post_kernel, psmem); // (beyond 64 KB only under a MPCGPU_POST_SORT_CAP of more than 4096 entries)
		int pocc = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pocc, (const void *)post_kernel, 64, psmem) != hipSuccess || pocc < 1) pocc = 8;
		if (psmem) pocc = std::max(1, std::min(pocc, (int)((152 * 1024) / psmem))); // as for post_rows_kernel above
		const u32 pgrid = (u32)std::min<u64>(B, (u64)c->prop.multiProcessorCount * (u32)pocc);
		if (trace_on()) { fprintf(stderr, "[mpcgpu] post: sort_cap=%u lds=%zu B blocks/CU=%d grid=%u\n", pp.sort_cap, psmem, pocc, pgrid); fflush(stderr); }
		HIPCHK(c, c->d_sort_scratch.ensure(pp.sort_stride > pp.sort_cap ? (u64)pgrid * pp.sort_stride * 8 : 8));
		HIPCHK(c, c->d_srow_scratch.ensure(g.LYmax + 1 > pp.srow_cap ? (u64)pgrid * pp.srow_stride * 4 : 8));
		pp.sort_scratch = c->d_sort_scratch.as<u64>(); pp.srow_scratch = c->d_srow_scratch.as<float>();
		post_info_set(c, 1, 64, pgrid, B);
		TimedSpan sp;
		if (span_begin(c, 1, &sp)) return 1;
		MPC_LAUNCH(post_kernel, pgrid, 64, psmem, c->stream, pp);
		HIPCHK(c, hipGetLastError());
		if (span_end(c, &sp)) return 1;
	}
	HIPCHK(c, hipEventRecord(c->ev_post, c->stream));
	return 0;
}

// Sizes, EA and flags of the batch at pair `done`, back on the second stream (behind this batch's finishing kernel, beside the next batch's sweeps)
static int read_batch_sizes(mpcgpu_ctx *c, u64 done, u64 B, bool *overflow)
{
	std::vector<u32> &flags = c->v_flags; // (kept: see mpcgpu_ctx)
	flags.resize(B);
	HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_post, 0));
	HIPCHK(c, hipMemcpyAsync(&c->sh_nnz[done], c->d_nnz.p, B * 4, hipMemcpyDeviceToHost, c->stream2));
	HIPCHK(c, hipMemcpyAsync(&c->sh_ea[done], c->d_ea.p, B * 4, hipMemcpyDeviceToHost, c->stream2));
	HIPCHK(c, hipMemcpyAsync(flags.data(), c->d_flags.p, B * 4, hipMemcpyDeviceToHost, c->stream2));
	HIPCHK(c, hipStreamSynchronize(c->stream2));
	*overflow = false;
	for (u64 q = 0; q < B; ++q) *overflow = *overflow || (flags[q] & 1u);
	return 0;
}

// The records of batch P (pairs [done, done + P.B) of np) go behind the *words record words already in the shard; *words moves on.
static int pack_batch(mpcgpu_ctx *c, const StageAGeom &g, const BatchPrep &P, u64 done, u64 np, u64 hdr, u64 *words)
{
	const u64 B = P.B;
	std::vector<u64> &dstbase = c->v_dstbase, &recw = c->v_recw; // (kept: see mpcgpu_ctx)
	dstbase.resize(B); recw.resize(B);
	u64 w = *words;
	for (u64 q = 0; q < B; ++q) {
		recw[q] = rec_words(c->len[P.bx[q]], c->len[P.by[q]], c->sh_nnz[done + q]);
		dstbase[q] = hdr / 4 + w;
		w += recw[q];
	}
	// capacity estimate for the whole shard from the words seen so far
	const double per = double(w) / double(done + B);
	const u64 est = hdr + (u64)(per * 1.05 * double(np) + 1024) * 4;
	// (allocated with room to spare, asked for with less: the estimate moves by a fraction of a percent from batch to batch, and a
	// buffer that is a hair too small is replaced — a device-to-device copy of gigabytes behind the next batch's sweeps, once per
	// cold run: profiles/r13a_kernel_stats_1000x400.csv has 0.39 s of such copies in the first step of a process)
	if (std::max<u64>(est, hdr + w * 4) > c->d_shard.cap) {
		const size_t cap0 = c->d_shard.cap;
		HIPCHK(c, c->d_shard.ensure(std::max<u64>(hdr + (u64)(per * 1.15 * double(np) + 1024) * 4, hdr + w * 4), true, c->stream));
		if (trace_on()) {
			fprintf(stderr, "[mpcgpu] stage A shard: buffer %s at pair %llu, %zu -> %zu B, %llu record words kept\n", cap0 ? "replaced" : "allocated", done, cap0, c->d_shard.cap, *words);
			fflush(stderr);
		}
	}
	if (upload(c, c->d_dstbase, dstbase) || upload(c, c->d_recwords, recw)) return 1;
	TimedSpan sp;
	if (span_begin(c, 1, &sp)) return 1;
	MPC_LAUNCH(pack_kernel, (u32)std::min<u64>(B, (u64)c->prop.multiProcessorCount * 8), 256, 0, c->stream, c->d_res.as<u32>(), g.res_stride(),
		c->d_dstbase.as<u64>(), c->d_recwords.as<u64>(), c->d_shard.as<u32>(), (u32)B);
	HIPCHK(c, hipGetLastError());
	if (span_end(c, &sp)) return 1;
	*words = w;
	return 0;
}

// Stage A over an explicit list of (x,y) sequence-index pairs (host arrays of np entries): the packed
// shard of those pairs, in list order, ends up in c->d_shard with sh_nnz / sh_ea.
static int stage_a(mpcgpu_ctx *c, u64 np, const u32 *px, const u32 *py)
{
	HIPCHK(c, hipSetDevice(c->device));
	c->have_shard = c->have_store = false;
	c->shard_is_list = true; c->se.last = false;
	c->list_x.assign(px, px + np); c->list_y.assign(py, py + np); // mpcgpu_get_list_sparse
	c->list_q0 = 0;
	if (!c->ap_keep) { c->ap_x.clear(); c->ap_y.clear(); }
	c->sh_k0 = 0; c->sh_k1 = np;
	c->sh_nnz.assign(np, 0);
	c->sh_ea.assign(np, 0.0f);
	StageAGeom g = stage_a_geom(c, np, px, py);
	c->work_cells = g.work_cells;
	c->sa_pairs = np; c->sa_chained = c->sa_chains = 0; c->sa_chain_bins = 0;
	c->sa_coop_pairs = 0; c->sa_coop_waves = 0;
	const u64 hdr = shard_header_bytes(np);
	if (np == 0) {
		HIPCHK(c, c->d_shard.ensure(hdr));
		u64 h2[2] = {0, 0};
		HIPCHK(c, hipMemcpyAsync(c->d_shard.p, h2, 16, hipMemcpyHostToDevice, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
		c->shard_bytes = hdr;
		c->have_shard = true;
		return 0;
	}
	for (u64 k = 0; k < np; ++k) // calcposteriorflat.cpp:54-61, per pair (a registry holds sequences that never meet)
		if (double(c->len[px[k]]) * double(c->len[py[k]]) * 5 + 100 > double(INT_MAX))
			return fail(c, "mpcgpu_calc_posteriors: HMM overflow, sequence lengths %u, %u (max ~21k)", c->len[px[k]], c->len[py[k]]);
	if (g.LXlong > MPC_KEY_COL_MASK_LONG || g.LYlong > MPC_KEY_COL_MASK_LONG)
		return fail(c, "mpcgpu_calc_posteriors: a pair of %u x %u positions is beyond this build's limit of %u per sequence "
			"once the row sequence is longer than %u", g.LXlong, g.LYlong, MPC_KEY_COL_MASK_LONG, g.long_min - 1);
	const ScratchBudget budget = scratch_budget();
	ChainPlan chain;
	if (chain_plan(c, g, budget.planes, chain)) return 1;
	c->sa_fused = 0; c->sa_fuse_bins = 0;
	// the row-list finishing kernel when the list fits it; MPCGPU_POST=sort forces the general one
	const char *post_mode = getenv("MPCGPU_POST");
	// LDS list of a pair's candidates (larger lists cost resident waves, pairs that exceed it sort through HBM scratch; per
	// batch of 125 000 pairs at L~400: 512 entries 16.9 ms, 768: 12.3, 896: 11.9, 1024: 11.7, 1280: 12.7, 1408 (holds every
	// pair): 14.0, 1664: 15.8)
	const u32 sort_cap = (u32)std::max(env_int("MPCGPU_POST_SORT_CAP", 1024), 2);
	const bool post_sort = post_mode && !strcmp(post_mode, "sort");
	const int wide_env = post_wide_env();
	const bool fits = post_rows_fits(g.LXmax, g.LYmax, sort_cap);
	const bool post_rows = wide_env != 1 && !post_sort && fits;
	// the wide kernel: forced (MPCGPU_POST_WIDE=1, whatever else is set), or by the rule for a batch that does not FIT the row-list
	// kernel (MPCGPU_POST=sort keeps asking for post_kernel)
	const bool post_wide = wide_env == 1 || (wide_env < 0 && kPostWideDefault && !post_sort && !fits);
	if (fuse_plan(c, g, np, budget.batch, post_rows, sort_cap, chain)) return 1;
	const bool host_trace = trace_host(); // diagnostics: host wall time between the device phases of a batch
	auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	double lap_t[6] = {0, 0, 0, 0, 0, 0}, t_prev = host_trace ? now() : 0.0;
	auto lap = [&](int k) { if (host_trace) { const double t = now(); lap_t[k] += t - t_prev; t_prev = t; } };

	// ---- the batches as a PIPELINE (round 6). Rounds 1-5 ran a batch to its end — forward/backward, finishing kernel, sizes back to the
	// host, pack — before the next batch's sweeps were queued: a few ms of idle device per batch boundary. Measured gain on one GPU:
	// 1458.5 -> 1456.0 ms per step (profiles/r12i: two runs each on one box) — the boundaries were smaller than they looked (most of the
	// 22 ms between a step's wall time and its kernels is the relax's tile cutter, not stage A). Now the sweeps of batch b + 1 are queued BEHIND the finishing kernel of batch b, before the host
	// asks for b's sizes; those come back on a second stream (after an event that follows the finishing kernel), the host sizes the
	// records while the device sweeps, and the pack of b is queued behind the sweeps of b + 1, before the finishing kernel of b + 1
	// (which overwrites the records the pack reads). One stream carries the kernels, in the order
	//     fb(0) post(0) | fb(1) pack(0) post(1) | fb(2) pack(1) post(2) | ... | pack(last)
	// and no buffer is doubled except the per-batch index arrays (pairs, launch order, chains: a few MB).
	if (!c->stream2) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
	if (!c->ev_post) HIPCHK(c, hipEventCreateWithFlags(&c->ev_post, hipEventDisableTiming));
	BatchPrep cur, nxt;
	u64 words_done = 0, done = 0; // record words packed so far, pairs done
	if (prepare_batch(c, g, chain, budget.batch, np, px, py, 0, cur) || launch_fb_batch(c, g, chain, budget.planes, cur, false)) return 1;
	lap(0);
	while (done < np) {
		const u64 B = cur.B;
		if (launch_post_batch(c, g, post_rows, post_wide, sort_cap, B, chain.fuse_any ? &cur.rest : nullptr)) return 1;
		lap(1);
		// ---- the next batch: prepared on the host and its sweeps queued while the device runs this one
		nxt.valid = false;
		if (done + B < np && (prepare_batch(c, g, chain, budget.batch, np, px, py, done + B, nxt) || launch_fb_batch(c, g, chain, budget.planes, nxt, true))) return 1;
		lap(2);
		// ---- sizes back, overflow check, pack
		bool overflow = false;
		if (read_batch_sizes(c, done, B, &overflow)) return 1;
		lap(3);
		if (overflow) {
			const u64 room = (u64)g.LXmax * g.LYmax;
			if (g.capc >= room) return fail(c, "mpcgpu_calc_posteriors: candidate overflow at full capacity (internal error)");
			if (trace_on()) {
				fprintf(stderr, "[mpcgpu] stage A overflow: batch at pair %llu (%llu pairs) redone, capc %u -> %llu, next batch %s\n", done, B, g.capc,
					std::min<u64>((u64)g.capc * 2, room), nxt.valid ? "queued and dropped" : "not queued");
				fflush(stderr);
			}
			g.capc = (u32)std::min<u64>((u64)g.capc * 2, room);
			// redo this batch with a larger candidate capacity: what is queued behind it (the next batch's sweeps) is drained and dropped
			HIPCHK(c, hipStreamSynchronize(c->stream));
			if (prepare_batch(c, g, chain, budget.batch, np, px, py, done, cur) || launch_fb_batch(c, g, chain, budget.planes, cur, false)) return 1;
			continue;
		}
		if (pack_batch(c, g, cur, done, np, hdr, &words_done)) return 1;
		// what the LAST batch left in the scratch buffers (mpcgpu_align_pairs reads the candidate lists of a one-batch stage)
		c->sa_b0 = done; c->sa_B = B; c->sa_capc = g.capc; c->sa_post_rows = post_rows; c->sa_long_min = g.long_min;
		done += B;
		for (u32 c2 : cur.chain_cnt) if (c2 >= 2) { c->sa_chains += 1; c->sa_chained += c2; }
		c->sa_fused += cur.fused;
		for (u32 H = 1; H <= MPC_HMAX; ++H) if (chain.fuse[H] && cur.ccount[H]) c->sa_fuse_bins |= 1u << H;
		for (u32 H = 1; H <= MPC_HMAX; ++H) if (cur.ccount[H]) c->sa_chain_bins |= 1u << H;
		if (cur.coop_pairs) { c->sa_coop_pairs += cur.coop_pairs; c->sa_coop_waves = cur.coop_waves; }
		std::swap(cur, nxt);
		if (cur.valid) { // the next batch's index arrays become the current set
			std::swap(c->d_bx, c->d_bx_n); std::swap(c->d_by, c->d_by_n); std::swap(c->d_order, c->d_order_n);
			std::swap(c->d_chain_first, c->d_chain_first_n); std::swap(c->d_chain_cnt, c->d_chain_cnt_n);
			if (chain.fuse_any) {
				std::swap(c->d_rest, c->d_rest_n); std::swap(c->d_res, c->d_res_n);
				std::swap(c->d_nnz, c->d_nnz_n); std::swap(c->d_ea, c->d_ea_n); std::swap(c->d_flags, c->d_flags_n);
			}
		}
		lap(4);
	}
	HIPCHK(c, hipStreamSynchronize(c->stream)); // the last pack
	if (host_trace)
		fprintf(stderr, "[mpcgpu] stage A host seconds: prepare (first batch / retries) %.4f, uploads + launches %.4f, next batch prepared %.4f, "
			"waiting for the device %.4f, sizes -> pack -> wait %.4f\n", lap_t[0], lap_t[1], lap_t[2], lap_t[3], lap_t[4]);
	// header
	std::vector<u8> &h = c->v_shdr; // (kept: see mpcgpu_ctx)
	h.assign(hdr, 0);
	u64 h2[2] = {np, words_done};
	memcpy(h.data(), h2, 16);
	memcpy(h.data() + 16, c->sh_nnz.data(), np * 4);
	memcpy(h.data() + 16 + np * 4, c->sh_ea.data(), np * 4);
	HIPCHK(c, hipMemcpyAsync(c->d_shard.p, h.data(), hdr, hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->shard_bytes = hdr + words_done * 4;
	c->have_shard = true;
	return 0;
}

int mpcgpu_calc_posteriors(mpcgpu_ctx *c, uint64_t k0, uint64_t k1)
{
	if (!c) return 1;
	if (c->n == 0) return fail(c, "mpcgpu_calc_posteriors: call mpcgpu_set_seqs first");
	if (k0 > k1 || k1 > c->npairs) return fail(c, "mpcgpu_calc_posteriors: bad pair range [%llu,%llu)", (u64)k0, (u64)k1);
	++c->epoch;
	const int rc = stage_a(c, k1 - k0, c->h_pair_x.data() + k0, c->h_pair_y.data() + k0);
	c->shard_is_list = false;
	c->sh_k0 = k0; c->sh_k1 = k1;
	return rc;
}

// mpcgpu_upgma.inc — host side of kernels_upgma.h: mpcgpu_upgma, mpcgpu_sw_tree, mpcgpu_upgma_info, mpcgpu_upgma_scale. Included by mpcgpu.cpp
// inside its extern "C" block. Everything here lives in buffers of its own (mpcgpu_ctx::up; mpcgpu_sw_tree also uses mpcgpu_ctx::sw as
// mpcgpu_sw_scores does): shard, store and stage-A scratch of the context are neither read nor written, and the store epoch stays where it is.

extern "C++" {
namespace {

// refusals shared by both entries; `who` names the entry
int upgma_check(mpcgpu_ctx *c, const char *who, u64 n, int transform, int linkage)
{
	if (n < 2) return fail(c, "%s: %llu leaves, a tree needs 2", who, (unsigned long long)n);
	if (n > MPC_UPGMA_NMAX) return fail(c, "%s: %llu leaves, more than %u (upgma5.h:68: the reference's 32-bit triangle subscript wraps)", who, (unsigned long long)n, MPC_UPGMA_NMAX);
	if (transform < MPC_UPGMA_T_NONE || transform > MPC_UPGMA_T_EA) return fail(c, "%s: unknown transform %d", who, transform);
	if (linkage < MPC_UPGMA_L_AVG || linkage > MPC_UPGMA_L_BIASED) return fail(c, "%s: unknown linkage %d", who, linkage);
	return 0;
}

// room for the triangle of n leaves (a query, no allocation). MPCGPU_UPGMA_MEM_MB: the device memory to count on, for tests.
int upgma_check_room(mpcgpu_ctx *c, const char *who, u32 n)
{
	const u64 need = (u64)n * (n - 1) / 2 * sizeof(float) + 24ull * n + ((u64)64 << 20);
	HIPCHK(c, hipSetDevice(c->device));
	size_t freeb = 0, totb = 0;
	HIPCHK(c, hipMemGetInfo(&freeb, &totb));
	u64 have = (u64)freeb + c->up.d_tri.cap;
	const int cap_mb = env_int("MPCGPU_UPGMA_MEM_MB", 0);
	if (cap_mb > 0) have = std::min<u64>(have, (u64)cap_mb << 20);
	if (need > have)
		return fail(c, "%s: the triangle of %u leaves needs %llu MB of device memory, %llu MB are free", who, n, (unsigned long long)(need >> 20), (unsigned long long)(have >> 20));
	return 0;
}

int upgma_alloc(mpcgpu_ctx *c, u32 n)
{
	mpcgpu_ctx::UpgmaState &u = c->up;
	const u64 m = (u64)n * (n - 1) / 2;
	if (u.d_tri.cap < m * sizeof(float)) u.d_tri.release(); // never two triangles at once
	HIPCHK(c, u.d_tri.ensure(m * sizeof(float)));
	HIPCHK(c, u.d_row.ensure((size_t)n * 3 * sizeof(u32)));
	HIPCHK(c, u.d_out.ensure((size_t)(n - 1) * 5 * sizeof(u32)));
	HIPCHK(c, u.d_stat.ensure(4 * sizeof(u32)));
	return 0;
}

// the triangle is in c->up.d_tri (work queued on c->stream): transform, initialisation, join loop, the four arrays back
int upgma_run(mpcgpu_ctx *c, const char *who, u32 n, int transform, int linkage, uint32_t *left, uint32_t *right, float *left_len, float *right_len)
{
	mpcgpu_ctx::UpgmaState &u = c->up;
	const u64 m = (u64)n * (n - 1) / 2;
	const u32 cus = (u32)std::max(1, c->prop.multiProcessorCount);
	float *tri = u.d_tri.as<float>();
	float *mn = u.d_row.as<float>();
	u32 *nn = u.d_row.as<u32>() + n, *node = u.d_row.as<u32>() + 2 * (size_t)n;
	u32 *d_left = u.d_out.as<u32>(), *d_right = d_left + (n - 1);
	float *d_llen = (float *)(d_right + (n - 1)), *d_rlen = d_llen + (n - 1), *d_height = d_rlen + (n - 1);
	float *stat = u.d_stat.as<float>();
	u32 *status = u.d_stat.as<u32>() + 2;
	HIPCHK(c, hipMemsetAsync(u.d_stat.p, 0, 4 * sizeof(u32), c->stream));
	const u32 grid = (u32)std::max<u64>(1, std::min<u64>((m + 255) / 256, (u64)cus * 8));
	const bool scale = transform == MPC_UPGMA_T_SCALE_SIM || transform == MPC_UPGMA_T_SCALE_DIST;
	if (scale) HIPCHK(c, u.d_partial.ensure((size_t)grid * 2 * sizeof(float)));
	hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
	HIPCHK(c, hipEventCreate(&e0));
	HIPCHK(c, hipEventCreate(&e1));
	HIPCHK(c, hipEventCreate(&e2));
	HIPCHK(c, hipEventRecord(e0, c->stream));
	const size_t fold_smem = 2 * 4 * sizeof(float);
	if (scale) {
		MPC_LAUNCH(upgma_minmax_kernel, grid, 256, fold_smem, c->stream, (const float *)tri, m, u.d_partial.as<float>());
		HIPCHK(c, hipGetLastError());
	}
	MPC_LAUNCH(upgma_transform_kernel, grid, 256, fold_smem, c->stream, tri, m, transform, (const float *)u.d_partial.as<float>(), grid, stat, status);
	HIPCHK(c, hipGetLastError());
	MPC_LAUNCH(upgma_init_kernel, std::min<u32>((n + 3) / 4, cus * 8), 256, 0, c->stream, (const float *)tri, n, mn, nn, node);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(e1, c->stream));
	const u32 cut = (u32)std::min<long long>(MPC_UPGMA_LDS_ROWS_MAX, std::max(0, env_int("MPCGPU_UPGMA_LDS_ROWS", (int)MPC_UPGMA_LDS_ROWS_MAX)));
	const bool lds = n <= cut;
	UpgmaJoinParams p;
	p.tri = tri; p.n = n; p.linkage = linkage; p.mn = mn; p.nn = nn; p.node = node; p.height = d_height;
	p.left = d_left; p.right = d_right; p.llen = d_llen; p.rlen = d_rlen; p.status = status;
	if (lds) {
		const size_t smem = MPC_UPGMA_SCRATCH_BYTES + (size_t)n * 12;
		auto kern = upgma_join_kernel<true>;
		ensure_dyn_smem((const void *)kern, smem);
		MPC_LAUNCH(kern, 1, MPC_UPGMA_THREADS, smem, c->stream, p);
	} else {
		auto kern = upgma_join_kernel<false>;
		MPC_LAUNCH(kern, 1, MPC_UPGMA_THREADS, (size_t)MPC_UPGMA_SCRATCH_BYTES, c->stream, p);
	}
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(e2, c->stream));
	u32 h_stat[4] = {0, 0, 0, 0};
	HIPCHK(c, hipMemcpyAsync(h_stat, u.d_stat.p, sizeof(h_stat), hipMemcpyDeviceToHost, c->stream));
	std::vector<u32> out((size_t)(n - 1) * 4);
	HIPCHK(c, hipMemcpyAsync(out.data(), u.d_out.p, out.size() * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	float ms_prep = 0, ms_join = 0;
	HIPCHK(c, hipEventElapsedTime(&ms_prep, e0, e1));
	HIPCHK(c, hipEventElapsedTime(&ms_join, e1, e2));
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(e2);
	u.n = n; u.lds = lds ? 1 : 0; u.ms_prep += ms_prep; u.ms_join = ms_join;
	u.scaled = scale;
	memcpy(&u.smin, &h_stat[0], 4);
	memcpy(&u.smax, &h_stat[1], 4);
	if (trace_on()) {
		fprintf(stderr, "[mpcgpu] upgma: %u leaves, row state in %s, transform + init %.3f ms, joins %.3f ms\n", n, lds ? "LDS" : "global memory", u.ms_prep, ms_join);
		fflush(stderr);
	}
	if (h_stat[2] & MPC_UPGMA_ST_EA_RANGE) return fail(c, "%s: an EA value outside 0 .. 1 (upgma5.cpp:512)", who);
	if (h_stat[2] & MPC_UPGMA_ST_NO_MIN)
		return fail(c, "%s: no distance below FLT_MAX is left at join %u of %u (upgma5.cpp:197-199)", who, h_stat[2] & 0xffffffu, n - 1);
	const size_t k = n - 1;
	memcpy(left, out.data(), k * 4);
	memcpy(right, out.data() + k, k * 4);
	memcpy(left_len, out.data() + 2 * k, k * 4);
	memcpy(right_len, out.data() + 3 * k, k * 4);
	return 0;
}

} // namespace
} // extern "C++"

int mpcgpu_upgma(mpcgpu_ctx *c, uint32_t n, const float *dist, int transform, int linkage, uint32_t *left, uint32_t *right, float *left_len, float *right_len)
{
	if (!c) return 1;
	if (!dist || !left || !right || !left_len || !right_len) return fail(c, "mpcgpu_upgma: NULL argument");
	if (upgma_check(c, "mpcgpu_upgma", n, transform, linkage)) return 1;
	if (upgma_check_room(c, "mpcgpu_upgma", n)) return 1;
	if (upgma_alloc(c, n)) return 1;
	const u64 m = (u64)n * (n - 1) / 2;
	c->up.ms_prep = 0;
	HIPCHK(c, hipMemcpyAsync(c->up.d_tri.p, dist, m * sizeof(float), hipMemcpyHostToDevice, c->stream));
	return upgma_run(c, "mpcgpu_upgma", n, transform, linkage, left, right, left_len, right_len);
}

int mpcgpu_sw_tree(mpcgpu_ctx *c, int linkage, uint32_t *left, uint32_t *right, float *left_len, float *right_len, float *scores)
{
	if (!c) return 1;
	if (!left || !right || !left_len || !right_len) return fail(c, "mpcgpu_sw_tree: NULL argument");
	if (!c->sw.have) return fail(c, "mpcgpu_sw_tree: call mpcgpu_sw_set_scores first");
	if (c->n == 0) return fail(c, "mpcgpu_sw_tree: call mpcgpu_set_seqs / mpcgpu_set_seqs_registry first");
	if (upgma_check(c, "mpcgpu_sw_tree", c->n, MPC_UPGMA_T_SCALE_SIM, linkage)) return 1;
	for (u32 i = 0; i < c->n; ++i)
		if (c->len[i] > 65535u) return fail(c, "mpcgpu_sw_tree: sequence %u has %u positions, more than 65535", i, c->len[i]);
	if (upgma_check_room(c, "mpcgpu_sw_tree", c->n)) return 1;
	const u32 n = c->n;
	if (upgma_alloc(c, n)) return 1;
	const u64 m = (u64)n * (n - 1) / 2;
	if (sw_scores_run(c, m, nullptr, nullptr, scores, c->up.d_tri.as<float>())) return 1;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	HIPCHK(c, hipEventCreate(&e0));
	HIPCHK(c, hipEventCreate(&e1));
	HIPCHK(c, hipEventRecord(e0, c->stream));
	MPC_LAUNCH(upgma_sw_norm_kernel, std::min<u32>(n - 1, (u32)std::max(1, c->prop.multiProcessorCount) * 8), 256, 0, c->stream, c->up.d_tri.as<float>(), n, (const u32 *)c->d_seq_len.as<u32>());
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(e1, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	float ms = 0;
	HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	c->up.ms_prep = ms;
	return upgma_run(c, "mpcgpu_sw_tree", n, MPC_UPGMA_T_SCALE_SIM, linkage, left, right, left_len, right_len);
}

int mpcgpu_upgma_info(mpcgpu_ctx *c, uint64_t out[4])
{
	if (!c) return 1;
	if (!out) return fail(c, "mpcgpu_upgma_info: NULL argument");
	const mpcgpu_ctx::UpgmaState &u = c->up;
	out[0] = u.n; out[1] = u.lds;
	out[2] = (u64)(u.ms_prep * 1e6); out[3] = (u64)(u.ms_join * 1e6); // nanoseconds
	return 0;
}

int mpcgpu_upgma_scale(mpcgpu_ctx *c, float out[2])
{
	if (!c) return 1;
	if (!out) return fail(c, "mpcgpu_upgma_scale: NULL argument");
	if (!c->up.scaled) return fail(c, "mpcgpu_upgma_scale: the last tree on this context was not built with a scaling transform");
	out[0] = c->up.smin; out[1] = c->up.smax;
	return 0;
}

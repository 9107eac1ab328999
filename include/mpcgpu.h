/*
 * mpcgpu.h — C ABI of libmpcgpu.so: the MI355X (gfx950) implementation of MUSCLE5's MPCFlat
 * all-pairs posterior stage. Plain pointers and sizes only; no C++/torch types.
 *
 * The reference (rcedgar/muscle 5.3) has no plugin/FFI API: its seam is C++ link time, one
 * numeric function per translation unit. Each entry point below names the
 * reference interface it replaces (paths relative to the reference's src/). The C++ drop-in
 * translation units that bind these into an unmodified mpcflat.{h,cpp} are in hostcxx/ and
 * described in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; mpcgpu_last_error() then holds a
 *    message (the reference has no error codes: fatal -> Die(), myutils.cpp:883; the C++ shim
 *    converts non-zero into Die()).
 *  - pair index k enumerates (i<j) row-major over the n sequences, exactly MPCFlat::InitPairs
 *    (mpcflat.cpp:139-159); "pair range [k0,k1)" arguments select a contiguous shard of it.
 *  - sparse posterior matrices cross the boundary in MySparseMx's own layout
 *    (mysparsemx.h:6-98): uint32 offsets[LX+1] and nnz 8-byte entries {float P; uint32 col},
 *    rows ascending, columns ascending.
 *  - the library never falls back to a CPU implementation: without a usable gfx950 device
 *    mpcgpu_create() fails.
 */
#ifndef MPCGPU_H
#define MPCGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpcgpu_ctx mpcgpu_ctx;

/* Library / device lifetime. One context = one GPU = one MPCFlat::Run at a time
 * (device buffers live for one Run: mpcflat.cpp:285-337). */
int mpcgpu_create(mpcgpu_ctx **out, int device_ordinal);
void mpcgpu_destroy(mpcgpu_ctx *ctx);
const char *mpcgpu_last_error(const mpcgpu_ctx *ctx); /* ctx may be NULL: last create() error */
const char *mpcgpu_version(void);

/* Kernel constants. Replaces the process-global PairHMM::m_StartScore[5] / m_TransScore[5][5] /
 * m_MatchScore[256][256] / m_InsScore[256] (pairhmm.h:23-29; filled by HMMParams::ToPairHMM,
 * hmmparams.cpp:298-409; bound inside every DP function by hmmscores.h:1-16). The tables can
 * change between replicates (align.cpp:35-40) so this is called once per Run.
 * min_sparse_score = MIN_SPARSE_SCORE = logf(0.01f) as evaluated by the host (mysparsemx.h:4).
 * expf_variant selects which glibc expf build the device reproduces for calcposteriorflat.cpp:20:
 *   0 = baseline (separate mul/add), 1 = FMA build, -1 = whatever this host's libm resolves to. */
int mpcgpu_set_hmm(mpcgpu_ctx *ctx, const float start[5], const float trans[25],
                   const float match[256 * 256], const float ins[256],
                   float min_sparse_score, int expf_variant);

/* Input sequences. Replaces MPCFlat::InitSeqs + GetBytePtr/GetSeqLength (mpcflat.cpp:41-57,
 * 121-137): n raw ASCII byte strings (already upper-cased by the loader, sequence.cpp:87-88).
 * The bytes are copied; every seven-bit byte value is taken (the emission tables are compacted to the A distinct values that
 * occur, A <= 128, and live in LDS: (A*A + A) floats — beyond the 64 KB default the library asks for the larger dynamic LDS).
 * Bytes >= 128 are refused: the reference indexes m_MatchScore[256][256] by a plain `char` (fwdflat3.cpp:102-109), a negative
 * index there.
 * Also performs MPCFlat::InitPairs (all i<j pairs). Length overflow check of
 * calcposteriorflat.cpp:54-61 (LX*LY*5+100 > INT_MAX) is preserved as an error. Build limits beyond
 * the reference's: a pair whose row sequence is longer than 768 takes the row-block kernels (a choice up to
 * 1024, the only way beyond), which need both lengths <= 65535 (the reference's own limit is ~21k x 21k); the
 * consistency relax runs LDS-tiled while the records of a pair fit the CU's LDS (sequences of up to ~1000-2000 residues,
 * depending on how many cells a row stores; never beyond 4095) and through the gather kernel beyond —
 * mpcgpu_relax_info says which.
 * The size of the all-pairs store is bounded by device memory, not by an index: the row-indexed records are addressed by 32-bit
 * block indices (16-byte blocks) INSIDE A SEGMENT, a run of whole Z slabs (the records (., Z) of all sequences) with a device
 * allocation of its own; a store beyond 2^32 blocks (64 GiB; about 2 900 sequences of length 400) is cut into several
 * (mpcgpu_plan_store_segments) and relaxed by the same band-tile kernel — mpcgpu_relax_info then names the number of segments.
 * What still sends a store to the gather kernel: a sequence longer than 4095 or a record of more than 4095 blocks; n * n or the
 * number of pairs >= 2^32; 2^32 or more stored posteriors in all (about 3 400 sequences of length 400); one Z slab alone of 2^32
 * blocks (n * 4095 blocks: no n below 2^20). */
int mpcgpu_set_seqs(mpcgpu_ctx *ctx, uint32_t n, const uint8_t *const *seqs, const uint32_t *lens);

/* Structure-profile ("mega") emissions for stage A. Replaces the Mega statics a .mega input fills
 * (Mega::FromFile, mega.cpp:119-270; mega.h:9-33) as CalcPost uses them when Mega::m_Loaded
 * (calcpost.cpp:14-22): Mega::CalcFwdFlat_mega / CalcBwdFlat_mega (fwdflat_mega.cpp:14-165,
 * bwdflat_mega.cpp:13-193) with Mega::GetInsScore (mega.cpp:273-285) and Mega::GetMatchScore
 * (mega.cpp:341-363) in place of the PairHMM emission tables; transitions still come from set_hmm.
 *   nfeat                 Mega::m_FeatureCount (<= 8 in this build); 0 switches back to byte sequences
 *   alpha[f], weight[f]   Mega::m_AlphaSizes, Mega::m_Weights
 *   logprobs[f]           Mega::m_LogProbsVec[f]: alpha[f] floats
 *   logprob_mx[f]         Mega::m_LogProbMxVec[f]: alpha[f] x alpha[f] floats, row-major
 *   profiles[i]           profile of sequence i of the last set_seqs/set_seqs_registry (Mega::m_Profiles
 *                         via GetProfileByLabel): len[i] positions x nfeat letters, position-major
 * Call after every set_seqs (which drops the previous profiles). Everything downstream of the
 * emissions (posterior, sparsify, EA, relax, joins) is unchanged. Structure profiles chain too (fb_chain_mega_kernel, kernels_fbc.h:
 * consecutive pairs with the same row sequence swept back to back), per rows-per-lane bin under MPCGPU_FB_CHAIN_MEGA: see
 * mpcgpu_stage_a_info. */
int mpcgpu_set_mega(mpcgpu_ctx *ctx, uint32_t nfeat, const uint32_t *alpha, const float *weight,
                    const float *const *logprobs, const float *const *logprob_mx,
                    const uint8_t *const *profiles);

uint64_t mpcgpu_pair_count(const mpcgpu_ctx *ctx); /* n(n-1)/2 */

/* ---- the store epoch -----------------------------------------------------------------------------------------
 * A counter that moves whenever anything a reader of this context's store could observe may have changed: a caller that has
 * fingerprinted what a store was computed from (the drop-in: the replicates of an ensemble, align.cpp:150-167, run MPCFlat::Run
 * on the same input with the same tables) keeps the epoch beside the fingerprint, and an equal epoch later says the store, the
 * tables, the sequences and the committed values are still the memory it left. One uint64_t in the context, no device work.
 * 0 after mpcgpu_create. Every entry of this header is on one side:
 *   MOVES IT (by at least 1, also when the call then fails half-way; not when the call is refused by the checks it makes before it
 *   touches anything: a NULL argument, a range out of bounds, a missing store, a refused mpcgpu_set_pair_order list, overlapping
 *   shards of mpcgpu_store_import_part): mpcgpu_set_hmm, mpcgpu_set_seqs, mpcgpu_set_seqs_registry, mpcgpu_set_mega, an accepted
 *   mpcgpu_set_pair_order (the order the context already has included: it drops shard and store), mpcgpu_calc_posteriors,
 *   mpcgpu_build_store, mpcgpu_store_import, mpcgpu_store_import_part, mpcgpu_values_import, mpcgpu_cons_iter, mpcgpu_cons_commit,
 *   mpcgpu_cons_commit_range, the list stages mpcgpu_align_pairs and mpcgpu_search_pairs and mpcgpu_align_msas and mpcgpu_post_scores (they take the
 *   scratch and invalidate the all-pairs store), and mpcgpu_group_set_hmm, _set_seqs, _set_mega, _calc_posteriors, _cons_iter on
 *   every context of the group (they are made of the calls above).
 *   LEAVES IT: mpcgpu_store_epoch itself, mpcgpu_last_error, mpcgpu_version, mpcgpu_pair_count, mpcgpu_pair_position,
 *   mpcgpu_plan_partition and mpcgpu_plan_store_segments (no context), mpcgpu_shard_info, mpcgpu_shard_entries, mpcgpu_shard_export,
 *   mpcgpu_store_complete (the same values in records of every sequence), mpcgpu_values_info, mpcgpu_values_slice,
 *   mpcgpu_values_export, mpcgpu_get_ea, mpcgpu_get_nnz, mpcgpu_get_sparse, mpcgpu_get_sparse_range, mpcgpu_get_list_sparse,
 *   mpcgpu_calc_aln, mpcgpu_align_alns, mpcgpu_align_alns_w, mpcgpu_align_alns_batch, mpcgpu_build_post, mpcgpu_get_last_post,
 *   mpcgpu_timers_reset, _enable, _get, mpcgpu_work_get, mpcgpu_stage_a_info, mpcgpu_stage_a_chain_bins, mpcgpu_stage_a_coop_info, mpcgpu_stage_a_fuse_info, mpcgpu_post_info,
 *   mpcgpu_store_info, mpcgpu_relax_info, mpcgpu_search_info, mpcgpu_synchronize, mpcgpu_sw_set_scores, mpcgpu_sw_scores, mpcgpu_sw_info and mpcgpu_sw_bins (tables, letters,
 *   work lists and results of the local-alignment scores live in buffers of their own: shard, store, values and the stage-A scratch are
 *   neither read nor written), mpcgpu_ea_scores and mpcgpu_ea_info (the call runs stage A's sweeps in stage A's scratch, which holds nothing
 *   between calls, and keeps its results in buffers of its own: shard, store, values and the results of the last stage A are neither read
 *   nor written), mpcgpu_upgma, mpcgpu_sw_tree, mpcgpu_upgma_info and mpcgpu_upgma_scale (triangle, row state and tree arrays live in
 *   buffers of their own; mpcgpu_sw_tree's scores in those of mpcgpu_sw_scores), and mpcgpu_group_create, _destroy, _last_error, _size, _ctx, _transport.
 * (mpcgpu_values_info hands out the device address of the NEXT values, which the caller of a sharded run writes itself: such a
 * write is seen by no reader until mpcgpu_cons_commit(_range), which moves the epoch.) */
int mpcgpu_store_epoch(mpcgpu_ctx *ctx, uint64_t *epoch);

/* ---- pair order of a block-partitioned multi-GPU run -------------------------------
 * MPCFlat::InitPairs (mpcflat.cpp:139-159) enumerates the pairs row-major, and a contiguous range of that order holds pairs
 * (X, Y) with Y anywhere behind X: a rank that owns such a range needs the sparse matrices of nearly every sequence for
 * MPCFlat::ConsPair (conspairflat.cpp:37-92). A rank that owns BLOCKS of the pair triangle (sequence group i x group j) needs
 * those of a few groups only. mpcgpu_set_pair_order makes the context enumerate its pairs rectangle by rectangle (row-major
 * inside each): rects[4 r ..] = {xa, xb, ya, yb} is either off the diagonal (ya >= xb: every (x, y) of [xa,xb) x [ya,yb)) or a
 * triangle (xa == ya, xb == yb: the pairs x < y inside [xa,xb)); together they must hold every pair exactly once. nrects == 0:
 * back to InitPairs order. Call after mpcgpu_set_seqs (which resets it), before stage A. A refused list changes nothing: the
 * order, shard and store the context had stay as they were.
 * From then on the SHARDING calls — mpcgpu_calc_posteriors, mpcgpu_store_import(_part), mpcgpu_values_slice, mpcgpu_cons_iter —
 * take POSITIONS in this order ("[k0,k1)" = the k0-th to k1-th pair of the enumeration), and the values array is in position
 * order; the RESULT getters (mpcgpu_get_ea, _get_nnz, _get_sparse, _get_sparse_range) and everything that names sequences
 * (mpcgpu_align_alns ...) keep speaking InitPairs pair numbers / sequence indices. */
int mpcgpu_set_pair_order(mpcgpu_ctx *ctx, uint32_t nrects, const uint32_t *rects);
/* position of pair (x, y), x < y, in the context's pair order */
int mpcgpu_pair_position(mpcgpu_ctx *ctx, uint32_t x, uint32_t y, uint64_t *pos);
/* The partition itself (host only, no context): n sequences of the given lengths over `world` ranks. Sequences fall into g groups
 * of equal weight (sum of L + 1), the pair triangle into g (g + 1) / 2 blocks, a rank owns whole blocks: world = g (g - 1) / 2 +
 * g / 2 with g even (2, 8, 18 ...) — one off-diagonal block per rank and one rank per two diagonal blocks (8 ranks: every rank
 * touches 2 of 4 groups, half of the store); any other world — g = world, rank i owns the triangle of group i and the blocks
 * {i, i + d}, d < g / 2, the antipodal blocks of an even g cut in two by rows. rects (capacity max_rects x 4 words) receives the
 * rectangles in rank order, rank_pos[world + 1] the positions where each rank's pairs begin: rank r owns [rank_pos[r],
 * rank_pos[r + 1]). *nrects == 0: no block cut (one rank, too few sequences): InitPairs order,
 * contiguous ranges balanced by DP cells — the partition of rounds 1-5. Returns 0, or 2 when max_rects is too small. */
int mpcgpu_plan_partition(uint32_t n, const uint32_t *lens, uint32_t world, uint32_t max_rects, uint32_t *rects,
                          uint32_t *nrects, uint64_t *rank_pos);

/* The segments of a record store (host only, no context; the store build calls the same function). sizes: the n * n record sizes
 * in 16-byte blocks, Z-MAJOR (sizes[Z * n + A] = record (A, Z)); limit_blocks: the most a segment may hold, 0 or anything above it = the layout's own
 * limit, 2^32 - 1 (a record's start and a slab's end are 32-bit block indices inside their segment). The n Z slabs are cut into
 * the fewest runs of consecutive slabs within the limit: segment g holds the slabs [z_first[g], z_first[g + 1]) and blocks[g]
 * blocks; z_first has max_segs + 1 entries, blocks max_segs. *nsegs receives the number of segments. Returns 0; 1 for missing
 * arguments; 2 when max_segs is too small (*nsegs is set: call again); 3 when one slab alone is larger than the limit (no
 * segmentation exists: a store build falls back to the gather layout). */
int mpcgpu_plan_store_segments(uint32_t n, const uint32_t *sizes, uint64_t limit_blocks, uint32_t max_segs, uint32_t *z_first,
                               uint64_t *blocks, uint32_t *nsegs);

/* Stage A for the pair range [k0,k1): replaces MPCFlat::CalcPosteriors' OpenMP loop
 * (mpcflat.cpp:239-251) over MPCFlat::CalcPosterior (calcposteriorflat.cpp:45-92), i.e.
 * CalcFwdFlat (fwdflat3.cpp:12) + CalcBwdFlat (bwdflat3.cpp:10) + CalcTotalProbFlat
 * (totalprobflat.cpp:3) + CalcPostFlat (calcposteriorflat.cpp:4) + MySparseMx::FromPost
 * (mysparsemx.cpp:115) + CalcAlnScoreFlat (calcalnscoreflat.cpp:4) + EA = Score/min(LX,LY).
 * Results stay on the device ("packed shard"). */
int mpcgpu_calc_posteriors(mpcgpu_ctx *ctx, uint64_t k0, uint64_t k1);

/* Builds the device-resident all-pairs store the relax kernel reads, from this context's own
 * shard. Only valid when the shard is the full range [0, pair_count) (single GPU). */
int mpcgpu_build_store(mpcgpu_ctx *ctx);

/* ---- multi-GPU exchange (one process per GPU; the collective itself is the caller's RCCL
 * all-gather over xGMI on these device pointers — SURVEY.md §8e) --------------------------- */
/* Size in bytes and device address of this context's packed shard (valid after calc_posteriors). */
int mpcgpu_shard_info(mpcgpu_ctx *ctx, uint64_t *bytes, void **dev_ptr);
/* Stored cells (sparse posterior entries) of this context's shard: this rank's share of the values a relax iteration exchanges
 * (mpcgpu_values_slice gives the same count once the store exists; this one is known right after stage A, so that a caller sizes
 * both exchanges — the shards' bytes and the values' counts — with ONE size exchange). */
int mpcgpu_shard_entries(mpcgpu_ctx *ctx, uint64_t *entries);
/* Copy the packed shard (bytes from mpcgpu_shard_info) into caller-owned device memory. */
int mpcgpu_shard_export(mpcgpu_ctx *ctx, void *dev_dst);
/* Build the all-pairs store from nshards packed shards laid out back to back in device memory
 * (dev_all; shard s occupies bytes[s] bytes, covers pairs [k0[s],k1[s]), ascending, contiguous,
 * covering [0,pair_count)). The library ADOPTS dev_all as the packed half of its store: it must stay
 * valid and otherwise untouched until the next set_seqs/destroy, and mpcgpu_cons_commit writes the
 * new probabilities into it (the swap of consflat.cpp:22) — hence not const. */
int mpcgpu_store_import(mpcgpu_ctx *ctx, uint32_t nshards, const uint64_t *k0, const uint64_t *k1,
                        const uint64_t *bytes, void *dev_all);
/* The same for a rank of a pair-sharded run whose stage A ran in pieces: the shards may come in any order and lie anywhere in
 * dev_all (offsets[s], multiples of 4; NULL: back to back in the order given); sorted by k0 they must tile [0, pair_count).
 * [own_k0, own_k1) = the positions this context will relax (mpcgpu_cons_iter): the store is PARTIAL — it holds the row-indexed
 * matrices (A, Z) of the sequences A that those pairs touch and of no other (the block partition: half of the store at 8 ranks;
 * what a ConsPair of the range reads, conspairflat.cpp:49-89), while everything per pair (packed matrices, values, EA) is
 * complete. mpcgpu_cons_iter outside the range is refused; mpcgpu_cons_commit(_range) commits every entry into what exists.
 * Shards whose byte ranges [offsets[s], offsets[s] + bytes[s]) overlap are refused before the current store is touched.
 * own = [0, pair_count) is mpcgpu_store_import. */
int mpcgpu_store_import_part(mpcgpu_ctx *ctx, uint32_t nshards, const uint64_t *k0, const uint64_t *k1, const uint64_t *bytes,
                             const uint64_t *offsets, void *dev_all, uint64_t own_k0, uint64_t own_k1);
/* Makes a partial store whole (the matrices of every sequence, from the packed ones, which hold the current values): what the
 * host that reads results — progressive alignment, MPCFlat::BuildPost — needs after the last mpcgpu_cons_iter. mpcgpu_align_alns
 * and mpcgpu_build_post call it themselves; a no-op on a complete store. */
int mpcgpu_store_complete(mpcgpu_ctx *ctx);
/* Device address + element count of the float array holding the next-iteration probabilities of
 * ALL pairs in canonical order (pair ascending, entries row-major), and the [first, first+count)
 * slice that cons_iter(k0,k1) writes. The caller all-gathers the slices in place, then commits. */
int mpcgpu_values_info(mpcgpu_ctx *ctx, void **dev_ptr, uint64_t *total_count);
int mpcgpu_values_slice(mpcgpu_ctx *ctx, uint64_t k0, uint64_t k1, uint64_t *first, uint64_t *count);
/* Copy count floats starting at canonical entry index `first` out of / into the values array
 * (caller-owned device memory on the other side) — the staging form of the same exchange. */
int mpcgpu_values_export(mpcgpu_ctx *ctx, uint64_t first, uint64_t count, void *dev_dst);
int mpcgpu_values_import(mpcgpu_ctx *ctx, uint64_t first, uint64_t count, const void *dev_src);

/* One consistency iteration for the pair range [k0,k1): replaces MPCFlat::ConsIter
 * (consflat.cpp:5-23) -> ConsPair (conspairflat.cpp:10-110) -> RelaxFlat_{XZ_ZY,ZX_ZY,XZ_YZ}
 * (relaxflat.cpp:4-94) -> MySparseMx::UpdateFromPost (mysparsemx.cpp:87-113). Jacobi: reads the
 * current store, writes the "values" array; mpcgpu_cons_commit makes them current (the buffer
 * swap of consflat.cpp:22). */
int mpcgpu_cons_iter(mpcgpu_ctx *ctx, uint64_t k0, uint64_t k1);
int mpcgpu_cons_commit(mpcgpu_ctx *ctx);
/* The same swap for the canonical entries [first, first+count) only (see mpcgpu_values_slice): a rank of a pair-sharded run
 * commits the slice it relaxed itself while the other ranks' values are still arriving, and the rest after them. Committing
 * every entry exactly once, in any split, equals mpcgpu_cons_commit (consflat.cpp:22). */
int mpcgpu_cons_commit_range(mpcgpu_ctx *ctx, uint64_t first, uint64_t count);

/* ---- results back to the host (the reference's in-memory formats) ------------------------- */
/* EA per pair: what calcposteriorflat.cpp:89-91 stores in m_DistMx[i][j]. Valid for own shard
 * after calc_posteriors, for all pairs after build_store/store_import. */
int mpcgpu_get_ea(mpcgpu_ctx *ctx, uint64_t k0, uint64_t k1, float *ea);
/* nnz per pair (MySparseMx::m_VecSize). */
int mpcgpu_get_nnz(mpcgpu_ctx *ctx, uint64_t k0, uint64_t k1, uint32_t *nnz);
/* Current sparse matrix of pair k in MySparseMx layout: offsets[LX+1], values[8*nnz bytes]. */
int mpcgpu_get_sparse(mpcgpu_ctx *ctx, uint64_t k, uint32_t *offsets, void *values);
/* Bulk form for [k0,k1): offsets concatenated (sum of LX+1 uint32), values concatenated
 * (8*sum nnz bytes). Sizes via mpcgpu_get_nnz and the sequence lengths. */
int mpcgpu_get_sparse_range(mpcgpu_ctx *ctx, uint64_t k0, uint64_t k1, uint32_t *offsets, void *values);

/* The finishing kernels on one caller-supplied candidate list (cells (rows[q], cols[q]) with log-space Score scores[q] >=
 * MIN_SPARSE_SCORE, any order, no duplicates): the expf half of CalcPostFlat (calcposteriorflat.cpp:16-22),
 * MySparseMx::FromPost (mysparsemx.cpp:115-152) and CalcAlnScoreFlat / EA (calcalnscoreflat.cpp:4-32,
 * calcposteriorflat.cpp:89) for ONE pair of lengths LX, LY. kernel: 0 = row-list kernel (post_rows_kernel), 1 = general (sort)
 * kernel (post_kernel), 2 = the workgroup-per-pair kernel (post_wide_kernel: radix sort, row-start table, EA over the whole
 * workgroup; MPCGPU_POSTW_LDS = entries it sorts in LDS and floats of an LDS DP row, 0 = everything through its global slots);
 * any other value is refused.
 * batch: cells of a row per EA pass (64; smaller values exercise the multi-pass path). offsets[LX+1] / values (8 bytes per
 * kept entry, capacity ncand) may be NULL. A unit-test reach into inputs the pair-HMM itself never produces. */
int mpcgpu_post_scores(mpcgpu_ctx *ctx, uint32_t LX, uint32_t LY, uint32_t ncand, const uint32_t *rows,
                       const uint32_t *cols, const float *scores, int kernel, uint32_t batch, float *ea, uint32_t *nnz,
                       uint32_t *offsets, void *values);

/* Posterior-DP alignment of one dense LX x LY matrix resident in HOST memory: replaces
 * CalcAlnFlat (calcalnflat.cpp:6-46) + TraceBackFlat (tracebackflat.cpp:3-37), tie order of
 * best3.h:5-28. path receives the B/X/Y string (capacity >= LX+LY), not NUL-terminated.
 * Limits: none on the columns from the kernels (a matrix wider than the two DP rows the LDS holds, LY + 1 > ~20 470, is swept in
 * column tiles: same cells, same comparisons, same letters); the matrix (4 * LX * LY bytes) and its traceback letters
 * ((LX + 1) * (LY + 1) bytes) must fit device memory. */
int mpcgpu_calc_aln(mpcgpu_ctx *ctx, const float *post, uint32_t LX, uint32_t LY,
                    char *path, uint32_t *pathlen, float *score);

/* Alignment of two alignments on the device: replaces MPCFlat::AlignAlns' numeric part
 * (alnalnsflat.cpp:7-52) = MPCFlat::BuildPost (buildpostflat.cpp:18-106: dense C1 x C2 matrix, sum over
 * s in MSA1 (outer), t in MSA2 (inner) of the CURRENT pairwise posteriors of the device store scattered
 * through the position->column maps, weights 1.0f as set at mpcflat.cpp:324) followed by CalcAlnFlat +
 * TraceBackFlat (calcalnflat.cpp:6-46, tracebackflat.cpp:3-37) on it. Bit-exact: every cell receives
 * its contributions in the reference's (s,t) order.
 * seq1[n1] / seq2[n2]: sequence indices (InitPairs numbering) of the rows of MSA1 / MSA2, in row order;
 * pos2col1 / pos2col2: Sequence::GetPosToCol (sequence.cpp:144-154) of every row, concatenated
 * (row a contributes len(seq a) entries); C1, C2: column counts. path: B/X/Y string, capacity C1+C2. */
int mpcgpu_align_alns(mpcgpu_ctx *ctx, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2,
                      uint32_t C1, uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2,
                      char *path, uint32_t *pathlen, float *score);
/* The same with sequence weights: every contribution is (w1[a] * w2[b]) * P, the product of the two weights rounded first,
 * as at buildpostflat.cpp:41,52,74,96 (w1[a] / w2[b] = the reference's m_Weights[SeqIndex1] / m_Weights[SeqIndex2] of row a of
 * MSA1 / row b of MSA2; NULL = all 1.0f, which is what MPCFlat::Run sets at mpcflat.cpp:324). */
int mpcgpu_align_alns_w(mpcgpu_ctx *ctx, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2,
                        uint32_t C1, uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2,
                        const float *w1, const float *w2, char *path, uint32_t *pathlen, float *score);

/* mpcgpu_align_alns for a LIST of independent joins: the joins of one level of the guide tree MPCFlat::ProgressiveAlign walks
 * (progalnflat.cpp:72-100 runs its N - 1 joins one after the other; a join needs only its two children). Join j aligns n1[j] rows
 * with n2[j] rows, C1[j] x C2[j] columns; seqs holds the sequence indices of its rows, MSA1's then MSA2's, the joins back to back;
 * pos2col likewise the rows' position -> column maps. All weights are 1.0f (what MPCFlat::Run sets, mpcflat.cpp:324).
 * paths: njoins slots of path_stride bytes (>= C1[j] + C2[j]); scores may be NULL. The small joins — nearly all of a tree's — run
 * in two launches together, the few large ones as mpcgpu_align_alns does; every matrix and path is the single call's.
 * Here, in mpcgpu_align_alns(_w), mpcgpu_build_post and mpcgpu_align_msas a row's position -> column map must rise strictly (as
 * Sequence::GetPosToCol of an aligned row does); a map with two positions on one column or a step back is refused. */
int mpcgpu_align_alns_batch(mpcgpu_ctx *ctx, uint32_t njoins, const uint32_t *n1, const uint32_t *n2, const uint32_t *C1,
                            const uint32_t *C2, const uint32_t *seqs, const uint32_t *pos2col, uint32_t path_stride,
                            char *paths, uint32_t *pathlens, float *scores);

/* MPCFlat::BuildPost alone (buildpostflat.cpp:18-106): the C1 x C2 matrix (row-major floats, host memory) that
 * mpcgpu_align_alns_w would align — for the callers of BuildPost outside MPCFlat::Run (profseq.cpp:33-49). Arguments as
 * for mpcgpu_align_alns_w (w1 / w2 may be NULL: all weights 1.0f). */
int mpcgpu_build_post(mpcgpu_ctx *ctx, uint32_t n1, const uint32_t *seq1, uint32_t n2, const uint32_t *seq2, uint32_t C1,
                      uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, const float *w1, const float *w2,
                      float *post);
/* The dense matrix of the last mpcgpu_align_alns(_w) / mpcgpu_build_post / mpcgpu_align_msas / mpcgpu_calc_aln call on this
 * context (C1 x C2 must be that call's shape): what BuildPost (buildpostflat.cpp:18-106) resp. CalcPosteriorFlat3
 * (buildposterior3flat.cpp:19-85) left for CalcAlnFlat. */
int mpcgpu_get_last_post(mpcgpu_ctx *ctx, uint32_t C1, uint32_t C2, float *post);

/* The MSA x MSA join of PProg (pprog2.cpp:7-56 -> PProg::AlignMSAsFlat, alnmsasflat.cpp:4-50) for an
 * explicit list of cross pairs (getpairs.cpp:33-69 samples at most 2000): per pair
 * PProg::GetPostPairsAlignedFlat (getpostpairsalignedflat.cpp:5-98) = CalcPost + MySparseMx::FromPost
 * + the alignment score (EA = Score / min(L1,L2)), then CalcPosteriorFlat3
 * (buildposterior3flat.cpp:19-85, contributions in pair-list order) and CalcAlnFlat + TraceBackFlat.
 * Sequences are indices into the set given to mpcgpu_set_seqs_registry (the reference's global input
 * registry, globalinputms.cpp:11-143: any sequence may pair with any other, no all-pairs tables);
 * pair q aligns seq1[q] (a row of MSA1, X) with seq2[q] (a row of MSA2, Y); pos2col1 / pos2col2 hold
 * the position->column map of seq1[q] / seq2[q] for q = 0..npairs-1, concatenated. ea_out (may be
 * NULL) receives EA per pair. */
int mpcgpu_set_seqs_registry(mpcgpu_ctx *ctx, uint32_t n, const uint8_t *const *seqs, const uint32_t *lens);
int mpcgpu_align_msas(mpcgpu_ctx *ctx, uint32_t npairs, const uint32_t *seq1, const uint32_t *seq2, uint32_t C1,
                      uint32_t C2, const uint32_t *pos2col1, const uint32_t *pos2col2, char *path, uint32_t *pathlen,
                      float *score, float *ea_out);

/* AlignPairFlat (alignpairflat.cpp:3-27; callers uclust.cpp:14, transaln.cpp:787, eadistmx.cpp:54, eacluster.cpp:209) for a
 * LIST of pairs of registered sequences: CalcPost (calcpost.cpp:4-36: fwd + bwd + CalcPostFlat), CalcAlnFlat + TraceBackFlat on the
 * dense thresholded posterior. paths: npairs slots of path_stride bytes (>= LX+LY of every pair), B/X/Y strings of pathlens[q]
 * characters; scores[q] = CalcAlnFlat's score, ea[q] = score / min(LX, LY) — what AlignPairFlat returns (either may be NULL).
 * The sparse matrices of the same pairs (AlignPairFlat_SparsePost) are then available through mpcgpu_get_list_sparse.
 * Like every stage-A call on a context, this one takes the context's scratch and INVALIDATES the all-pairs store the context may
 * hold (mpcgpu_build_store / mpcgpu_store_import): callers that interleave pair lists with a consistency run use a context of
 * their own for the lists (the drop-in's join contexts). A list is cut into chunks that one stage-A batch serves and whose dense
 * matrices fit the device together (halved as often as needed, down to one pair).
 * Limits: a pair must satisfy the reference's own test, double(LX) * double(LY) * 5 + 100 <= INT_MAX (calcposteriorflat.cpp:54-61,
 * about 20 724 x 20 724, or 7 000 x 60 000) — a list with a pair beyond it is refused before any device work, with an error that names
 * both lengths and the bound — and what stage A asks of the lengths (65 535 positions per sequence once the row sequence takes the
 * row-block kernels; mpcgpu_set_seqs_registry tests no pairs, the calls that receive them do). A list whose sequences do not fit the
 * row-list finishing kernel (roughly LXmax + 2 * LYmax > 36 344: sequences beyond ~12 000 residues) is finished by the sort-based
 * kernel and its dense posteriors are built from the raw candidate lists: same bits. MPCGPU_POST=sort forces the sort-based kernel on
 * lists that would fit and is refused here (error, not a fallback). */
int mpcgpu_align_pairs(mpcgpu_ctx *ctx, uint32_t npairs, const uint32_t *seq1, const uint32_t *seq2, uint32_t path_stride,
                       char *paths, uint32_t *pathlens, float *scores, float *ea);
/* MySparseMx::FromPost (mysparsemx.cpp:115-152) of pair q of the LAST list stage on this context (mpcgpu_align_pairs of at most 256
 * pairs, mpcgpu_align_msas): nnz, offsets[LX+1], values (8 bytes per entry; capacity from a first call with values == NULL). */
int mpcgpu_get_list_sparse(mpcgpu_ctx *ctx, uint32_t q, uint32_t *nnz, uint32_t *offsets, void *values);

/* The loop of UClust::Search (uclust.cpp:44-54) for a LIST of queries (kernels_search.h, mpcgpu_search.inc): the reference aligns a query's
 * word-count hits one after the other with AlignPairFlat and keeps the path of the first whose EA reaches the threshold. Group g holds the
 * candidate pairs [group_first[g], group_first[g + 1]) of registered sequences in the order they are to be tried (group_first: ngroups + 1
 * entries, ascending from 0; an empty group is allowed).
 *   ea[q]        (all pairs; may be NULL) the float mpcgpu_align_pairs returns for the pair, bit for bit
 *   accepted[g]  the smallest t with ea[group_first[g] + t] >= min_ea — the reference's own comparison, so a NaN never qualifies —, UINT32_MAX
 *                when no candidate qualifies
 *   paths (ngroups slots of path_stride bytes), pathlens[g], scores[g] (may be NULL): path and CalcAlnFlat score of the accepted pair, the
 *                bytes mpcgpu_align_pairs writes; pathlens[g] = 0 for a group without one
 * ONLY THE ACCEPTED PAIRS get a dense posterior and a trace-back: a pair's EA is known after the finishing kernel. The list runs in chunks
 * of MPCGPU_SEARCH_CHUNK pairs (512; at most 1024) that may end inside a group — a group that has its hit enters later chunks with nothing
 * to try; the result does not depend on the cut. A chunk that satisfies what mpcgpu_align_pairs asks of a short list (no row-block pair, every
 * alignment a one-wave alignment, the row-list finishing kernel) runs FUSED: sweeps, finishing kernel, search_pick_kernel (a wavefront per
 * group folds its candidates' EAs), then the dense build and the one-wave alignment indirectly — a workgroup per group reads the pick on the
 * device and leaves when there is none — on one stream with one wait. Every other chunk, a fused chunk whose candidate room overflowed, and
 * every chunk under MPCGPU_SEARCH_FUSED=0 takes the GENERAL route: stage A as mpcgpu_align_pairs runs it, the EAs read back, the picks made
 * on the host, dense posteriors and alignments for the picked pairs only. Same bits on both.
 * A list stage like mpcgpu_align_pairs: it moves the store epoch, takes the scratch and invalidates an all-pairs store. It keeps no sparse
 * matrices: mpcgpu_get_list_sparse after it is refused by name.
 * Refused by name before any device work, the context left as it was: no sequences; a NULL argument other than scores / ea; a group_first
 * that does not ascend from 0; an index outside the set; a path_stride smaller than LX + LY of a candidate; a pair beyond
 * mpcgpu_align_pairs' envelope (LX * LY * 5 + 100 > INT_MAX). */
int mpcgpu_search_pairs(mpcgpu_ctx *ctx, uint32_t ngroups, const uint32_t *group_first, const uint32_t *seq1, const uint32_t *seq2,
                        float min_ea, uint32_t path_stride, char *paths, uint32_t *pathlens, uint32_t *accepted, float *scores, float *ea);
/* The last mpcgpu_search_pairs call: out[0] groups, out[1] pairs, out[2] pairs whose dense posterior and trace-back were handed out (= the
 * accepted groups, on both routes: the saving), out[3] chunks, out[4] chunks on the general route, out[5] device nanoseconds of pick + dense
 * posteriors + alignments (hipEvents). All 0 before the first call; a refused call leaves them. */
int mpcgpu_search_info(mpcgpu_ctx *ctx, uint64_t out[6]);

/* ---- guide tree from bare sequences: all-pairs local-alignment scores (kernels_sw.h, mpcgpu_sw.inc) ------------------------
 * Tables of the score-only Smith-Waterman below. Replaces what MakeBlosum62SMx builds per pair (blosumsmx.cpp:32-53: a letter pair
 * scores Blosum62_sij[a][b], blosum.cpp:8, when both letters are < 20 and 0 otherwise) and the Open / Ext arguments of SWFast_SMx
 * (sw.cpp:142-144; -11 and -1 at swdistmx.cpp:106-107). The caller supplies the tables, the library carries no copy of them:
 *   letter_of_char[256]   g_CharToLetterAmino (alpha.cpp): the letter of every byte value
 *   alpha, sub            alphabet size (1 .. 32) and alpha x alpha scores, row-major; a letter >= alpha scores 0 against everything
 *   open, ext             gap scores, both <= 0 (sw.cpp:151-152 asserts the same)
 * Single context only; the tables stay until the next call or mpcgpu_destroy. */
int mpcgpu_sw_set_scores(mpcgpu_ctx *ctx, const uint8_t letter_of_char[256], uint32_t alpha, const float *sub, float open,
                         float ext);
/* Raw local-alignment scores of a list of pairs of the set given to mpcgpu_set_seqs_registry (or mpcgpu_set_seqs): pair q aligns
 * seq1[q] with seq2[q]; seq1 == seq2 == NULL means all pairs i < j in InitPairs order (npairs must then be n (n - 1) / 2). Replaces
 * the value SWFast_Seqs_BLOSUM62 returns (sw.cpp:287-295 -> SWFast_SMx, sw.cpp:142-275) in ThreadBody's loop over all pairs
 * (swdistmx.cpp:25-85), bit for bit: every cell is the reference's chain of single fp32 adds and maxima. The trace-back
 * (TraceBackBitSW, sw.cpp:69-140), which feeds only a log line there, is not computed, and no LA x LB matrix exists; the
 * normalisation by the mean length (swdistmx.cpp:75-76) stays with the caller. Consecutive pairs with the same first sequence and
 * second sequences q, q + 1, ... are swept as one chain (MPCGPU_SW_CHAIN_COLS columns at most, 8192). The list is cut into batches
 * of MPCGPU_SW_BATCH pairs (2^24): a result word per pair and a 16-byte item per chain, in device memory of the call's own.
 * Refused by name before any device work, the context left as it was: scores not set, no sequences, an index outside the set, a
 * sequence of more than 65 535 positions among those the list names, a pair count that is not n (n - 1) / 2 with NULL lists. */
int mpcgpu_sw_scores(mpcgpu_ctx *ctx, uint64_t npairs, const uint32_t *seq1, const uint32_t *seq2, float *scores);
/* The last mpcgpu_sw_scores call: out[0] pairs, out[1] DP cells (sum of LA x LB), out[2] batches, out[3] chains, out[4] chains whose
 * first sequence is longer than 512 and ran in row blocks, out[5] device time of the kernels in nanoseconds (hipEvents around each batch). */
int mpcgpu_sw_info(mpcgpu_ctx *ctx, uint64_t out[6]);
/* last mpcgpu_sw_scores call, summed over its batches: per bin b = 1 .. MPC_SW_HMAX + 1 (index 0 unused; bins 1 .. 8: sw_kernel<b> with b
 * rows per lane, bin 9: the row-block kernel) items[b] = work items of the bin, groups[b] = workgroups launched for it (4 waves each) */
int mpcgpu_sw_bins(mpcgpu_ctx *ctx, uint64_t items[10], uint64_t groups[10]);

/* ---- UPGMA on the device (kernels_upgma.h, mpcgpu_upgma.inc) ----------------------------------------------------------------
 * The tree UPGMA5 builds from a distance matrix. dist: the n (n - 1) / 2 distances of the pairs i < j in InitPairs order
 * (mpcflat.cpp:145-155), the order mpcgpu_sw_scores and mpcgpu_ea_scores write. transform, applied first:
 *   MPCGPU_UPGMA_NONE        the values as they are (cmd_upgma5 without options, upgma5.cpp:578)
 *   MPCGPU_UPGMA_SCALE_SIM   UPGMA5::ScaleDistMx(true), upgma5.cpp:521-563: 10 * (Max - d) / (Max - Min) (-scaledist, -reseek, swdistmx.cpp:125)
 *   MPCGPU_UPGMA_SCALE_DIST  UPGMA5::ScaleDistMx(false): 10 * (d - Min) / (Max - Min)
 *   MPCGPU_UPGMA_EA          UPGMA5::FixEADistMx, upgma5.cpp:504-519: 1 - d (-eadist)
 * Then UPGMA5::Run(linkage), upgma5.cpp:87-305: negative distances become 0, every row's smallest distance and nearest neighbour, and n - 1
 * joins with the linkage formula MPCGPU_UPGMA_AVG, _MIN, _MAX or _BIASED (upgma5.cpp:227-247) — the reference's procedure statement by
 * statement, with the cached row minima it never repairs and the neighbour redirect of upgma5.cpp:249-259, every float rounded as the
 * reference rounds it. Outputs, n - 1 entries each: the arrays UPGMA5::Run hands to Tree::Create (upgma5.cpp:306-308) — left / right child
 * of internal node k (a value < n is a leaf, n + k' internal node k'), and the branch lengths to them. The root is node n - 2.
 * One persistent workgroup runs the joins; the per-row state is in LDS up to MPCGPU_UPGMA_LDS_ROWS rows (12 288, also the most), in global
 * memory beyond. Only the triangle goes to the device and 4 (n - 1) words come back.
 * Refused by name before any device work, the context left as it was: n < 2; n > 65 536 (upgma5.h:68: the reference's own 32-bit
 * uIndex1 * (uIndex1 - 1) wraps there); an unknown transform or linkage; a NULL argument; a triangle that does not fit the device's free
 * memory. Refused by name after the run, the outputs untouched: an EA value outside 0 .. 1 (the reference dies, upgma5.cpp:512); a join
 * that finds no distance below FLT_MAX (the reference asserts, upgma5.cpp:197-199: all remaining distances FLT_MAX or NaN, as after
 * scaling a matrix whose entries are all equal).
 * A reader in the sense of mpcgpu_store_epoch, with buffers of its own. */
enum { MPCGPU_UPGMA_NONE = 0, MPCGPU_UPGMA_SCALE_SIM = 1, MPCGPU_UPGMA_SCALE_DIST = 2, MPCGPU_UPGMA_EA = 3 };
enum { MPCGPU_UPGMA_AVG = 0, MPCGPU_UPGMA_MIN = 1, MPCGPU_UPGMA_MAX = 2, MPCGPU_UPGMA_BIASED = 3 };
int mpcgpu_upgma(mpcgpu_ctx *ctx, uint32_t n, const float *dist, int transform, int linkage, uint32_t *left, uint32_t *right,
                 float *left_len, float *right_len);
/* The guide tree of CalcGuideTree_SW_BLOSUM62 (swdistmx.cpp:87-127) for the set given to mpcgpu_set_seqs(_registry), with the tables of
 * mpcgpu_sw_set_scores, in one call: the all-pairs scores of mpcgpu_sw_scores written to device memory, NormScore = Score / ((Li + Lj) / 2.0f)
 * there (swdistmx.cpp:75-76), ScaleDistMx(true) and UPGMA5::Run(linkage) as above (swdistmx.cpp:123-126 with LINKAGE_Avg). No n x n matrix
 * exists on either side; the four tree arrays come back, and the raw scores (n (n - 1) / 2 floats, the bits of mpcgpu_sw_scores) when
 * scores != NULL. Refusals: those of mpcgpu_sw_scores for all pairs and of mpcgpu_upgma. mpcgpu_sw_info reports the scores' part. */
int mpcgpu_sw_tree(mpcgpu_ctx *ctx, int linkage, uint32_t *left, uint32_t *right, float *left_len, float *right_len, float *scores);
/* The last mpcgpu_upgma / mpcgpu_sw_tree call: out[0] n, out[1] 1 when the row state lived in LDS, out[2] device nanoseconds of transform and
 * initialisation (for mpcgpu_sw_tree with the normalisation), out[3] device nanoseconds of the join loop (hipEvents). */
int mpcgpu_upgma_info(mpcgpu_ctx *ctx, uint64_t out[4]);
/* out[0] = Min, out[1] = Max as the last call's scaling transform found them (the values of ScaleDistMx's "Re-scaling" log line,
 * upgma5.cpp:536; the scaled extremes of upgma5.cpp:561 follow from them: the transform is monotone). Refused when the last tree was built
 * without a scaling transform. */
int mpcgpu_upgma_scale(mpcgpu_ctx *ctx, float out[2]);

/* ---- EA of a list of pairs, nothing else: the distance matrix over consensus sequences (kernels_postea.h, mpcgpu_ea.inc) ----------------
 * ea[q] = the float AlignPairFlat returns for (seq1[q], seq2[q]) — CalcAlnFlat's score over the dense thresholded posterior divided by
 * min(L1, L2) (alignpairflat.cpp:11,19) — for pairs of the set given to mpcgpu_set_seqs_registry (or mpcgpu_set_seqs); seq1 == seq2 == NULL
 * means all pairs i < j in InitPairs order (mpcflat.cpp:145-155; npairs must then be n (n - 1) / 2). Replaces the loop of CalcEADistMx
 * (eadistmx.cpp:33-69), which keeps that one float per pair and throws the path away; the same bits as mpcgpu_calc_posteriors +
 * mpcgpu_get_ea and as mpcgpu_align_pairs' ea.
 * The forward/backward sweeps are stage A's own, through its dispatcher: chains where consecutive pairs share the row sequence,
 * fb_kernel otherwise, row blocks from 769 rows on, structure profiles wherever mpcgpu_set_mega is in force. The finish is post_ea_kernel:
 * probabilities and the EA recurrence exactly as post_rows_kernel forms them, one float out — no trace-back, no packed record, no sparse
 * matrix; nothing is read back from the device but ea[]. The list runs in batches bounded like stage A's by MPCGPU_SCRATCH_GB (a pair costs
 * its candidate room alone, so the batches are larger), and a batch whose candidate room overflows is redone with twice the room.
 * post_ea_kernel keeps three per-position arrays in a CU's LDS, which two sequences of 12 115 positions no longer fit. With MPCGPU_EA_WIDE=1
 * (unset = 0 in the library; the drop-in binary sets 1) the list is split: a pair whose longer sequence has at least MPCGPU_EA_WIDE_MIN
 * positions (unset: 12 115 at the default MPCGPU_POST_SORT_CAP, the smallest length at which two such sequences stop fitting) is WIDE.
 * The narrow pairs run as above, then the wide pairs the same way with post_wide_ea_kernel as the finish (kernels_postwea.h: a workgroup per
 * pair, the first half of post_wide_kernel — radix sort, row starts in global scratch, the EA recurrence across all lanes; the same bits),
 * each sub-list with its own geometry, batches and candidate room; the floats go back into the caller's order.
 * A reader in the sense of mpcgpu_store_epoch: shard, store, committed values and what the getters and the info calls report of the last
 * stage A stay as they are — mpcgpu_align_alns on a store built before the call gives what it gave before. (Stage A's scratch is used; no
 * call keeps anything there.)
 * Refused by name before any device work, the context left as it was: no sequences; one list NULL and the other not; a pair count that is
 * not n (n - 1) / 2 with NULL lists; an index outside the set; a pair beyond the envelope of mpcgpu_align_pairs (LX * LY * 5 + 100 >
 * INT_MAX, calcposteriorflat.cpp:54-61; more than 65 535 positions once the row sequence takes the row-block kernels); a list whose
 * NARROW pairs do not fit the LDS arrays of the row-list finishing code (roughly LXmax + 2 * LYmax > 36 000) — without MPCGPU_EA_WIDE=1
 * every pair is narrow (mpcgpu_align_pairs takes such pairs); with it, only under a MPCGPU_EA_WIDE_MIN above its default. */
int mpcgpu_ea_scores(mpcgpu_ctx *ctx, uint64_t npairs, const uint32_t *seq1, const uint32_t *seq2, float *ea);
/* The last mpcgpu_ea_scores call: out[0] pairs, out[1] batches, out[2] batches that were redone with a larger candidate room, out[3] launches
 * of post_ea_kernel and post_wide_ea_kernel (batches + redone batches): totals over the narrow and the wide pairs. All 0 before the first
 * call; a refused call leaves them. */
int mpcgpu_ea_info(mpcgpu_ctx *ctx, uint64_t out[4]);
/* ... and what of it went through post_wide_ea_kernel: out[0] wide pairs, out[1] their batches, out[2] those redone with a larger candidate
 * room, out[3] launches of post_wide_ea_kernel. All 0 when no pair was wide. */
int mpcgpu_ea_wide_info(mpcgpu_ctx *ctx, uint64_t out[4]);

/* ---- several GPUs of one node inside ONE process (muscle_amd/csrc/mpcgpu_group.cpp) --------------------------
 * The drop-in binary is one process; it consumes the multi-GPU path through these calls. A group owns one context per
 * listed device (an ordinal may repeat: two contexts on one device is how the tests run this on a one-GPU box), shards
 * the pair loops of MPCFlat::CalcPosteriors (mpcflat.cpp:239-251) and MPCFlat::ConsIter (consflat.cpp:5-23) over them
 * (contiguous pair ranges balanced by DP cells) and performs the two exchanges itself: the all-gather of the packed
 * sparse posteriors before relax and the all-gather of the new probabilities after each iteration — RCCL point-to-point
 * sends/receives over xGMI with exact sizes when the devices are distinct and librccl loads (transport "rccl"), peer
 * copies otherwise ("peer"; MPCGPU_GROUP_TRANSPORT=peer|rccl forces one). After group_calc_posteriors every context
 * holds the full store, so the host reads results (EA, matrices, mpcgpu_align_alns ...) from mpcgpu_group_ctx(g, 0). */
typedef struct mpcgpu_group mpcgpu_group;
int mpcgpu_group_create(mpcgpu_group **out, uint32_t ndev, const int *device_ordinals);
void mpcgpu_group_destroy(mpcgpu_group *g);
const char *mpcgpu_group_last_error(const mpcgpu_group *g); /* g may be NULL: last create() error */
uint32_t mpcgpu_group_size(const mpcgpu_group *g);
mpcgpu_ctx *mpcgpu_group_ctx(mpcgpu_group *g, uint32_t rank);
const char *mpcgpu_group_transport(const mpcgpu_group *g); /* "rccl" or "peer" */
/* mpcgpu_set_hmm / mpcgpu_set_seqs / mpcgpu_set_mega on every context */
int mpcgpu_group_set_hmm(mpcgpu_group *g, const float start[5], const float trans[25], const float match[256 * 256],
                         const float ins[256], float min_sparse_score, int expf_variant);
int mpcgpu_group_set_seqs(mpcgpu_group *g, uint32_t n, const uint8_t *const *seqs, const uint32_t *lens);
int mpcgpu_group_set_mega(mpcgpu_group *g, uint32_t nfeat, const uint32_t *alpha, const float *weight,
                          const float *const *logprobs, const float *const *logprob_mx, const uint8_t *const *profiles);
/* MPCFlat::CalcPosteriors for all pairs: stage A sharded, all-gather, store built on every device. */
int mpcgpu_group_calc_posteriors(mpcgpu_group *g);
/* One MPCFlat::ConsIter: relax sharded, all-gather of the values, commit on every device. */
int mpcgpu_group_cons_iter(mpcgpu_group *g);

/* ---- measurement hooks (bench.py) --------------------------------------------------------- */
/* Kernel time in ms measured with hipEvents on the library's own stream, accumulated since the
 * last reset, per kernel family: 0 = fwd/bwd (fb), 1 = posterior finish (sort/EA/pack),
 * 2 = store build, 3 = relax, 4 = commit/scatter; and launches counted per family. */
#define MPCGPU_NKERNELS 9 /* ... 5 = BuildPost record generation, 6 = BuildPost grouping (sort), 7 = BuildPost in-order reduction,
                             8 = CalcAlnFlat + traceback (families 5-8: mpcgpu_align_alns / mpcgpu_align_msas / mpcgpu_calc_aln) */
int mpcgpu_timers_reset(mpcgpu_ctx *ctx);
/* Timing on (default) / off. Off: no hipEvents around the launches (two events per launch family and call are a measurable share
 * of a small join: the drop-in switches them off unless MUSCLE_GPU_TIMING asks for the report); mpcgpu_timers_get then reports
 * what was measured while it was on. */
int mpcgpu_timers_enable(mpcgpu_ctx *ctx, int on);
int mpcgpu_timers_get(mpcgpu_ctx *ctx, float ms[MPCGPU_NKERNELS], uint64_t launches[MPCGPU_NKERNELS]);
/* Algorithmic work of the last calc_posteriors call: DP cells summed over pairs
 * (sum (LX+1)(LY+1)) and of the last cons_iter: (pair,Z) triples and stored entries. */
int mpcgpu_work_get(mpcgpu_ctx *ctx, uint64_t *dp_cells, uint64_t *relax_entry_z, uint64_t *store_entries);
/* How the last stage A (mpcgpu_calc_posteriors / a pair-list call) ran its forward/backward sweeps: pairs in all, pairs that
 * ran as members of chains (consecutive pairs with the same row sequence swept back to back by one wavefront, no systolic
 * fill/drain in between: kernels_fbc.h), and the number of chains. Same cells, same results; MPCGPU_FB_CHAIN=0 turns chains off.
 * With structure profiles loaded (mpcgpu_set_mega) the chains run in fb_chain_mega_kernel<H>, the chain kernel with the emissions of
 * fb_kernel<H, true>, bin by bin (H rows per lane = rows of the row sequence / 64, rounded up) under MPCGPU_FB_CHAIN_MEGA: 0 = never
 * (every pair alone in fb_kernel<H, true>), 1 = wherever the kernel launches, 2 = the rule: in bin H only where fb_chain_mega_kernel<H>
 * is resident on a CU at least as often as fb_kernel<H, true> (the runtime's occupancy at the launch's workgroup size and LDS) and
 * uses no scratch memory. Unset is 0 (the kernel is opt-in until its device time is on record). */
int mpcgpu_stage_a_info(mpcgpu_ctx *ctx, uint64_t *pairs, uint64_t *chained_pairs, uint64_t *chains);
/* bins: bit H set = the last stage A ran the pairs of bin H (H rows per lane) that can chain through the chain kernel (fb_chain_kernel,
 * fb_chain_post_kernel or, with structure profiles, fb_chain_mega_kernel), chains of one pair included; 0 when every pair ran in fb_kernel
 * or the row-block kernels. The bins of mpcgpu_stage_a_fuse_info are a subset. */
int mpcgpu_stage_a_chain_bins(mpcgpu_ctx *ctx, uint32_t *bins);
/* How the last stage A ran the pairs whose row sequence is cut into row blocks (769 residues or more: CalcFwdFlat, fwdflat3.cpp:12-153 /
 * CalcBwdFlat, bwdflat3.cpp:10-184 over blocks of 64 x 7 or 64 x 4 rows): pairs = the row-block pairs that ran cooperatively, the
 * wavefronts of a workgroup sweeping the blocks of ONE pair as a pipeline (kernels_fbcoop.h) where otherwise one wavefront walks them
 * one after the other; waves_per_pair = the wavefronts each such pair had. Both 0 when none ran that way. Same cells, same results
 * (the candidates of a pair reach the finishing kernels in another order, which those do not depend on). MPCGPU_FB_COOP: 0 never
 * (also when unset, until the rule has been measured on a device), 1 when a launch has fewer row-block pairs than the chip has wave
 * slots for them, 2..16 that many waves, always (clamped to the waves of a workgroup the chip keeps resident). */
int mpcgpu_stage_a_coop_info(mpcgpu_ctx *ctx, uint64_t *pairs, uint32_t *waves_per_pair);
/* How many pairs of the last stage A were FINISHED inside the sweeps: a wavefront of fb_chain_post_kernel (kernels_fbc.h) that has swept
 * a chain backward runs the row-list finishing code (what post_rows_kernel runs) for the chain's pairs before it takes the next chain,
 * and the finishing launch of the batch is left with the other pairs. bins: bit H set = the chains of the bin of H rows per lane (rows
 * of the row sequence / 64, rounded up) were finished that way. Either pointer may be NULL. Same records, same EA bits. MPCGPU_FB_POST_FUSE: 0 and unset = never,
 * 1 = wherever the workgroup with its finishing slices fits a CU, 2 = where it is as often resident as the plain chain kernel and uses no
 * scratch memory. */
int mpcgpu_stage_a_fuse_info(mpcgpu_ctx *ctx, uint64_t *pairs, uint32_t *bins);
/* How the last finishing launch on this context ran (the kernels behind the sweeps: the expf half of CalcPostFlat,
 * calcposteriorflat.cpp:16-22; MySparseMx::FromPost, mysparsemx.cpp:115-152; CalcAlnScoreFlat, calcalnscoreflat.cpp:4-32; EA,
 * calcposteriorflat.cpp:89), whichever call made it: mpcgpu_calc_posteriors, a pair-list stage (its last batch) or
 * mpcgpu_post_scores. out[0] the kernel: 0 = post_rows_kernel (row lists in LDS), 1 = post_kernel (one wavefront per pair, bitonic
 * sorts), 2 = post_wide_kernel (a workgroup per pair, radix sort); out[1] threads per workgroup; out[2] pairs the launch finished;
 * out[3] radix passes of the row-major sort of the pair with the most candidates (kernel 2; 0 for kernels 0 and 1). All 0 before the
 * first such launch. Same records, same EA bits whichever kernel ran. MPCGPU_POST_WIDE: 0 = never post_wide_kernel, 1 = always (also
 * for lists that fit the row-list kernel; mpcgpu_align_pairs then builds its dense posteriors from the raw candidate lists, as for
 * a list that does not fit), unset = post_kernel for what the row-list kernel does not take. */
int mpcgpu_post_info(mpcgpu_ctx *ctx, uint64_t out[4]);
/* Sizes of the current store, for the measurement's lower bounds (bench.py: min_bytes_per_launch): out[0] bytes of the row-indexed
 * block records, out[1] of the window records (0: not built), out[2] of the packed matrices of all pairs, out[3] stored posteriors
 * of all pairs, out[4] of the pairs this context relaxes, out[5] sequences whose records the store holds (all of them unless the
 * store is partial: mpcgpu_store_import_part). */
int mpcgpu_store_info(mpcgpu_ctx *ctx, uint64_t out[6]);
int mpcgpu_synchronize(mpcgpu_ctx *ctx);
/* Which store layout and relax kernel the current store uses, in words (record sizes, workgroup geometry, the tile shapes
 * once a relax iteration has built them), and whether that is a FALLBACK this build chose because the run exceeds the default
 * layout's limits (sequences longer than 4095, records beyond the CU's LDS ...): bench.py prints it, the drop-in warns. */
int mpcgpu_relax_info(mpcgpu_ctx *ctx, char *buf, uint32_t buflen, int *is_fallback);

#ifdef __cplusplus
}
#endif
#endif /* MPCGPU_H */

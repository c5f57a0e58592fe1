/*
 * nais.h -- C-ABI of the MI355X-native NAIS scoring path (gfx950, libnais_hip.so).
 *
 * The reference (muyeon-jo/POI_recommendation_models) is pure Python + PyTorch and exposes no
 * FFI; the boundary this library replaces is the Python call surface of its NAIS hot path:
 *
 *   nais_forward        replaces NAIS_basic.forward            model.py:40-55  (+ attention_network :57-89)
 *                                NAIS_regionEmbedding.forward   model.py:132-142 (+ :144-180)
 *                                NAIS_region_distance_Embedding.forward model.py:231-244 (+ :246-297)
 *                                NAIS_distance_Embedding.forward model.py:340-353 (+ :355-395)
 *   nais_score_topk     replaces the per-user loop body of      validation.py:11-27 (NAIS_validation),
 *                                                               validation.py:38-55 (NAIS_region_validation),
 *                                                               validation.py:69-127 (NAIS_region_distance_validation,
 *                                                               also run with NAIS_distance_Embedding, run.py:431)
 *                       i.e. get_NAIS_batch_test* (batches.py:52-65, 110-139) + chunked forward + torch.topk
 *   nais_gather_rows    the embedding gather of model.py:64 (nn.Embedding -> index_select) as a standalone
 *                       HBM-roofline kernel
 *   nais_train_*        one NAIS_basic training step (run.py:91-109): train-mode forward with dropout
 *                       (model.py:22,40-89), backward of the attention pooling, dense embedding grads;
 *                       nais_adagrad* = torch.optim.Adagrad's update (run.py:89)
 *
 * Conventions: every pointer is caller-owned DEVICE memory (e.g. torch tensor.data_ptr()); the library
 * never allocates, frees or copies caller memory, never synchronises, and issues all work on `stream`
 * (a hipStream_t; NULL = legacy default stream). Calls are asynchronous and stream-ordered.
 * Scratch memory comes from a caller-supplied workspace sized by the matching *_workspace_size().
 * Return value: 0 on success, < 0 on error (see NAIS_E_*); nais_last_error() then describes it
 * (thread-local). All arithmetic is IEEE fp32 (fp64 for coordinates), as in the reference.
 */
#ifndef NAIS_H_
#define NAIS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NAIS_ABI_VERSION 23   /* still 23 with the New2 model (nais_new2_forward, nais_new2_score_topk, nais_new2_score_topk_workspace_size, nais_new2_params_t): new entry points and one new struct only, no existing layout or behaviour moves, so the number did not change; 23: New1 training (nais_new1_make_train_batch, nais_new1_train_step, nais_new1_train_step_workspace_size; additive); 22: the New1 model (nais_new1_forward, nais_new1_catalog_tables, nais_new1_score_topk, nais_new1_score_topk_workspace_size; additive); 21: the BPR model (nais_bpr_forward, nais_bpr_score_topk, nais_bpr_score_topk_workspace_size, nais_bpr_make_train_batch, nais_bpr_train_step, nais_bpr_train_step_workspace_size; additive); 20: block-scaled 16-bit pair words for the bounded gather ("q16": nais_pair_table_bound1_q16_queued, nais_pair_bound_topk_q16, nais_q16_pitch; additive); 19: GeoIE training (nais_geoie_make_train_batch, nais_geoie_train_step, nais_geoie_train_step_workspace_size, nais_sgd; additive); 18: the GeoIE model (nais_geoie_table, nais_geoie_score, nais_geoie_forward; additive); 17: nais_pair_table_bound1_queued (the bound table with one f16 product per attention-logit term; additive); 16: nais_pair_table_bound_queued (the 3-product bound table as a work queue; additive), and the item-side fp16x3 table kernel takes nais_pair_table's / nais_pair_table_split's work counter too (as does fp16x6 at embed_dim 16, the same kernel); 15: on-demand exact refine of the bounded gather (nais_pair_table_bound, nais_pair_scales, nais_pair_bound_topk_widened, nais_pair_refine_topk_exact, nais_pair_recompute; additive); 14: nais_pair_bound_topk / nais_pair_refine_topk take the optional per-entry table rows and per-slot history spans; 13: split16 pair tables, bounded gather + exact refine (nais_pair_table_split, nais_pair_bound_topk, nais_pair_refine_topk); 12: any embed_dim <= 256 and any hidden (generic-shape kernels); 11: hidden up to 256 (fp16x6 scoring, nais_forward), any variant on the x6n kernel */

/* model variants */
#define NAIS_VARIANT_BASIC 0           /* NAIS_basic                      model.py:8-97    */
#define NAIS_VARIANT_REGION 1          /* NAIS_regionEmbedding            model.py:99-187  */
#define NAIS_VARIANT_REGION_DISTANCE 2 /* NAIS_region_distance_Embedding  model.py:189-304 */
#define NAIS_VARIANT_DISTANCE 3        /* NAIS_distance_Embedding         model.py:306-408 */

/* arithmetic of the W1 x products in the catalog scorer (nais_score_topk / nais_score_catalog) */
#define NAIS_PRECISION_FP32 0          /* v_mfma_f32_32x32x2_f32: exact fp32 (k-ordered fmaf chain)           */
#define NAIS_PRECISION_FP16X3 1        /* v_mfma_f32_32x32x16_f16 on power-of-two-scaled hi/lo fp16 splits:
                                          3 products per fp32 product, fp32 accumulate, ~2^-21 relative;
                                          operands A_j = W1 diag(h_j) (split once per item) and t_c     */
#define NAIS_PRECISION_FP16X3_PAIRSPLIT 2 /* same arithmetic class, splitting x = h_j (.) t_c per pair
                                          (the reference's operand order; more VALU work)                 */
#define NAIS_PRECISION_FP16X6 3        /* fp32-faithful split (the default): hi/mid/lo fp16 pieces hold
                                          every operand exactly, 6 f16 MFMA products per fp32 product
                                          (dropped terms <= ~2^-33 relative, below fp32's 2^-24 product
                                          rounding), fp32 accumulate; item-side operands as FP16X3     */
#define NAIS_PRECISION_FP16X6_PAIRSPLIT 4 /* FP16X6 arithmetic on the per-pair split of x = h_j (.) t_c */

/* flags for nais_forward */
#define NAIS_FLAG_SIGMOID 1            /* apply sigmoid (model.py:55); else return the logits of attention_network */

/* error codes */
#define NAIS_OK 0
#define NAIS_E_INVALID (-1)            /* bad pointer / shape / dtype-implied size */
#define NAIS_E_UNSUPPORTED (-2)        /* a dimension outside the compiled kernel set */
#define NAIS_E_HIP (-3)                /* a HIP runtime error while launching */
#define NAIS_E_WORKSPACE (-4)          /* workspace missing or too small */

/*
 * Parameters of one NAIS model: device pointers to the reference's nn.Module parameters
 * (state_dict names in comments) plus their dimensions. Shapes (the reference builds
 * Linear(embed_size, hidden_size) for any sizes, model.py:9-38): embed_dim 1..256, hidden >= 1,
 * every entry point. The tuned kernels are compiled for embed_dim in {8, 16, 32, 64, 128} and
 * hidden <= 256 (scoring at precision FP16X6 with embed_dim 32 / 64 / 128, and nais_forward;
 * <= 128 for the other catalog precisions); every other shape runs the generic-shape kernels
 * (exact fp32 whatever the precision; nais_generic.hip) -- a caller with a width < 128 off that
 * set may instead zero-pad the tables (each half of the region variants' rows separately) and
 * attn_layer1's columns to the next native width for the tuned kernels (exact; the Python drop-in
 * does, model._NAISDevice._score_params). Training: the tuned / general kernels up to 128, the
 * generic-shape ones above. embed_dim > 256 is NAIS_E_UNSUPPORTED (the LDS budget).
 */
typedef struct nais_params {
  int32_t variant;              /* NAIS_VARIANT_* */
  int32_t embed_dim;            /* D: width of h_j (.) t (embed_size in every variant)                 */
  int32_t item_dim;             /* columns of embed_history/embed_target: D (basic, distance), D/2 (region*) */
  int32_t region_dim;           /* columns of embed_region: D/2 (region*), 0 (basic, distance)         */
  int32_t hidden;               /* H = attn_layer1.out_features (1..256, see above)                    */
  int32_t din;                  /* attn_layer1.in_features: D, or D+2 for region_distance / distance   */
  int64_t num_pois;             /* P = rows of embed_history / embed_target                            */
  int64_t num_regions;          /* R = rows of embed_region (0 for basic)                              */
  float beta;                   /* attention smoothing exponent (model.py:80), 0.5 in every driver     */
  int32_t precision;            /* NAIS_PRECISION_* (catalog scorer; nais_forward is always fp32)      */
  const float* embed_history;   /* embed_history.weight [P, item_dim]        model.py:15,106,198      */
  const float* embed_target;    /* embed_target.weight  [P, item_dim]        model.py:16,107,199      */
  const float* embed_region;    /* embed_region.weight  [R, region_dim]|NULL model.py:109,203         */
  const float* w1;              /* attn_layer1.weight   [H, din]             model.py:25,116,212      */
  const float* b1;              /* attn_layer1.bias     [H]                                           */
  const float* w2;              /* attn_layer2.weight   [1, H]               model.py:26,117,213      */
  const float* dist_w;          /* dist_layer.weight    [2, 2] | NULL        model.py:215             */
  const float* dist_b;          /* dist_layer.bias      [2]    | NULL                                 */
} nais_params_t;

/* Optional power-law geo prior blended into the catalog scores before the top-k (powerLaw.py:86-92,
 * run.py:55-59, run.py:537-539): G(u,c) = prod_j a*max(0.01, dist(coo_j, coo_c))^b (float64, history in
 * CSR order), G_norm = G / max_c G (unless the max is 0), score' = f32((1-alpha)*score) + alpha*G_norm
 * (float64), ranked on score'. out_scores then carries score' rounded to float32. */
typedef struct nais_prior {
  double a, b, alpha;
  const double* coords;         /* [P, 2] (lat, lng) float64 */
} nais_prior_t;

/* ABI version of the loaded library (== NAIS_ABI_VERSION it was built with). */
int32_t nais_abi_version(void);

/* Thread-local description of the last error returned by this thread. */
const char* nais_last_error(void);

/*
 * General forward (any per-row histories): for row r in [0,b) with history hist[r*hist_ld + j],
 * j in [0,n), and target item target[r], write out[r] = sigmoid(logit) (flags & NAIS_FLAG_SIGMOID)
 * or the logit of attention_network, exactly as model.py:57-89 (mask model.py:92-95, no
 * max-subtraction, beta-smoothed denominator). n == 0 gives logit 0.
 *   hist_region [b, n] (row stride hist_region_ld), target_region [b]: region variants only.
 *   target_lat_long [b, n, 2] f32 (row stride latlon_ld, in elements): region_distance and
 *   distance, = (|lat_c - lat_j|, |lng_c - lng_j|) as built at run.py:47-54 / validation.py:108-118;
 *   the kernels scale it x100 (model.py:265) or x1000 (distance, model.py:369) before dist_layer.
 *   nan_count (may be NULL): device int32, atomically incremented by the number of NaN logits
 *   (model.py:50-54 prints this count).
 */
int32_t nais_forward(const nais_params_t* params,
                     const int64_t* hist, int64_t b, int64_t n, int64_t hist_ld,
                     const int64_t* target,
                     const int64_t* hist_region, int64_t hist_region_ld,
                     const int64_t* target_region,
                     const float* target_lat_long, int64_t latlon_ld,
                     float* out, int32_t* nan_count, int32_t flags, void* stream);

/*
 * Full-catalog scoring + top-k for a list of users (validation.py:11-27 per-user body):
 * candidates of user u are every POI not in its training history
 *   indices[indptr[u] .. indptr[u+1])   (CSR of train_matrix, batches.py:55-56),
 * each scored with the variant's forward (sigmoid), then the k best are returned ordered by
 * (score desc, POI id asc); NaN ranks first (torch.topk semantics).
 *   users[i] (i < num_users): user ids to score; out_ids / out_scores are [num_users, k].
 *   region_of [P] int64: POI -> region (businessRegionEmbedList, run.py:149-152), region variants.
 *   coords [P, 2] float64 (lat, lng): (region_)distance -- (|dlat|, |dlng|) formed on the fly in
 *   float64, bit-identical to run.py:47-54. latlon_mat [P, P, 2] float64: the reference's own
 *   matrix (run.py:214), read instead when coords is NULL (feasible only for small P).
 *   k <= 1024 and every user needs at least k candidates (torch.topk raises otherwise; the
 *   caller checks -- the kernel writes id -1 / NaN for missing slots and counts them in *short_count).
 *   nan_count / short_count (device int32, may be NULL) are atomically incremented.
 */
size_t nais_score_topk_workspace_size(const nais_params_t* params, int32_t num_users, int32_t k,
                                      int32_t with_prior);
int32_t nais_score_topk(const nais_params_t* params,
                        const int64_t* indptr, const int64_t* indices,
                        const int32_t* users, int32_t num_users, int32_t k,
                        const int64_t* region_of, const double* coords,
                        const double* latlon_mat, const nais_prior_t* prior,
                        int32_t* out_ids, float* out_scores,
                        int32_t* nan_count, int32_t* short_count,
                        void* workspace, size_t workspace_bytes, void* stream);

/*
 * Scores only (the first half of nais_score_topk): scores[i * score_ld + c] = sigmoid score of POI c
 * for user users[i], c in [0, P); POIs in the user's history are written as -1.0f (they are not
 * candidates, batches.py:56). score_ld >= P. Used for parity tests and by callers that post-process
 * the full score row (e.g. the geo-prior blend).
 */
int32_t nais_score_catalog(const nais_params_t* params,
                           const int64_t* indptr, const int64_t* indices,
                           const int32_t* users, int32_t num_users,
                           const int64_t* region_of, const double* coords, const double* latlon_mat,
                           float* scores, int64_t score_ld, int32_t* nan_count, void* stream);

/*
 * Power-law prior rows (powerLaw.py:90-92): out[i * out_ld + c] = prod_j pr_d(dist(coo_j, coo_c)) for user
 * users[i], c in [0, P), float64 in the reference's operation order; history POIs get -1. out_max[i] =
 * max over the user's candidates (the normalize() divisor of run.py:55-59). coords [P, 2] float64.
 */
int32_t nais_powerlaw_prior(const double* coords, int64_t num_pois, const int64_t* indptr,
                            const int64_t* indices, const int32_t* users, int32_t num_users, double a,
                            double b, double* out, int64_t out_ld, double* out_max, void* stream);

/*
 * Pair-distance histogram for PowerLaw.fit_distance_distribution (powerLaw.py:41-55): hist[bin] = number of
 * pairs i < j within a user's history (all num_users users) with int(dist) == bin (km); pairs with
 * dist >= nbins or NaN are counted in *overflow. Both outputs are zeroed by the call.
 */
int32_t nais_distance_histogram(const double* coords, const int64_t* indptr, const int64_t* indices,
                                int64_t num_users, uint64_t* hist, int64_t nbins, uint64_t* overflow,
                                void* stream);

/*
 * Top-k of score rows (the second half of nais_score_topk): for row i in [0, num_rows), the k largest
 * entries of scores[i * score_ld + c], c in [0, P), ignoring negative entries (non-candidates), ordered
 * (score desc, c asc), NaN first -> out_ids / out_scores [num_rows, k]. k <= 1024.
 */
int32_t nais_topk_rows(const float* scores, int64_t score_ld, int64_t num_pois, int32_t num_rows,
                       int32_t k, int32_t* out_ids, float* out_scores, int32_t* short_count,
                       void* stream);

/*
 * Standalone embedding-row gather (model.py:64, nn.Embedding): out[i, :] = table[idx[i], :],
 * table [rows, dim] f32 row-major, idx [m] int64 (caller guarantees 0 <= idx < rows).
 */
int32_t nais_gather_rows(const float* table, int64_t rows, int32_t dim,
                         const int64_t* idx, int64_t m, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * "Pairs" strategy of the full-catalog loop (validation.py:11-27). Every term of a user's score
 * for history item j and candidate c depends on (j, c) only (model.py:57-89), so a user list's
 * scores can be formed from two per-pair tables computed ONCE for the list's distinct history
 * items instead of once per user:
 *   nais_pair_rows     items[0 .. *num_items) = distinct history POIs of users[] (ascending),
 *                      rowmap[P] = row of each POI in items[] or -1. Workspace:
 *                      nais_pair_rows_workspace_size(P) bytes. *num_items is device memory.
 *   nais_pair_table    for item rows r < num_items and candidates c in [col0, col0 + cols):
 *                      e[r*ld + c-col0] = exp(a_rc) * [items[r] != c],  es[...] = e * (h_r . t_c),
 *                      with the catalog kernels' arithmetic for params->precision (split-fp16
 *                      where nais_score_catalog uses the fused split kernel, else exact fp32).
 *   nais_pair_gather   for every user and c in [col0, col0 + cols): N = sum_j es[row(j), c],
 *                      S = sum_j e[row(j), c] over the user's history in CSR order,
 *                      scores[slot*score_ld + c - score_col0] = sigmoid(N / S^beta) (history
 *                      POIs = -1, empty history = 0.5; score_col0 = the POI of column 0 of
 *                      scores, 0 for full rows); NaNs counted into *nan_count as
 *                      nais_score_catalog does.
 * The caller loops over column blocks sized to its memory budget and runs nais_topk_rows.
 *   work (nais_pair_table, nais_pair_gather_topk; may be NULL): one int32 of device memory private
 *                      to the stream. Given, the launch runs as a work queue -- about one
 *                      resident round of workgroups takes (item group, column tile) or user slots
 *                      from this counter (zeroed by the call, stream-ordered) until they run out,
 *                      so a CU-masked stream whose CU count is not a multiple of the shader-engine
 *                      count still uses every CU (the table calls: the 16x16x32 fp16x6 kernel
 *                      and, since ABI 16, the item-side split-fp16 kernel -- precision fp16x3, and
 *                      fp16x6 at embed_dim 16 -- for the variants without distance inputs; other
 *                      shapes and precisions ignore it). Results are identical either way.
 *   nais_pair_gather_topk  the same sums and scores, but instead of score rows each user keeps a
 *                      running top-k: keys[slot*k ..] (uint64, sorted descending, kcount[slot]
 *                      valid; zero kcount before the first call) with key = ordered(score) << 32 |
 *                      (0xFFFFFFFF - poi), i.e. torch.topk's (score desc) with ties by POI id asc
 *                      and NaN first; history POIs are never candidates. Columns of one call may
 *                      be any block; the calls of one user list must be stream-ordered. k <= 256.
 *   nais_topk_keys_finish  keys -> out_ids / out_scores [num_users, k] (short lists padded with
 *                      -1 / NaN and counted into *short_count), as nais_topk_rows reports them.
 */
size_t nais_pair_rows_workspace_size(int64_t num_pois);
int32_t nais_pair_rows(const int64_t* indptr, const int64_t* indices, const int32_t* users,
                       int32_t num_users, int64_t num_pois, int32_t* rowmap, int64_t* items,
                       int64_t* num_items, void* workspace, size_t workspace_bytes, void* stream);
int32_t nais_pair_table(const nais_params_t* params, const int64_t* items, int64_t num_items,
                        int64_t col0, int64_t cols, const int64_t* region_of,
                        const double* coords, const double* latlon_mat, float* e, float* es,
                        int64_t ld, int32_t* work, void* stream);
int32_t nais_pair_gather(const float* e, const float* es, int64_t ld, const int32_t* rowmap,
                         const int64_t* indptr, const int64_t* indices, const int32_t* users,
                         int32_t num_users, int64_t col0, int64_t cols, float beta, float* scores,
                         int64_t score_ld, int64_t score_col0, int32_t* nan_count, void* stream);
int32_t nais_pair_gather_topk(const float* e, const float* es, int64_t ld, const int32_t* rowmap,
                              const int64_t* indptr, const int64_t* indices, const int32_t* users,
                              int32_t num_users, int64_t col0, int64_t cols, float beta, int32_t k,
                              uint64_t* keys, int32_t* kcount, int32_t* nan_count, int32_t* work,
                              void* stream);
int32_t nais_topk_keys_finish(const uint64_t* keys, const int32_t* kcount, int32_t num_users, int32_t k,
                              int32_t* out_ids, float* out_scores, int32_t* short_count, void* stream);
/*
 * Bounded gather + exact refine (filter-and-refine top-k; DESIGN.md (d) "bounded gather"): the
 * lists of nais_pair_gather_topk -- the same ids and score bits -- from half the gathered bytes.
 *   nais_pair_table_split  nais_pair_table's pairs stored split16: hi[r*ld + c-col0] = (top 16 bits
 *                      of e*s) << 16 | (top 16 bits of e) -- both values truncated to 8 significant
 *                      bits -- and ex[2*(r*ld + c-col0)] = e, ex[... + 1] = e*s (the exact pair,
 *                      8 bytes side by side; ex row pitch 2*ld).
 *   nais_pair_bound_topk   per column block (stream-ordered over the blocks of one user list): each
 *                      user's S, N = sum over its history of the truncated e, e*s and sum |e*s| give
 *                      an interval around every candidate's exact score (the fp32 arithmetic of
 *                      nais_pair_gather_topk on the untruncated pairs); lo_keys[slot*k ..] / lo_count
 *                      keep the k best lower bounds (zero lo_count before the first block), and the
 *                      key (upper bound, id) of every candidate whose upper bound reaches the k-th
 *                      lower bound so far is appended to surv[slot*surv_cap ..] (surv_count[slot];
 *                      zero it before the first block; compacted when full, -1 if it overflows).
 *                      Keys as nais_pair_gather_topk. ld % 4 == 0, hi 16-byte aligned, k <= 256.
 *   nais_pair_refine_topk  after the last block: for each survivor whose upper key reaches the final
 *                      k-th lower key (every column for an overflowed user), the exact N, S from the
 *                      ex pairs in history (CSR) order and its score; keys / kcount receive the top-k
 *                      exactly as nais_pair_gather_topk leaves them (NaNs counted into *nan_count).
 *                      ex: block b (columns col0 + b*block_cols ..) at ex + b*block_stride (uint32
 *                      words, even), rows of ld pairs (nais_pair_table_split's ex). stats (may be
 *                      NULL): stats[0] += candidates refined, stats[1] += overflowed users. tau (may
 *                      be NULL): per user a threshold key to use when larger than its own k-th lower
 *                      key -- a column shard of a process group passes the k-th lower key over ALL
 *                      shards (exchanged after the last block) and then returns only its candidates
 *                      that can reach the global top-k: kcount may be < k (padding as short lists).
 *                      A column shard's k-th lower key is a lower bound of the global k-th exact key,
 *                      so every global winner on this shard is still returned.
 *   entry_rows (both; may be NULL): entry_rows[e] = rowmap[indices[e]] for every CSR entry e of the
 *                      listed users -- the table row of each history entry, read beside its POI id
 *                      instead of after it. spans (nais_pair_bound_topk; may be NULL):
 *                      spans[2*s] = indptr[users[s]], spans[2*s+1] = the history length of users[s]
 *                      -- one load per slot instead of two in a row. Both only shorten the chains
 *                      of dependent loads (ABI 14); the results are the same with or without them.
 */
int32_t nais_pair_table_split(const nais_params_t* params, const int64_t* items, int64_t num_items,
                              int64_t col0, int64_t cols, const int64_t* region_of,
                              const double* coords, const double* latlon_mat, uint32_t* hi,
                              uint32_t* ex, int64_t ld, int32_t* work, void* stream);
int32_t nais_pair_bound_topk(const uint32_t* hi, int64_t ld, const int32_t* rowmap,
                             const int64_t* indptr, const int64_t* indices, const int32_t* users,
                             int32_t num_users, int64_t col0, int64_t cols, float beta, int32_t k,
                             uint64_t* lo_keys, int32_t* lo_count, uint64_t* surv, int32_t* surv_count,
                             int32_t surv_cap, const int32_t* entry_rows, const int64_t* spans,
                             int32_t* work, void* stream);
int32_t nais_pair_refine_topk(const uint32_t* ex, int64_t block_stride,
                              int64_t ld, int64_t block_cols, const int32_t* rowmap,
                              const int64_t* indptr, const int64_t* indices, const int32_t* users,
                              int32_t num_users, int64_t col0, int64_t cols, float beta, int32_t k,
                              const uint64_t* lo_keys, const int32_t* lo_count, const uint64_t* surv,
                              const int32_t* surv_count, int32_t surv_cap, const uint64_t* tau,
                              uint64_t* keys, int32_t* kcount, int32_t* nan_count, int32_t* stats,
                              const int32_t* entry_rows, void* stream);
/*
 * On-demand exact refine (ABI 15; DESIGN.md (d) "3-product bound, on-demand refine"): the bounded
 * gather needs only 8 significant bits of every pair, and the refine reads the exact pair of a few
 * dozen candidates per user, so the pair table need neither be fp32-faithful nor stay resident.
 * The table stream writes hi words alone from the 3-product (fp16x3) kernels, the gather widens
 * its intervals by a bound on the difference between that arithmetic and fp16x6, and the refine
 * RECOMPUTES each surviving (history item, candidate) pair with the bits the fp16x6 table of the
 * same job would hold. Same lists, ids and score bits as nais_pair_gather_topk on fp16x6 tables.
 *   nais_pair_table_bound  the hi words of nais_pair_table_split at precision fp16x3 (same layout
 *                      and bits), whatever params->precision says; no (e, e*s) pairs are stored.
 *                      Native embed widths with hidden <= 128 (NAIS_E_UNSUPPORTED otherwise).
 *   nais_pair_table_bound_queued  (ABI 16) the same table with nais_pair_table's `work` counter
 *                      (above; zeroed by the call, stream-ordered): the item-side 3-product kernel
 *                      then runs as a work queue, so the table stream's CU count may be any number.
 *                      Every word equals nais_pair_table_bound's, which is this call with work = NULL.
 *   nais_pair_table_bound1_queued  (ABI 17) hi words of the one-product-logit table; s as in
 *                      nais_pair_table_bound. The attention logit of each pair takes one f16
 *                      product per term (hi * hi of the same scaled operands) instead of three, so
 *                      e = exp(a) carries a relative error near 2^-10 of the logit's terms where
 *                      nais_pair_table_bound's carries 2^-21; s = h . t keeps the three products
 *                      and the bits it has there, and e * s is their fp32 product. Same arguments;
 *                      work = NULL selects the fixed grid, whose words equal the queued ones. The
 *                      gather must widen by the one-product bound (catalog.ondemand_widening with
 *                      products = 1). NAIS_basic, embed_dim 32 or 64, hidden <= 64
 *                      (NAIS_E_UNSUPPORTED otherwise).
 *   nais_pair_bound_topk_widened  nais_pair_bound_topk with widen = {eta, delta_s} (device floats;
 *                      NULL or zeros: nais_pair_bound_topk exactly): every exact e lies within
 *                      [1 - eta, 1 + eta] of the e whose truncation the hi word holds, and the two
 *                      arithmetics' s = h . t differ by at most delta_s (absolute). The caller
 *                      derives both from the weights (catalog.ondemand_widening).
 *   nais_pair_scales   the power-of-two operand scales of the fp16x6 pair-table kernel for one job:
 *                      row_scales[2r], [2r+1] = (S_A, S_h) of item row r (its 32-row chunk inside
 *                      its 128-row group of the list), col_scales[c - col0] = S_t of column c (its
 *                      32-column wave tile, counted from the first column of its table block; the
 *                      blocks are block_cols wide from col0). Pure functions of the model and this
 *                      geometry, which must be the one the tables would be built with.
 *   nais_pair_refine_topk_exact  nais_pair_refine_topk without the ex tables: the pair values are
 *                      recomputed from params and the scales. Other arguments as there.
 *   nais_pair_recompute  out_e / out_es [num_rows][num_columns] = the recomputed (e, e*s) of table
 *                      rows rows[] x POI columns columns[] (within [col0, col0 + cols)): the
 *                      refine's arithmetic laid bare, bit-equal to nais_pair_table at fp16x6 for
 *                      the same items, col0-block geometry and scales (tests/test_gpu_ondemand_refine.py).
 * Shapes of the last three: NAIS_basic at precision fp16x6, embed_dim 32 or 64, hidden <= 64
 * (NAIS_E_UNSUPPORTED otherwise; the caller keeps the split16 route).
 *
 * "q16" (ABI 20; DESIGN.md (d) "Block-scaled 16-bit pair words"): the one-product bound table in
 * 16-bit pair words with one scale pair per (row, 16 columns) -- 1152 bytes per 512-column row
 * where the hi words take 2048. One buffer per table block; row r starts at byte r * pitch,
 *   pitch = nais_q16_pitch(ld) = 4 * ceil(ld / 16) + 2 * ld, rounded up to 128  (ld = 512: 1152).
 * A row holds ceil(ld / 16) scale words (uint32: bits 31..16 = q_s, bits 15..0 = q_e, each the top
 * 16 bits of a non-negative fp32, the low 16 read as 0), then ld pair words (uint16: low byte m_e
 * in 0..255, high byte m_s + 128 with m_s in -128..127). Column x of the block belongs to group
 * x / 16. For the pair values (e, p = e * s) nais_pair_table_bound1_queued computes:
 *   (m_e - 2^-14) q_e <= e < (m_e + 1 + 2^-14) q_e,   (m_s - 2^-14) q_s <= p < (m_s + 1 + 2^-14) q_s
 * (the 2^-14, in units of the scale, is the slack of the quantiser's v_rcp_f32 and one fp32
 * rounding on a quotient below 256; the gather's margins hold it).
 * Scales: with M_e = the largest e and M_s the largest |p| over the group's columns inside the
 * launch's [col0, col0 + cols) (a ragged last group counts its valid columns only), q_e is
 * M_e / 255 and q_s is M_s / 127, each times (1 + 2^-7)(1 + 2^-13) and truncated to 16 bits: no
 * less than the quotient and less than (1 + 2^-6) of it. A quotient below 2^-100 gets the scale
 * 2^-100 (below fp32's normal range the 16 bits no longer resolve 2^-6 and the reciprocal
 * overflows; the contract above holds all the same, and pairs that small bound nothing under the
 * hi words either once their sum leaves the normal range); an all-zero group stores scale 0 and
 * the words 0 / 128; a group with a NaN or an infinity stores a non-finite scale (its words are
 * then meaningless, and the gather refines every candidate whose sums touch it). Pair words past
 * `cols` and the scale words of groups wholly past it are not written.
 *   nais_pair_table_bound1_q16_queued  nais_pair_table_bound1_queued writing that format: q16 is
 *                      the block [num_items rows], pitch must be nais_q16_pitch(ld). Same kernel,
 *                      same (e, p) before quantisation; work = NULL selects the fixed grid, whose
 *                      bytes equal the queued ones.
 *   nais_pair_bound_topk_q16  nais_pair_bound_topk_widened reading that format. Other arguments,
 *                      lists, survivors and the overflow mark as there; the intervals are wider
 *                      by the quantisation (nais_pairs.hip, make_bounds_q16).
 */
int64_t nais_q16_pitch(int64_t ld);   /* the row pitch above, in bytes (0 for ld <= 0) */
int32_t nais_pair_table_bound1_q16_queued(const nais_params_t* params, const int64_t* items,
                                          int64_t num_items, int64_t col0, int64_t cols,
                                          const int64_t* region_of, const double* coords,
                                          const double* latlon_mat, void* q16, int64_t ld,
                                          int64_t pitch, int32_t* work, void* stream);
int32_t nais_pair_bound_topk_q16(const void* q16, int64_t ld, int64_t pitch, const int32_t* rowmap,
                                 const int64_t* indptr, const int64_t* indices, const int32_t* users,
                                 int32_t num_users, int64_t col0, int64_t cols, float beta, int32_t k,
                                 uint64_t* lo_keys, int32_t* lo_count, uint64_t* surv,
                                 int32_t* surv_count, int32_t surv_cap, const int32_t* entry_rows,
                                 const int64_t* spans, const float* widen, int32_t* work, void* stream);
int32_t nais_pair_table_bound(const nais_params_t* params, const int64_t* items, int64_t num_items,
                              int64_t col0, int64_t cols, const int64_t* region_of,
                              const double* coords, const double* latlon_mat, uint32_t* hi,
                              int64_t ld, void* stream);
int32_t nais_pair_table_bound_queued(const nais_params_t* params, const int64_t* items,
                                     int64_t num_items, int64_t col0, int64_t cols,
                                     const int64_t* region_of, const double* coords,
                                     const double* latlon_mat, uint32_t* hi, int64_t ld,
                                     int32_t* work, void* stream);
int32_t nais_pair_table_bound1_queued(const nais_params_t* params, const int64_t* items,
                                      int64_t num_items, int64_t col0, int64_t cols,
                                      const int64_t* region_of, const double* coords,
                                      const double* latlon_mat, uint32_t* hi, int64_t ld,
                                      int32_t* work, void* stream);
int32_t nais_pair_bound_topk_widened(const uint32_t* hi, int64_t ld, const int32_t* rowmap,
                                     const int64_t* indptr, const int64_t* indices, const int32_t* users,
                                     int32_t num_users, int64_t col0, int64_t cols, float beta, int32_t k,
                                     uint64_t* lo_keys, int32_t* lo_count, uint64_t* surv,
                                     int32_t* surv_count, int32_t surv_cap, const int32_t* entry_rows,
                                     const int64_t* spans, const float* widen, int32_t* work,
                                     void* stream);
int32_t nais_pair_scales(const nais_params_t* params, const int64_t* items, int64_t num_items,
                         int64_t col0, int64_t cols, int64_t block_cols, float* row_scales,
                         float* col_scales, void* stream);
int32_t nais_pair_refine_topk_exact(const nais_params_t* params, const float* row_scales,
                                    const float* col_scales, const int32_t* rowmap, const int64_t* indptr,
                                    const int64_t* indices, const int32_t* users, int32_t num_users,
                                    int64_t col0, int64_t cols, int32_t k, const uint64_t* lo_keys,
                                    const int32_t* lo_count, const uint64_t* surv, const int32_t* surv_count,
                                    int32_t surv_cap, const uint64_t* tau, uint64_t* keys, int32_t* kcount,
                                    int32_t* nan_count, int32_t* stats, const int32_t* entry_rows,
                                    void* stream);
int32_t nais_pair_recompute(const nais_params_t* params, const int64_t* items, int64_t num_items,
                            const float* row_scales, const float* col_scales, int64_t col0, int64_t cols,
                            const int32_t* rows, int64_t num_rows, const int64_t* columns,
                            int64_t num_columns, float* out_e, float* out_es, void* stream);
/*
 * Power-law prior on the pairs route (powerLaw.py:86-92, run.py:537-539; the direct route's
 * nais_score_topk with a prior computes the same G rows per user):
 *   nais_pair_prior_table   pr[r*ld + c-col0] = pr_d(dist(items[r], c)) (float64, powerLaw.py's
 *                           operation order) for r < num_items, c in [col0, col0 + cols).
 *   nais_pair_prior_gather  per user slot and c in [col0, col0 + cols):
 *                           g[slot*g_ld + c-g_col0] = prod_j pr[row(j), c] over the history in CSR
 *                           order (1.0 for an empty history; -1.0 for history POIs) -- the bits of
 *                           nais_powerlaw_prior -- and gmax_bits[slot] = max(gmax_bits[slot], the
 *                           block's largest candidate value) as u64 bits; zero gmax_bits before the
 *                           first block. ld must be a multiple of 4 (32-byte loads).
 *   nais_topk_blend_rows    top-k of f32((1 - alpha) * score) + alpha * g / gmax (float64; history
 *                           POIs, score < 0, excluded) per row, (score desc, id asc), as
 *                           nais_score_topk ranks with a prior; out_scores = the blended score as f32.
 *   nais_topk_blend_rows_f64  the same, and (out_blend != NULL) the f64 blended score of every
 *                           returned candidate (NaN for padding) -- the key a column-sharded job
 *                           merges on.
 *   nais_topk_merge_f64     merge of per-column-block lists: row r's m candidates
 *                           (keys[r*m + i] f64, ids[r*m + i] global POI ids, id < 0 = padding) ->
 *                           the k best by (key desc, id asc), NaN first, as out_ids / out_scores
 *                           (f32) / out_keys (f64, optional). m <= 2048, k <= m.
 */
int32_t nais_pair_prior_table(const double* coords, int64_t num_pois, const int64_t* items,
                              int64_t num_items, int64_t col0, int64_t cols, double a, double b,
                              double* pr, int64_t ld, void* stream);
#define NAIS_PRIOR_FINITE 1   /* flags: every pr entry is finite and >= +0 (a > 0, a * max(0.01, d)^b
                                 finite for every distance): a product that underflowed to +0.0
                                 stays +0.0, so
                                 the gather stops reading a wave's rows once all its columns are 0 */
int32_t nais_pair_prior_gather(const double* pr, int64_t ld, const int32_t* rowmap,
                               const int64_t* indptr, const int64_t* indices, const int32_t* users,
                               int32_t num_users, int64_t col0, int64_t cols, double* g, int64_t g_ld,
                               int64_t g_col0, uint64_t* gmax_bits, int32_t flags, void* stream);
int32_t nais_topk_blend_rows(const float* scores, int64_t score_ld, const double* g, int64_t g_ld,
                             const uint64_t* gmax_bits, int64_t num_pois, int32_t num_rows, int32_t k,
                             double alpha, int32_t* out_ids, float* out_scores, int32_t* short_count,
                             void* stream);
int32_t nais_topk_blend_rows_f64(const float* scores, int64_t score_ld, const double* g, int64_t g_ld,
                                 const uint64_t* gmax_bits, int64_t num_pois, int32_t num_rows, int32_t k,
                                 double alpha, int32_t* out_ids, float* out_scores, double* out_blend,
                                 int32_t* short_count, void* stream);
int32_t nais_topk_merge_f64(const double* keys, const int64_t* ids, int32_t num_rows, int32_t m,
                            int32_t k, int64_t* out_ids, float* out_scores, double* out_keys,
                            void* stream);

/*
 * A stream restricted to the CUs whose bits are set in cu_mask[mask_words] (bit i = CU i), for
 * running an MFMA-bound and an HBM-bound kernel side by side on disjoint CUs (the pairs strategy's
 * table / gather overlap). Destroy with nais_stream_destroy.
 */
int32_t nais_stream_create_cu_mask(const uint32_t* cu_mask, uint32_t mask_words, void** stream);
int32_t nais_stream_destroy(void* stream);

/*
 * New4 family (model.py:1169-1306): the per-POI context tables its forward builds
 * from the near-POI lists before NAIS_basic's attention (self_attention, model.py:1272-1295):
 *   ext_history[p] = [embed_history[p] | result_in[p] | result_out[p]]   [P, embed_size]
 *   ext_target[p]  = [embed_target[p]  | result_out[p] | result_in[p]]   [P, embed_size]
 * embed_history / embed_target [P, embed_size/2], embed_ingoing / embed_outgoing [P, embed_size/4],
 * near_pois [P, num_near] int64 (nearPOI, datasets.py:418). Scoring New4 is then the basic variant
 * (nais_forward / nais_score_topk) with these two tables as embed_history / embed_target.
 */
int32_t nais_new4_tables(const float* embed_history, const float* embed_target,
                         const float* embed_ingoing, const float* embed_outgoing,
                         int64_t num_pois, int32_t embed_size, const int64_t* near_pois,
                         int32_t num_near, float* ext_history, float* ext_target, void* stream);

/*
 * The near-POI pooling every table-based New4-family member runs (New4 / New4_padding /
 * all_in_out / transform_ingoing_outgoing / transform_attn: two pools, model.py:1269-1295,
 * 1551-1566, 1922-1950; nearPOI_embedding / only_area_not_inout: one pool, model.py:1680-1686,
 * 2198-2218; no_POI_emb: two pools of width embed_size/2, model.py:1797-1812). For every p < P:
 *   x_k = kv_src[near[p][k]], q = query_src[near[p][0]]              (rows of width dim)
 *   key_k = wk x_k + bk, val_k = wv x_k + bv, q = wq q + bq         (nn.Linear [dim, dim], [dim];
 *                                                 NULL weight = identity, NULL bias = zero)
 *   out[p * out_ld + c] = (softmax(q . reshape(key, [dim, K]) / sqrt(scale_dim)) @ val)[c]
 * out may point into a column range of a wider row table (out_ld >= dim).
 * nais_copy_columns: dst[p * dst_ld + dst_col0 + c] = src[p * src_ld + c], p < rows, c < dim.
 */
int32_t nais_near_attention(const float* query_src, const float* kv_src, int64_t num_pois,
                            int32_t dim, const int64_t* near_pois, int32_t num_near,
                            const float* wq, const float* bq, const float* wk, const float* bk,
                            const float* wv, const float* bv, float scale_dim, float* out,
                            int64_t out_ld, void* stream);
int32_t nais_copy_columns(const float* src, int64_t src_ld, int64_t rows, int32_t dim, float* dst,
                          int64_t dst_ld, int32_t dst_col0, void* stream);

/*
 * transform_attn (model.py:1959-2098): dot-product attention over New4-layout rows (SURVEY.md
 * 8(f4)). Its query/key/value projections act on one POI row each, so they are per-POI tables:
 *   xh, xt   [P, D]  history / target rows (nais_near_attention + nais_copy_columns, New4 layout)
 *   qt = xt Wq^T + bq, kh = xh Wk^T + bk, vh = xh Wv^T + bv   [P, D]   (nais_linear_rows)
 * and the prediction (model.py:2030-2055) is
 *   logit = sum_j m_j e_j (vh_j . xt_c) / (sum_j m_j e_j)^beta,  e_j = exp(qt_c . kh_j / sqrt(scale_dim))
 * with m_j = [h_j != c]; scale_dim = embed_size (torch.sqrt(torch.tensor(self.embed_size))).
 * nais_dot_forward: out[r] for rows r < b as nais_forward (flags, nan_count). For n == 1 it
 *   restates the reference's shapes exactly: exp_A.squeeze(dim=-1) (model.py:2042) leaves [b] and
 *   the mask broadcast couples all b rows: out_r = m_r s_r S / (m_r S)^beta, S = sum_r' e_r'.
 * nais_dot_pair_table: the pair tables of nais_pair_table for this core (E = e_jc, ES = e_jc s_jc),
 *   consumed by nais_pair_gather unchanged.
 * nais_dot_single_fixup: for the listed users with exactly one history item, overwrite their score
 *   rows with new4_validation's chunk-coupled scores (1024-candidate chunks of the ascending
 *   complement list, validation.py:262-270): score_c = sigmoid(s_c S_k / S_k^beta), S_k the sum of
 *   e over c's chunk. Columns [col0, col0 + cols) of rows laid out as in nais_pair_gather.
 * nais_linear_rows: y[r, :dout] = x[r, :din] W^T + b (nn.Linear; b may be NULL), dout <= 256.
 */
typedef struct nais_dot_tables {
  int32_t embed_dim;            /* D (<= 128)                                                 */
  int64_t num_pois;             /* P                                                          */
  float beta;                   /* 0.5                                                        */
  float scale_dim;              /* logits divide by sqrt(scale_dim) (= embed_size)            */
  const float* xh;              /* [P, D] each                                                */
  const float* xt;
  const float* qt;
  const float* kh;
  const float* vh;
} nais_dot_tables_t;

int32_t nais_linear_rows(const float* x, int64_t x_ld, int64_t rows, int32_t din, const float* w,
                         const float* b, int32_t dout, float* y, int64_t y_ld, void* stream);
int32_t nais_dot_forward(const nais_dot_tables_t* tables, const int64_t* hist, int64_t b, int64_t n,
                         int64_t hist_ld, const int64_t* target, float* out, int32_t* nan_count,
                         int32_t flags, void* stream);
int32_t nais_dot_pair_table(const nais_dot_tables_t* tables, const int64_t* items, int64_t num_items,
                            int64_t col0, int64_t cols, float* e, float* es, int64_t ld,
                            void* stream);
int32_t nais_dot_single_fixup(const nais_dot_tables_t* tables, const int64_t* indptr,
                              const int64_t* indices, const int32_t* users, int64_t num_users,
                              int64_t col0, int64_t cols, float* scores, int64_t score_ld,
                              int64_t score_col0, void* stream);

/*
 * NAIS_region_distance_disentangled_Embedding (model.py:409-541): two attention
 * MLPs (POI rows and region rows, both embed_size wide) with a shared additive distance term
 * d_j = sum_e embed_distance[0][e] * target_distance[r, j]; forward (model.py:446-455) =
 *   sigmoid( sum_j a_j (h_j . t) + rho_j (g_j . g_t) ),
 *   a_j = m_j exp(l_j + d_j) / (sum m exp(l + d))^beta, rho_j likewise with the region MLP.
 * Arguments as nais_forward (regions per entry / per row, target_distance [b, n] f32 with row
 * stride dist_ld = run.py:326-333's target_dist). Eval arithmetic (the model has no dropout).
 * nais_pair_distances: out[r * n + j] = f32(powerLaw.dist(coords[target[r]], coords[hist[j]]))
 *   (haversine km, float64 in the reference's order) -- run.py:326-333 for one batch (one shared
 *   history of n items, b targets); coords [P, 2] (lat, lng) float64.
 * The reference's evaluation call for this model (run.py:353) does not match
 * NAIS_region_distance_validation's signature, so only the forward has a defined meaning.
 */
typedef struct nais_disent_params {
  int32_t embed_dim;            /* D (<= 128)                                                 */
  int32_t hidden;               /* H (<= 128)                                                 */
  int64_t num_pois, num_regions;
  float beta;
  const float* embed_history;   /* [P, D]                                                     */
  const float* embed_target;    /* [P, D]                                                     */
  const float* embed_region;    /* [R, D]                                                     */
  const float* embed_distance;  /* [dist_embed_size, D] (row 0 is read)                       */
  const float* w1;              /* attn_layer1 [H, D], [H]; attn_layer2 [1, H]                */
  const float* b1;
  const float* w2;
  const float* region_w1;       /* region_attn_layer1 [H, D], [H]; region_attn_layer2 [1, H]  */
  const float* region_b1;
  const float* region_w2;
} nais_disent_params_t;

int32_t nais_disent_forward(const nais_disent_params_t* params, const int64_t* hist, int64_t b,
                            int64_t n, int64_t hist_ld, const int64_t* target,
                            const int64_t* hist_region, int64_t hist_region_ld,
                            const int64_t* target_region, const float* target_distance,
                            int64_t dist_ld, float* out, int32_t* nan_count, int32_t flags,
                            void* stream);
int32_t nais_pair_distances(const double* coords, const int64_t* hist, int64_t n,
                            const int64_t* target, int64_t b, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GeoIE (model.py:757-828; DESIGN.md (c) "GeoIE"): for user u with CSR-order history hist[0..h)
 * and candidate c,
 *   Gr[e][j] = flat[e*h + j], flat = the rows GeoInfluence[hist[0..h)] laid end to end (h*D floats):
 *              the reference's reshape([b, -1, h]) of a [b, h, D] gather (model.py:795-798), not a
 *              transpose
 *   S[j]     = sum_e Gr[e][j] * GeoSusceptibility[c][e]                      (model.py:800-802)
 *   f[j]     = a * d_j ** b,  d_j = float32(min(max(0.01, dist(coo_c, coo_hist[j])), 100))
 *              (run.py:40-46 builds the float64 matrix, batches.py:256-267 slices and casts it)
 *   out      = sigmoid(UserPreference[u] . PoiPreference[c] + (sum_j S[j] f[j]) / h)
 * in fp32; a and b are the module's Python floats, used as float32 (torch's scalar operands).
 *
 *   nais_geoie_table    f[r*ld + c-col0] = a * d ** b for item rows r < num_items (items[] and the
 *                       rowmap of nais_pair_rows) and candidates c in [col0, col0 + cols): the
 *                       model's only (history POI, candidate) term, evaluated once per pair of a
 *                       user list instead of once per (user, history entry, candidate). Exactly
 *                       one distance source: coords [P, 2] float64 (lat, lng) -- powerLaw.dist in
 *                       float64 on the device, clamped to [0.01, 100], then cast -- or dist_mat
 *                       [P, P] float64, the caller's run.distance_mat result, read at [c][item]
 *                       and cast (run.py:683, batches.py:256). ld >= cols.
 *   nais_geoie_score    scores[slot*score_ld + c - score_col0] = out for users[slot] and every c in
 *                       [col0, col0 + cols); history POIs are written as -1 (they are not
 *                       candidates, batches.py:250), NaN scores counted into *nan_count (may be
 *                       NULL). Replaces get_GeoIE_batch_test + the forward of
 *                       validation.py:187-189; nais_topk_rows then is validation.py:190. S is an
 *                       exact-fp32 MFMA product per (32 history entries, 32 candidates) tile, the
 *                       history staged in LDS chunks (any h), any embed_dim 1..256. Every listed
 *                       user's history POIs must be rows of the table (rowmap, num_items).
 *   nais_geoie_forward  out[i] for rows (user[i], target[i], hist[i*hist_ld + 0..n),
 *                       distances[i*dist_ld + 0..n) float32): the tensors GeoIE.forward receives
 *                       (model.py:785), evaluated with the arithmetic and summation order of
 *                       nais_geoie_score, so a catalog winner re-scored here has the same bits.
 * num_pois < 2^24 (NAIS_E_UNSUPPORTED above).
 */
typedef struct nais_geoie_params {
  int32_t embed_dim;            /* D, 1..256                                                  */
  int64_t num_users;            /* rows of user_pref                                          */
  int64_t num_pois;             /* P = rows of the three POI tables                           */
  float a, b;                   /* the power law f = a * d ** b (model.py:763-764, :799)      */
  const float* user_pref;       /* UserPreference.weight    [num_users, D]  model.py:769      */
  const float* poi_pref;        /* PoiPreference.weight     [P, D]          model.py:770      */
  const float* geo_influence;   /* GeoInfluence.weight      [P, D]          model.py:771      */
  const float* geo_suscept;     /* GeoSusceptibility.weight [P, D]          model.py:772      */
} nais_geoie_params_t;

int32_t nais_geoie_table(const double* coords, const double* dist_mat, int64_t num_pois,
                         const int64_t* items, int64_t num_items, int64_t col0, int64_t cols,
                         float a, float b, float* f, int64_t ld, void* stream);
int32_t nais_geoie_score(const nais_geoie_params_t* params, const int64_t* indptr,
                         const int64_t* indices, const int32_t* users, int32_t num_users,
                         const int32_t* rowmap, const float* f, int64_t ld, int64_t num_items,
                         int64_t col0, int64_t cols, float* scores, int64_t score_ld,
                         int64_t score_col0, int32_t* nan_count, void* stream);
int32_t nais_geoie_forward(const nais_geoie_params_t* params, const int64_t* user,
                           const int64_t* target, const int64_t* hist, int64_t b, int64_t n,
                           int64_t hist_ld, const float* distances, int64_t dist_ld, float* out,
                           void* stream);

/* ---------------------------------------------------------------------------------------------
 * GeoIE training (run.py:687-715, model.py:785-828, batches.py:204-242; DESIGN.md "GeoIE training").
 * One batch is one user u: hist[h] = the user's positives in shuffled order, b = h * (1 + num_ng)
 * rows target[b] = [pos_i, neg_i1 .. neg_i,num_ng], labels 1 / 0, freq[b] int64, distances[b, h]
 * float32 = dist_mat[target_i][hist_j]. With the symbols of the GeoIE block above, c_i = target[i]:
 *   p_i   = sigmoid(UserPreference[u] . PoiPreference[c_i] + (sum_j S_i[j] f_ij) / h)
 *   w_i   = 1 + log(float32(1 + freq_i * 10^10))                             (model.py:812)
 *   L     = sum_i -w_i (label_i log(p_i + 1e-10) + (1 - label_i) log(1 - p_i + 1e-10))   (:816-828)
 *   d_i   = -w_i (label_i / (p_i + 1e-10) - (1 - label_i) / (1 - p_i + 1e-10)) p_i (1 - p_i)
 *           -- the composed form autograd produces, NOT w (p - label): where p_i rounds to exactly
 *           0 or 1 the reference's gradient is 0
 *   dUserPreference[u]        = sum_i d_i PoiPreference[c_i]
 *   dPoiPreference[c_i]       = d_i UserPreference[u]
 *   dGeoSusceptibility[c_i][e] = (d_i / h) sum_j Gr[e][j] f_ij
 *   dflat[e*h + j]            = sum_i (d_i / h) f_ij GeoSusceptibility[c_i][e], which is the
 *                               gradient of GeoInfluence[hist[(e*h+j) / D]][(e*h+j) % D]
 *   torch.optim.SGD (run.py:687, no momentum): g' = g + weight_decay p; p -= lr g'. With
 *   weight_decay == 0 only the touched rows change (1 user row, the b target rows of PoiPreference
 *   and GeoSusceptibility, the h history rows of GeoInfluence), every other row stays bit-identical;
 *   otherwise every element of the four tables moves, the untouched rows by one dense pass.
 *
 *   nais_geoie_make_train_batch  get_GeoIE_batch (batches.py:204-242) on the device. hist / target /
 *       labels as nais_make_train_batch (same negative distribution; h * (1 + num_ng) <= num_pois),
 *       freq[i] = int64(data[indptr[user] + i / (1 + num_ng)]) -- attached by CSR POSITION while
 *       the positives are shuffled, as batches.py:238-239 -- and distances[i*dist_ld + j] from
 *       exactly one source, as nais_geoie_table derives them: coords [P, 2] float64 (powerLaw.dist
 *       in float64, clamped to [0.01, 100], cast) or dist_mat [P, P] float64 read at
 *       [target][hist] and cast. data = the CSR values as float64. *err is set to 1 if h disagrees
 *       with indptr.
 *   nais_geoie_train_step  replaces run.py:705-715 for one batch: forward, loss_function,
 *       backward and the SGD step, in place on the four tables of `params` (written through for
 *       this call). *loss_sum += L; *bad_rows += rows whose loss term is not finite (the update
 *       still goes through: the reference only prints, model.py:820-826); pred[b] (optional) = p.
 *       grads (optional, any member NULL): the row gradients, in batch order. stamp_target /
 *       stamp_hist: [P] int32 each, zero-initialised once, `tag` a value not used by an earlier
 *       step (the caller's step counter, as nais_adagrad_state_t's stamps): they mark the rows the
 *       step touches, and detect a repeated target or history entry or an id outside [0, P),
 *       which sets *err (1 repeat, 2 range). While *err is non-zero NO table is written -- a
 *       repeat is never applied half-summed -- so the caller checks and clears it. Any embed_dim
 *       1..256, h >= 1, b >= 1 (b need not be h * (1 + num_ng)). Exact-fp32 MFMA products; the
 *       summation order differs from nais_geoie_forward's, so pred agrees with it to rounding,
 *       not bitwise.
 *   nais_sgd  the dense pass: p -= lr (g + weight_decay p) for every row of a [rows, dim] tensor
 *       whose stamp is not `tag` (stamp may be NULL) and that is not skip_row (-1: none); grad may
 *       be NULL (zero). Nothing is written while *err (optional) is non-zero.
 */
typedef struct nais_geoie_train_grads {
  float* user_pref;             /* [D]     dUserPreference[u]                                  */
  float* poi_pref;              /* [b, D]  dPoiPreference[target[i]]                           */
  float* geo_suscept;           /* [b, D]  dGeoSusceptibility[target[i]]                       */
  float* geo_influence;         /* [h, D]  dGeoInfluence[hist[r]]                              */
} nais_geoie_train_grads_t;

int32_t nais_geoie_make_train_batch(const int64_t* indptr, const int64_t* indices,
                                    const double* data, int64_t user, int64_t h, int64_t num_pois,
                                    int32_t num_ng, uint64_t seed, const double* coords,
                                    const double* dist_mat, int64_t* hist, int64_t* target,
                                    float* labels, int64_t* freq, float* distances, int64_t dist_ld,
                                    int32_t* err, void* stream);
size_t nais_geoie_train_step_workspace_size(const nais_geoie_params_t* params, int64_t b, int64_t h);
int32_t nais_geoie_train_step(const nais_geoie_params_t* params, int64_t user, const int64_t* hist,
                              int64_t h, const int64_t* target, const float* labels,
                              const int64_t* freq, int64_t b, const float* distances,
                              int64_t dist_ld, float lr, float weight_decay, int32_t* stamp_target,
                              int32_t* stamp_hist, int32_t tag, float* loss_sum, int32_t* bad_rows,
                              int32_t* err, float* pred, const nais_geoie_train_grads_t* grads,
                              void* workspace, size_t workspace_bytes, void* stream);
int32_t nais_sgd(float* param, const float* grad, int64_t rows, int32_t dim, float lr,
                 float weight_decay, const int32_t* stamp, int32_t tag, int64_t skip_row,
                 const int32_t* err, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BPR (model.py:587-620; DESIGN.md "BPR"): matrix factorisation, score(u, c) = embed_user[u] .
 * embed_item[c] in fp32. Both kernels below form that dot product as ONE fmaf chain over
 * e = 0, 1, ..., D - 1 from +0 (the scorer on v_mfma_f32_32x32x2_f32, which is that chain), fold
 * -0 into +0 and report every NaN as the quiet NaN 0x7FC00000, so the same (u, c) has the same
 * bits from both.
 *
 *   nais_bpr_forward     out_i[t] = score(user[t], item_i[t]), out_j[t] = score(user[t], item_j[t])
 *                        for t < n: model.py:613-618. item_j / out_j may both be NULL (the
 *                        evaluation calls the model with item_i == item_j, validation.py:144).
 *                        Bad shapes and pointers return NAIS_E_*; ids are device data, so a row
 *                        whose user or item id is outside the tables reads nothing and is NaN.
 *   nais_bpr_score_topk  replaces the user loop of validation.py:138-147: for users[num_users]
 *                        (int32 ids) and the CSR (indptr, indices; rows ascending) the k <= 256
 *                        best candidates of [0, P) \ history(u), as keys in the format of
 *                        nais_pair_gather_topk: ordered(score) << 32 | (0xFFFFFFFF - poi), sorted
 *                        descending in keys[slot*k ...] with kcount[slot] of them valid (NaN first,
 *                        ties by ascending POI id; a user with an empty history has all P
 *                        candidates). nais_topk_keys_finish turns them into ids and scores. No
 *                        score is written to memory: each user keeps the key of its k-th best
 *                        (tau) and only candidates that beat it are kept -- one float compare
 *                        per score, then the whole key for the few that pass. Survivors are
 *                        looked up in the history when the user's buffer is compacted, not
 *                        before they are buffered; tau is taken after that, so a history POI
 *                        never sets it.
 *                        num_chunks: column chunks the catalog is split into (0: chosen from the
 *                        shape); the keys do not depend on it. workspace: of
 *                        nais_bpr_score_topk_workspace_size(params, num_users, k, num_chunks) bytes
 *                        (0 for one chunk; may then be NULL).
 * embed_dim 1..256, num_pois < 2^24 (NAIS_E_UNSUPPORTED otherwise).
 */
typedef struct nais_bpr_params {
  int32_t embed_dim;            /* D, 1..256                                                  */
  int64_t num_users;            /* rows of embed_user                                         */
  int64_t num_pois;             /* P = rows of embed_item                                     */
  const float* embed_user;      /* embed_user.weight [num_users, D]   model.py:596            */
  const float* embed_item;      /* embed_item.weight [P, D]           model.py:597            */
} nais_bpr_params_t;

int32_t nais_bpr_forward(const nais_bpr_params_t* params, const int64_t* user,
                         const int64_t* item_i, const int64_t* item_j, int64_t n, float* out_i,
                         float* out_j, void* stream);
size_t nais_bpr_score_topk_workspace_size(const nais_bpr_params_t* params, int32_t num_users,
                                          int32_t k, int32_t num_chunks);
int32_t nais_bpr_score_topk(const nais_bpr_params_t* params, const int64_t* indptr,
                            const int64_t* indices, const int32_t* users, int32_t num_users,
                            int32_t k, int32_t num_chunks, uint64_t* keys, int32_t* kcount,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BPR training (run.py:490-509, batches.py:6-22; DESIGN.md "BPR"). A batch is n triples
 * (user[t], item_i[t], item_j[t]): a positive and a negative POI of one user. With U = embed_user,
 * I = embed_item, all in fp32:
 *   x_t = U[u_t] . I[i_t] - U[u_t] . I[j_t];  s_t = sigmoid(x_t);  L = -sum_t log s_t   (run.py:506)
 *   g_t = (-1 / s_t) * ((1 - s_t) * s_t)   -- in that order, the composed form autograd produces
 *         (log, then sigmoid): where s_t rounds to 0 the loss is inf and g_t is NaN, as the
 *         reference's; it is NOT -(1 - s_t)
 *   dU[u_t] += g_t (I[i_t] - I[j_t]);  dI[i_t] += g_t U[u_t];  dI[j_t] -= g_t U[u_t]
 *   from the pre-step tables; users and items repeat across triples and every repeat is summed
 *   before the row's one update p -= lr (grad + weight_decay p) (torch.optim.SGD, no momentum,
 *   run.py:481-482). With weight_decay == 0 an untouched row stays bit-identical; otherwise every
 *   element of both tables moves, the untouched rows by nais_sgd's dense pass.
 *
 *   nais_bpr_make_train_batch  get_BPR_batch (batches.py:6-22) on the device for users[num_users]
 *       (int64 ids into a CSR of num_rows users; an id outside sets *err |= 2): user u with h
 *       history POIs gives h triples at user / item_i / item_j
 *       [offsets[slot] ...] (offsets: the caller's exclusive prefix sum of the h's): the positives
 *       in CSR order, the negatives h distinct POIs drawn uniformly without replacement from
 *       outside the history (the sampler of nais_make_train_batch, seeded per user from `seed`).
 *       h > P - h sets *err to 1 and writes nothing for that user (the reference's negative[i]
 *       raises there, batches.py:14-16). Triples come out grouped by user: the reference's final
 *       random.shuffle(batch) (batches.py:17) only changes the order in which the step sums them.
 *   nais_bpr_train_step  replaces run.py:504-509 for one batch, in place on both tables of
 *       `params` (written through for this call). *loss_sum += L. Optional outputs: pred_i /
 *       pred_j [n] (the two dots), g [n], grads (dense [num_users, D] / [P, D], zeroed by the
 *       caller; only touched rows are written). stamp_user [num_users] / stamp_item [P]: int32,
 *       zero-initialised once, `tag` a value no earlier step used; they mark the touched rows. An
 *       id outside its table sets *err |= 2, and while *err is non-zero no table is written.
 *       Deterministic: no float atomics. item_order [2n] int64 is a STABLE sort permutation of the
 *       2n ids item_i[0..n) ++ item_j[0..n) (entry x < n is item_i[x], else item_j[x - n]);
 *       user_order [n] the same for user[] (NULL: user[] is already grouped, as
 *       nais_bpr_make_train_batch emits it). One wave per run of equal ids sums the run in that
 *       order, so equal inputs give equal bits. Entries outside [0, 2n) / [0, n) are skipped.
 */
typedef struct nais_bpr_train_grads {
  float* embed_user;            /* [num_users, D] dense dU, caller-zeroed                      */
  float* embed_item;            /* [P, D]         dense dI, caller-zeroed                      */
} nais_bpr_train_grads_t;

int32_t nais_bpr_make_train_batch(const int64_t* indptr, const int64_t* indices,
                                  int64_t num_rows, const int64_t* users, const int64_t* offsets, int64_t num_users,
                                  int64_t num_pois, uint64_t seed, int64_t* user, int64_t* item_i,
                                  int64_t* item_j, int32_t* err, void* stream);
size_t nais_bpr_train_step_workspace_size(const nais_bpr_params_t* params, int64_t n);
int32_t nais_bpr_train_step(const nais_bpr_params_t* params, const int64_t* user,
                            const int64_t* item_i, const int64_t* item_j, int64_t n,
                            const int64_t* user_order, const int64_t* item_order, float lr,
                            float weight_decay, int32_t* stamp_user, int32_t* stamp_item,
                            int32_t tag, float* loss_sum, int32_t* err, float* pred_i,
                            float* pred_j, float* g, const nais_bpr_train_grads_t* grads,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * New1 (model.py:830-925; DESIGN.md "New1"): Q / K / V attention over the user's history. With
 * t = [embed_target[c] | embed_region[treg]] (d floats), h_j the same for history item j,
 * q = attn_Q t, K_j = attn_K h_j, V_j = attn_V h_j and Kflat the row's contiguous [n, d] key buffer,
 *   a_j' = sum_e q[e] * Kflat[e * n + j'] / sqrtf(d)   (model.py:896-897: key_emb is RESHAPED to
 *          [d, n], not transposed; this needs hidden == embed_dim)
 *   e_j  = expf(a_j) * [hist_j != c]                   (model.py:899-901; no max-subtraction)
 *   pred = sum_j sum_k (e_j / powf(sum_j e_j, beta) * V_j[k] + r_j * h_j[k]) * t[k];  out = sigmoid(pred)
 * e_j = inf, all e_j = 0 and a row whose only history item is its target give NaN, as the
 * reference's. An empty history gives 0.5. At n == 1 the reference's squeeze() calls mix the rows
 * of the batch (model.py:898-901); here n == 1 is the per-row formula above.
 *
 *   nais_new1_forward    out[b] for rows (hist[row * hist_row_stride + j], hist_region likewise,
 *                        target[row], target_region[row]; int64 ids) and visit_rate[n] shared by
 *                        the rows: model.py:861-918. hist_row_stride 0 shares one history between
 *                        the rows (batches.py:355 repeats it). One wave per row: the general path.
 *                        Ids are device data: a row with an id outside its table is NaN.
 *   nais_new1_catalog_tables  T[p] = [embed_target[p] | embed_region[region_of[p]]], Q = T attn_Q^T,
 *                        K = T attn_K^T, V = T attn_V^T, each [P, d] and caller-owned: what
 *                        model.py:879-893 recompute for every row, once per POI
 *                        (v_mfma_f32_32x32x2_f32: the fmaf chain over k ascending). A region
 *                        outside the table makes that POI's rows NaN.
 *   nais_new1_score_topk replaces the user loop of validation.py:212-230 (batches.py:348-383):
 *                        for users[num_users] (int32 ids) and the CSR (indptr, indices; rows
 *                        ascending) with visit_rate[nnz] (r_j per CSR entry, batches.py:358-359 cast
 *                        to float) the k <= 256 best candidates of [0, P) \ history(u) by
 *                        sigmoid(pred), as keys for nais_topk_keys_finish (see nais_bpr_score_topk:
 *                        NaN first, ties by ascending POI id, -0 folded into +0). No score row is
 *                        written. Its sums over j run in another order than nais_new1_forward's
 *                        (and it forms sum_j e_j V_j.t before dividing by the power), so the two
 *                        agree to rounding, not bit for bit; where sum_j e_j overflows with every
 *                        e_j finite the scorer gives NaN if sum_j e_j V_j.t overflowed too.
 *                        num_chunks / workspace: as nais_bpr_score_topk.
 * embed_dim even, 2..256; hidden == embed_dim; num_pois < 2^24 (NAIS_E_UNSUPPORTED otherwise).
 */
typedef struct nais_new1_params {
  int32_t embed_dim;            /* d = embed_size (both halves concatenated)                   */
  int32_t hidden;               /* attn_Q / attn_K out_features; must equal embed_dim          */
  int64_t num_pois;             /* P = rows of embed_target                                    */
  int64_t num_regions;          /* R = rows of embed_region                                    */
  float beta;                   /* exponent of the softmax denominator (model.py:903)          */
  const float* embed_target;    /* embed_target.weight [P, d/2]       model.py:837             */
  const float* embed_region;    /* embed_region.weight [R, d/2]       model.py:839             */
  const float* attn_q;          /* attn_Q.weight [hidden, d]          model.py:846             */
  const float* attn_k;          /* attn_K.weight [hidden, d]          model.py:847             */
  const float* attn_v;          /* attn_V.weight [d, d]               model.py:848             */
} nais_new1_params_t;

int32_t nais_new1_forward(const nais_new1_params_t* params, const int64_t* hist,
                          int64_t hist_row_stride, const int64_t* target,
                          const int64_t* hist_region, const int64_t* target_region,
                          const float* visit_rate, int64_t b, int64_t n, float* out, void* stream);
int32_t nais_new1_catalog_tables(const nais_new1_params_t* params, const int64_t* region_of,
                                 float* T, float* Q, float* K, float* V, void* stream);
size_t nais_new1_score_topk_workspace_size(const nais_new1_params_t* params, int32_t num_users,
                                           int32_t k, int32_t num_chunks);
int32_t nais_new1_score_topk(const nais_new1_params_t* params, const float* T, const float* Q,
                             const float* K, const float* V, const int64_t* indptr,
                             const int64_t* indices, const float* visit_rate, const int32_t* users,
                             int32_t num_users, int32_t k, int32_t num_chunks, uint64_t* keys,
                             int32_t* kcount, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * New1 training (run_new.py:107-137, 389-410, model.py:861-918; DESIGN.md "New1 training"). One
 * batch is one user (trainDataset.__getitem__, run_new.py:107-137; NOT batches.get_New1_batch,
 * which shuffles the history after the visit rates are formed): hist[n] = the user's CSR row in
 * ascending order, visit_rate[n] = data / colsum[hist] (a float64 quotient cast to float32),
 * b = n * (1 + num_ng) rows target[b] = [pos_i, neg_i1 .. neg_i,num_ng], labels 1 / 0, regions
 * region_of[.]. With the symbols of the New1 block above, T / Q the b target rows' concatenated
 * embeddings and attn_Q projections, H / K / V the same for the history and Ks[e][j] =
 * Kflat[e * n + j] (the [n, d] key buffer read as [d, n], model.py:896):
 *   A = Q Ks / sqrtf(d)            E[c][j] = expf(A[c][j]) * [hist_j != target_c]
 *   S_c = sum_j E[c][j]            M = T V^T          g = sum_j r_j h_j
 *   N_c = sum_j E[c][j] M[c][j]    pred_c = N_c / powf(S_c, beta) + t_c . g
 *   x_c = sigmoid(pred_c)
 *   loss = mean_c -(y_c max(log x_c, -100) + (1 - y_c) max(log(1 - x_c), -100))   (nn.BCELoss)
 *   d_c = (x_c - y_c) / max((1 - x_c) x_c, 1e-12) / b * (1 - x_c) x_c
 *         -- the composed form autograd produces (BCELoss's backward, then the sigmoid's), NOT
 *         (x - y) / b: a label-0 row with x == 1.0f has d = 0, and a label-1 row whose
 *         x (1 - x) is below 1e-12 has |d| < 1 / b
 *   dM[c][j] = d_c E[c][j] S_c^-beta      dA[c][j] = dM[c][j] (M[c][j] - beta N_c / S_c)
 *   dQ = dA Ks^T / sqrtf(d)   dKs = Q^T dA / sqrtf(d) -> dKflat[e * n + j] = dKs[e][j]
 *   dV = dM^T T               dg = sum_c d_c t_c
 *   dT = dM V + d g^T + dQ Wq             dH = dK Wk + dV Wv + r dg^T
 *   dWq = dQ^T T    dWk = dK^T H    dWv = dV^T H
 *   dT / dH scatter into embed_target (the left halves; a positive's row receives its dT and its
 *   dH share) and embed_region (the right halves; up to b + n shares per row, summed with the
 *   targets in batch order first, then the history).
 *   torch.optim.Adam(lr, betas, eps, weight_decay) (run_new.py:389) over EVERY element of the five
 *   tensors -- dense: a row touched once keeps moving through exp_avg on later steps --
 *     g' = g + wd p;  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2
 *     p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *   the scalars formed in double as Python forms them, then cast to float.
 *
 *   nais_new1_make_train_batch  trainDataset.__getitem__ on the device for one user. rate[nnz] =
 *       the per-entry float64 visit rates (data / colsum), region_of[P] the POI -> region map. The
 *       negatives are nais_make_train_batch's: the first n * num_ng members of the seeded order
 *       of [0, P) that are outside the history (the distinct-subset sampler of nais_sampler.h, the
 *       same seed derivation). *err |= 1, and nothing is written, if n disagrees with indptr or
 *       n * num_ng > P - n.
 *   nais_new1_train_step  replaces run_new.py:403-410 for one batch: forward, loss_func, backward
 *       and optimizer.step(), in place on the five tensors of `params` (written through for this
 *       call) and on `state`. t = the step number, 1 for the first. *loss_sum (a double: an epoch's
 *       sum is not rounded to float at every user) += loss; pred[b]
 *       (optional) = x. grads (optional, any member NULL) receives the five DENSE gradients before
 *       weight decay, zero outside the touched rows (every element is written). stamp_target /
 *       stamp_hist: [P] int32 each, zero-initialised once, `tag` a value no earlier step used;
 *       they mark the touched rows (the rows' slots live in the workspace). *err |= 2 for an id
 *       outside its table, 1 for a repeated target or history entry, 4 for a NaN prediction (the
 *       reference raises inside BCELoss there). While *err is non-zero NEITHER parameters NOR
 *       state are written, so the caller checks and clears it. n >= 2 (at n = 1 the reference's
 *       positive row has no unmasked item and its step raises), b >= 1. No host sync; no float
 *       atomics: the same batch from the same state gives the same bits. Exact-fp32 MFMA
 *       products; the summation order differs from nais_new1_forward's.
 */
typedef struct nais_new1_adam_state {
  float* m_embed_target;        /* exp_avg / exp_avg_sq of embed_target.weight [P, d/2]        */
  float* v_embed_target;
  float* m_embed_region;        /* ... of embed_region.weight [R, d/2]                         */
  float* v_embed_region;
  float* m_attn_q;              /* ... of attn_Q.weight [d, d]                                 */
  float* v_attn_q;
  float* m_attn_k;              /* ... of attn_K.weight [d, d]                                 */
  float* v_attn_k;
  float* m_attn_v;              /* ... of attn_V.weight [d, d]                                 */
  float* v_attn_v;
} nais_new1_adam_state_t;

typedef struct nais_new1_train_grads {
  float* embed_target;          /* [P, d/2] dense                                              */
  float* embed_region;          /* [R, d/2] dense                                              */
  float* attn_q;                /* [d, d]                                                      */
  float* attn_k;                /* [d, d]                                                      */
  float* attn_v;                /* [d, d]                                                      */
} nais_new1_train_grads_t;

int32_t nais_new1_make_train_batch(const int64_t* indptr, const int64_t* indices,
                                   const double* rate, const int64_t* region_of, int64_t user,
                                   int64_t n, int64_t num_pois, int32_t num_ng, uint64_t seed,
                                   int64_t* hist, int64_t* hist_region, float* visit_rate,
                                   int64_t* target, int64_t* target_region, float* labels,
                                   int32_t* err, void* stream);
size_t nais_new1_train_step_workspace_size(const nais_new1_params_t* params, int64_t b, int64_t n);
int32_t nais_new1_train_step(const nais_new1_params_t* params, const int64_t* hist,
                             const int64_t* hist_region, const float* visit_rate,
                             const int64_t* target, const int64_t* target_region,
                             const float* labels, int64_t b, int64_t n, double lr,
                             double weight_decay, double beta1, double beta2, double eps,
                             int64_t t, const nais_new1_adam_state_t* state, int32_t* stamp_target,
                             int32_t* stamp_hist, int32_t tag, double* loss_sum, int32_t* err,
                             float* pred, const nais_new1_train_grads_t* grads, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * New2 (model.py:927-1027, run_new.py:173-264, 468-584; DESIGN.md "New2"): New1 plus a geographic
 * weight per (row, history item). With New1's symbols, w = embed_dist[uid] (R floats), b rows and
 * n history items:
 *   G[j]      = sum_c w[target_region[c]] * w[hist_region[c][j]]   (model.py:1008: a [b] @ [b, n]
 *               product; it sums over THE BATCH and is the same for every row)
 *   lambda[j] = -1 / (relu(G[j]) + 1)
 *   D'[c][j]  = dist[c * n + j]     (dist arrives as [n, b] = history rows x target columns and is
 *               RESHAPED to [b, n], not transposed: flat index f = c n + j holds the distance of
 *               history item f div b and target f mod b)
 *   geo[c][j] = expf(lambda[j] * D'[c][j])                         (not masked)
 *   pred_c    = sum_j (e_cj / powf(S_c, beta) + geo[c][j]) (V_j . t_c)  +  t_c . sum_j r_j h_j
 * Both oddities are the reference's and are reproduced. NaN rules, n == 0 and n == 1 as New1.
 *
 *   nais_new2_forward    out[b] for rows as nais_new1_forward's, dist[n * b] float32 read flat,
 *                        uid a host value. lambda_work[n] is scratch: lambda[j] is reduced over
 *                        the batch first, in a fixed order (no float atomics: same input, same
 *                        bits), then one wave per row. A row with an id outside its table is NaN;
 *                        a uid or a region id outside embed_dist makes G, so every row, NaN.
 *   nais_new2_score_topk the evaluation loop of run_new.py:551-570 (testDataset2.__getitem__,
 *                        run_new.py:242-264): nais_new1_score_topk with the geo term. The batch of
 *                        user u is its complement [0, P) \ history(u) in ascending POI id, b = P - n
 *                        rows that share the history, so G[j] = w[region_of[hist_j]] * sigma_u with
 *                        sigma_u = sum over the candidates of w[region_of[c]] (per-region counts,
 *                        float64, rounded once), and the row of the c-th candidate BY POSITION
 *                        pairs history item (c n + j) div b with the candidate at POSITION
 *                        (c n + j) mod b. T, Q, K, V are nais_new1_catalog_tables' (call it with
 *                        &params->base). The distances come from exactly one of
 *                          coords   [P, 2] float64 (lat, lng in degrees): the haversine package's
 *                                   formula evaluated per pair on the device in float64, in its
 *                                   operation order, kilometres (mean radius 6371.0088), rounded
 *                                   to float32; nothing P x P is allocated;
 *                          dist_mat [P, P] float32, row-major, the caller's.
 *                        users[.] indexes the CSR rows and embed_dist (a user outside embed_dist
 *                        scores NaN). Keys, order rules, num_chunks as nais_new1_score_topk; the
 *                        workspace (always needed) also holds the per-region counts and the
 *                        per-POI coordinate table.
 * nais_new2_params_t embeds New1's struct first, so &params->base is a nais_new1_params_t.
 */
typedef struct nais_new2_params {
  nais_new1_params_t base;      /* New1's fields (model.py:935-946)                             */
  int64_t num_users;            /* U = rows of embed_dist                                       */
  const float* embed_dist;      /* embed_dist [U, R]                  model.py:938              */
} nais_new2_params_t;

int32_t nais_new2_forward(const nais_new2_params_t* params, const int64_t* hist,
                          int64_t hist_row_stride, const int64_t* target,
                          const int64_t* hist_region, const int64_t* target_region,
                          const float* visit_rate, const float* dist, int64_t uid, int64_t b,
                          int64_t n, float* lambda_work, float* out, void* stream);
size_t nais_new2_score_topk_workspace_size(const nais_new2_params_t* params, int32_t num_users,
                                           int32_t k, int32_t num_chunks);
int32_t nais_new2_score_topk(const nais_new2_params_t* params, const float* T, const float* Q,
                             const float* K, const float* V, const int64_t* region_of,
                             const int64_t* indptr, const int64_t* indices,
                             const float* visit_rate, const double* coords, const float* dist_mat,
                             const int32_t* users, int32_t num_users, int32_t k,
                             int32_t num_chunks, uint64_t* keys, int32_t* kcount, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training step of NAIS_basic on one get_NAIS_batch batch (batches.py:24-50):
 * b rows (target[b], int64 POI ids) that all share ONE history hist[n] (int64, the user's positives;
 * the reference repeats it b times, batches.py:30). Replaces, for this batch shape,
 *   prediction = model(user_history, train_data)   (run.py:103; model.py:40-89 in train mode)
 *   loss.backward()                                (run.py:105; BCELoss model.py:21)
 * NAIS_VARIANT_BASIC; embed_dim up to 256, any hidden (fused MFMA kernels at embed_dim in
 * {8,16,32,64}, hidden <= 64; a general kernel up to 128; the generic-shape kernels above -- see
 * nais_train_forward_ex for the region variants).
 *
 * Dropout (nn.Dropout(dropout_p), model.py:22,71) keeps hidden unit i of pair (row c, item j) iff
 * a counter hash of (seed, c*n + j, i) is >= dropout_p * 2^32 and scales kept units by 1/(1-p);
 * dropout_p = 0 is eval-mode arithmetic. nais_dropout_mask() materialises the same mask
 * (uint8 [b, n, hidden], 1 = kept) for tests.
 *
 * nais_train_forward: pred[b] = sigmoid(logit) (model.py:55); saved[2b] = (S, N) per row for the
 *   backward; optional nan_count (+= rows whose logit is NaN, model.py:50-54).
 * nais_train_backward: given grad_pred[b] = dL/dpred (e.g. from BCELoss's backward), ADDS the
 *   gradients into grad_embed_history / grad_embed_target ([num_pois, embed_dim], dense, rows by
 *   POI id; repeated ids are summed with fp32 atomics), grad_w1 [hidden, embed_dim], grad_b1
 *   [hidden], grad_w2 [hidden]. Same params, hist, target, dropout_p and seed as the forward.
 *   Both calls take a workspace of nais_train_workspace_size(params, b, n) bytes (the forward's
 *   may be reused by the backward once the forward has run).
 * -------------------------------------------------------------------------------------------- */
size_t nais_train_workspace_size(const nais_params_t* params, int64_t b, int64_t n);

int32_t nais_train_forward(const nais_params_t* params, const int64_t* hist, int64_t n,
                           const int64_t* target, int64_t b, float dropout_p, uint64_t seed,
                           float* pred, float* saved, int32_t* nan_count, void* workspace,
                           size_t workspace_bytes, void* stream);

int32_t nais_train_backward(const nais_params_t* params, const int64_t* hist, int64_t n,
                            const int64_t* target, int64_t b, float dropout_p, uint64_t seed,
                            const float* pred, const float* saved, const float* grad_pred,
                            float* grad_embed_history, float* grad_embed_target, float* grad_w1,
                            float* grad_b1, float* grad_w2, void* workspace,
                            size_t workspace_bytes, void* stream);

int32_t nais_dropout_mask(uint64_t seed, int64_t b, int64_t n, int32_t hidden, float dropout_p,
                          uint8_t* out, void* stream);

/*
 * The same training forward / backward for every NAIS variant (NAIS_basic, NAIS_regionEmbedding,
 * NAIS_region_distance_Embedding, NAIS_distance_Embedding; run.py:91-280, 365-430) and any
 * embed_dim / hidden up to 128 (run.py's
 * defaults are factor_num = hidden_dim = 128). NAIS_basic at embed_dim in {8,16,32,64}, hidden <= 64
 * runs the fused MFMA kernels above; everything else a general kernel with the same math and the
 * same dropout draws. The region variants read full rows [embed_history | embed_region[region]]:
 *   side->hist_region [n], side->target_region [b]  (regions of the history items / target rows,
 *   get_NAIS_batch_region, batches.py:67-108); region_distance also side->target_lat_long
 *   [b, n, 2] f32, row stride latlon_ld (run.py:240-245), x100 before dist_layer (model.py:265).
 * NAIS_distance_Embedding reads basic rows and side->target_lat_long (x1000, model.py:369).
 * The two distance variants have no dropout (model.py:268, 369-371): pass dropout_p = 0.
 * Gradients are ADDED into grads (dense, fp32 atomics for repeated ids); embed_region and
 * dist_w / dist_b are required for the variants that have them. nais_train_forward / _backward
 * above are these with side = NULL (NAIS_basic only). Workspace: nais_train_workspace_size().
 */
typedef struct nais_train_side {
  const int64_t* hist_region;     /* [n]                                                        */
  const int64_t* target_region;   /* [b]                                                        */
  const float* target_lat_long;   /* [b, n, 2] f32 (region_distance)                           */
  int64_t latlon_ld;              /* row stride of target_lat_long in elements (>= 2n)         */
  /* optional u cache (general kernels, nais_train_ucache_size() > 0): with ucache_bytes >= that
   * size, nais_train_forward_ex leaves every pair's post-dropout W1 x + b1, h . t and attention
   * logit here and nais_train_backward_ex of the SAME batch, parameters and seed reads them instead
   * of recomputing the forward (a third of its MFMA work); NULL = recompute */
  float* ucache;
  uint64_t ucache_bytes;
} nais_train_side_t;

/* Bytes of the u cache for (params, b, n): 0 where the fused kernels run (they keep no cache) or
 * above 1 GiB (the backward then recomputes). */
size_t nais_train_ucache_size(const nais_params_t* params, int64_t b, int64_t n);

typedef struct nais_train_grads {
  float* embed_history;           /* [P, item_dim]  */
  float* embed_target;            /* [P, item_dim]  */
  float* embed_region;            /* [R, region_dim] (region variants)                          */
  float* w1;                      /* [H, din]       */
  float* b1;                      /* [H]            */
  float* w2;                      /* [H]            */
  float* dist_w;                  /* [2, 2] (region_distance)                                   */
  float* dist_b;                  /* [2]            */
} nais_train_grads_t;

int32_t nais_train_forward_ex(const nais_params_t* params, const nais_train_side_t* side,
                              const int64_t* hist, int64_t n, const int64_t* target, int64_t b,
                              float dropout_p, uint64_t seed, float* pred, float* saved,
                              int32_t* nan_count, void* workspace, size_t workspace_bytes,
                              void* stream);
int32_t nais_train_backward_ex(const nais_params_t* params, const nais_train_side_t* side,
                               const int64_t* hist, int64_t n, const int64_t* target, int64_t b,
                               float dropout_p, uint64_t seed, const float* pred,
                               const float* saved, const float* grad_pred,
                               const nais_train_grads_t* grads, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused training step of NAIS_basic (run.py:101-109 in one call; embed_dim / hidden up to 128,
 * the fused MFMA kernels where they apply, else the general ones): forward, BCELoss (model.py:21) added into
 * *loss_sum (device float, mean over the b rows -- run.py's train_loss accumulates loss.item()),
 * backward, and torch.optim.Adagrad's update of all five parameters IN PLACE (the params pointers
 * are written). Adagrad state lives in nais_adagrad_state_t; its gradient scratch must be all zero
 * on entry and is left all zero. Rows with a NaN prediction (a single-item history equal to its
 * target, model.py:92-95) are counted into *bad_rows (device int32); while *bad_rows != 0 the
 * update is skipped (the reference's BCELoss raises on such a batch). pred [b] is optional.
 * Workspace: nais_train_step_workspace_size(params, b, n) bytes.
 * -------------------------------------------------------------------------------------------- */
typedef struct nais_adagrad_state {
  float lr, lr_decay, weight_decay, eps;   /* torch.optim.Adagrad arguments (run.py:89)            */
  int64_t step;                            /* step count including this one (torch state['step']) */
  float* sum_embed_history;                /* Adagrad accumulators, shapes of the parameters       */
  float* sum_embed_target;
  float* sum_w1;
  float* sum_b1;
  float* sum_w2;
  float* grad_embed_history;               /* [P, D] zero-maintained gradient scratch              */
  float* grad_embed_target;                /* [P, D]                                               */
  float* grad_small;                       /* [H*din + 2H]: w1 | b1 | w2                           */
  int32_t* stamp_embed_history;            /* [P] row-claim stamps, initialised to 0               */
  int32_t* stamp_embed_target;             /* [P]                                                  */
} nais_adagrad_state_t;

size_t nais_train_step_workspace_size(const nais_params_t* params, int64_t b, int64_t n);

int32_t nais_train_step(const nais_params_t* params, const nais_adagrad_state_t* opt,
                        const int64_t* hist, int64_t n, const int64_t* target, const float* labels,
                        int64_t b, float dropout_p, uint64_t seed, float* loss_sum,
                        int32_t* bad_rows, float* pred, void* workspace, size_t workspace_bytes,
                        void* stream);

/*
 * The same fused step for the region / distance variants (run.py:139-200 NAIS_regionEmbedding,
 * :206-262 NAIS_region_distance_Embedding, :365-430 NAIS_distance_Embedding; batches from
 * get_NAIS_batch_region, batches.py:67-108): side = the batch's region ids / target_lat_long as
 * for nais_train_forward_ex (its ucache fields are ignored: the step keeps its own in the
 * workspace). opt covers embed_history / embed_target (rows of item_dim floats), attn_layer1 (its
 * grad_small block is [hidden * din | hidden | hidden]) and attn_layer2; opt_side the variant's
 * extra parameters, updated densely (torch.optim.Adagrad over model.parameters(), run.py:155):
 * embed_region [num_regions, region_dim] and / or dist_layer (weight [2, 2], bias [2]), each with
 * a zero-maintained gradient scratch. NAIS_basic with side = opt_side = NULL is nais_train_step.
 */
typedef struct nais_adagrad_side {
  float* sum_embed_region;                 /* [num_regions, region_dim] (region variants)          */
  float* grad_embed_region;                /* same shape, zero-maintained                          */
  float* sum_dist_w;                       /* [4] (distance variants)                              */
  float* sum_dist_b;                       /* [2]                                                  */
  float* grad_dist;                        /* [6]: dist_w | dist_b, zero-maintained                */
} nais_adagrad_side_t;

int32_t nais_train_step_ex(const nais_params_t* params, const nais_train_side_t* side,
                           const nais_adagrad_state_t* opt, const nais_adagrad_side_t* opt_side,
                           const int64_t* hist, int64_t n, const int64_t* target, const float* labels,
                           int64_t b, float dropout_p, uint64_t seed, float* loss_sum,
                           int32_t* bad_rows, float* pred, void* workspace, size_t workspace_bytes,
                           void* stream);

/*
 * get_NAIS_batch (batches.py:24-50) for one user on the device: hist [n] = the
 * user's n = indptr[user+1]-indptr[user] positives (CSR rows sorted ascending) in a seeded random
 * order; target / labels [n * (1 + num_ng)] = rows [pos_i, neg_i1 .. neg_i,num_ng], labels 1 / 0.
 * Negatives: distinct, uniform over the POIs not in the history (the reference's shuffle-and-slice
 * distribution; not Python's random stream). *err (optional) is set to 1 if n disagrees with indptr.
 */
int32_t nais_make_train_batch(const int64_t* indptr, const int64_t* indices, int64_t user,
                              int64_t n, int64_t num_pois, int32_t num_ng, uint64_t seed,
                              int64_t* hist, int64_t* target, float* labels, int32_t* err,
                              void* stream);

/*
 * torch.optim.Adagrad's update (run.py:89; lr_decay folded into clr = lr / (1 + (step-1) lr_decay)):
 *   g' = g + weight_decay * p ; state += g' * g' ; p -= clr * g' / (sqrt(state) + eps)
 * nais_adagrad: every element of a tensor of numel floats.
 * nais_adagrad_rows: only rows[num_rows] of a [*, dim] tensor, weight_decay 0. Rows whose
 *   gradient is zero are left bit-identical by the dense update, so this equals nais_adagrad
 *   when `rows` covers every row with a nonzero gradient. Rows are distinct, or sorted with
 *   repeats: an entry equal to the one before it is skipped (each row updated once).
 */
int32_t nais_adagrad(float* param, float* state_sum, const float* grad, int64_t numel, float clr,
                     float weight_decay, float eps, void* stream);
int32_t nais_adagrad_rows(float* param, float* state_sum, const float* grad, int32_t dim,
                          const int64_t* rows, int64_t num_rows, float clr, float eps,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NAIS_H_ */
